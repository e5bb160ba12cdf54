"""Upscale every image of a directory with a trained SR-family generator (the frame loop of the
reference's infer_video.py:73-159 on still images: uint8 -> [-1, 1] -> generator -> clip -> uint8
at `scale` times the size).

    python upscale.py --image_dir low/ --output_dir high/ --model models/fsrgan_generator.npz

--model is a `GraphNetwork.save` export: the .npz of weights and moving statistics.  Its .json
says only "generator", so --arch picks the builder: fsrgan (the reference's default model, x4),
srgan (--scale 2 or 4) or autoencoder (x1, inputs padded to a multiple of 32).  Images are read
and written with Pillow, as RGB, under their file names.  Whole images by default; --tile T with
--margin M runs T x T tiles with M pixels of context (10 cover FastSRGAN's receptive field, 36
SRGAN's), --batch of them per forward.  --fp16 1 runs the 3x3 convs on the mixed_float16 policy;
the fused FastSRGAN blocks stay fp32 (dgan/sr_infer.py).
"""
import os
from argparse import ArgumentParser

import numpy as np

parser = ArgumentParser()
parser.add_argument("--image_dir", type=str, required=True, help="Directory where images are kept.")
parser.add_argument("--output_dir", type=str, required=True, help="Directory where to write the upscaled images.")
parser.add_argument("--model", default="./models/fsrgan_generator.npz", type=str, help="Path to a GraphNetwork.save export (.npz).")
parser.add_argument("--arch", default="fsrgan", choices=["fsrgan", "srgan", "autoencoder"], help="Which generator the weights belong to.")
parser.add_argument("--scale", default=4, type=int, help="Upscale factor (srgan: 2 or 4; fsrgan: 4; autoencoder: 1).")
parser.add_argument("--tile", default=0, type=int, help="Tile size (0: whole image).")
parser.add_argument("--margin", default=0, type=int, help="Context pixels on each side of a tile.")
parser.add_argument("--pad", default="black", choices=["black", "reflect"], help="Values outside the image.")
parser.add_argument("--batch", default=8, type=int, help="Tiles per forward.")
parser.add_argument("--fp16", default=0, type=int, help="Run the conv GEMMs on the mixed_float16 policy.")


def load_network(arch, model_path, scale=4, fp16=False):
    """-> (network, scale, multiple) of a saved generator."""
    from dgan import zoo
    from dgan.sr_models import sr_generator_net
    from dgan.models import default_device
    if arch == "fsrgan":
        graph, scale, multiple = zoo.fsrgan_generator(), 4, 1
    elif arch == "srgan":
        if scale not in (2, 4):
            raise SystemExit(f"srgan upscales by 2 or 4, not {scale}")
        graph, multiple = zoo.srgan_generator(scale=scale), 1
    else:
        graph, scale, multiple = zoo.autoencoder_generator(), 1, 32
    net = sr_generator_net(graph, 0, default_device())
    net.load_weights(model_path)
    if fp16:
        net.conv_math = "fp16"
    return net, scale, multiple


def main(argv=None):
    from PIL import Image
    from dgan.sr_infer import Upscaler
    args = parser.parse_args(argv)
    image_dir = os.path.expanduser(os.path.expandvars(args.image_dir))
    output_dir = os.path.expanduser(os.path.expandvars(args.output_dir))
    model_path = os.path.expanduser(os.path.expandvars(args.model))
    image_paths = [os.path.join(image_dir, x) for x in sorted(os.listdir(image_dir))]
    os.makedirs(output_dir, exist_ok=True)
    net, scale, multiple = load_network(args.arch, model_path, args.scale, bool(args.fp16))
    upscaler = Upscaler(net, scale, multiple=multiple, tile=args.tile or None, margin=args.margin, pad=args.pad,
                        batch=args.batch)
    for image_path in image_paths:
        with Image.open(image_path) as im:
            low = np.asarray(im.convert("RGB"), np.uint8)
        high = upscaler.upscale(low)
        out_path = os.path.join(output_dir, os.path.basename(image_path))
        Image.fromarray(high, "RGB").save(out_path)
        print(f"{image_path} -> {out_path} {high.shape[1]}x{high.shape[0]}")


if __name__ == "__main__":
    main()
