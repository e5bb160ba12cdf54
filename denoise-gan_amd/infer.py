"""Denoise every image of a directory with a trained pix2pix generator (the reference's
infer.py:24-83, without its display window).

    python infer.py --image_dir noisy/ --output_dir clean/ --model models/pix2pix.npz

--model is a `Generator.save` export: the .npz of weights and moving statistics beside the .json
that names the width.  Images are read and written with Pillow, as RGB; each keeps its size and
file name.  Whole images are padded to a multiple of 256 by default; --tile T (a multiple of 256)
with --margin M runs T x T tiles with M pixels of context instead, --batch of them per forward.

Deviation from the reference: the generator is fed [-1, 1] (uint8 / 255 * 2 - 1, what it was
trained on, dataloader.py:173-175); the reference's infer.py:55 feeds [0, 1].
"""
import json
import os
from argparse import ArgumentParser

import numpy as np

parser = ArgumentParser()
parser.add_argument("--image_dir", type=str, required=True, help="Directory where images are kept.")
parser.add_argument("--output_dir", type=str, required=True, help="Directory where to write the denoised images.")
parser.add_argument("--model", default="./models/pix2pix.npz", type=str, help="Path to a Generator.save export (.npz).")
parser.add_argument("--tile", default=0, type=int, help="Tile size, a multiple of 256 (0: whole image).")
parser.add_argument("--margin", default=0, type=int, help="Context pixels on each side of a tile.")
parser.add_argument("--pad", default="black", choices=["black", "reflect"], help="Values outside the image.")
parser.add_argument("--batch", default=8, type=int, help="Tiles per forward.")


def load_generator(model_path):
    from dgan.models import Generator
    base = model_path[:-4] if model_path.endswith(".npz") else model_path
    with open(base + ".json") as f:
        meta = json.load(f)
    if meta.get("model") != Generator.kind:
        raise SystemExit(f"{base}.json describes a {meta.get('model')!r}, not a {Generator.kind!r}")
    g = Generator(width=int(meta["width"]))
    g.load_weights(base + ".npz")
    return g


def main(argv=None):
    from PIL import Image
    from dgan.infer import Denoiser
    args = parser.parse_args(argv)
    image_dir = os.path.expanduser(os.path.expandvars(args.image_dir))
    output_dir = os.path.expanduser(os.path.expandvars(args.output_dir))
    model_path = os.path.expanduser(os.path.expandvars(args.model))
    image_paths = [os.path.join(image_dir, x) for x in sorted(os.listdir(image_dir))]
    os.makedirs(output_dir, exist_ok=True)
    denoiser = Denoiser(load_generator(model_path), tile=args.tile or None, margin=args.margin, pad=args.pad,
                        batch=args.batch)
    for image_path in image_paths:
        with Image.open(image_path) as im:
            noisy = np.asarray(im.convert("RGB"), np.uint8)
        clean = denoiser.denoise(noisy)
        out_path = os.path.join(output_dir, os.path.basename(image_path))
        Image.fromarray(clean, "RGB").save(out_path)
        print(f"{image_path} -> {out_path} {clean.shape[1]}x{clean.shape[0]}")


if __name__ == "__main__":
    main()
