"""Denoise every image of a directory with a trained pix2pix generator (the reference's
infer.py:24-83, without its display window).

    python infer.py --image_dir noisy/ --output_dir clean/ --model models/pix2pix.npz

--model is a `Generator.save` export: the .npz of weights and moving statistics beside the .json
that names the width.  Images are read and written with Pillow, as RGB; each keeps its size and
file name.  Whole images are padded to a multiple of 256 by default; --tile T (a multiple of 256)
with --margin M runs T x T tiles with M pixels of context instead, --batch of them per forward.
--post median3 puts the denoised frame through a 3x3 median on the device before it is read back
(dgan.filters.median3: the reference's `sr_denoise` output, unit_test.py:95); --post bm3d through
BM3D's first stage set for --bm3d_sigma (dgan.filters.bm3d), --post bm3d2 through both stages
(dgan.filters.bm3d2), --post dejpeg through the shift-averaged JPEG re-application at
--dejpeg_quality (dgan.filters.dejpeg).  --format jpg writes
<stem>.jpg at --jpeg_quality instead: the frame is encoded on the device (dgan.jpeg.jpeg_encode) and
only the file's bytes are read back; --format png writes <stem>.png the same way, lossless
(dgan.png.png_encode).  --decode device reads baseline 4:2:0 .jpg / .jpeg inputs as bytes
and decodes them on the device (dgan.jpeg.jpeg_decode); every other file goes through Pillow, with
a line that says why.  --resize WxH [--resize_filter lanczos] resizes the output frame on the
device as Pillow's `Image.resize` does (dgan.resize.resize_pil) before it is read back or encoded.

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
parser.add_argument("--post", default=None, choices=["median3", "bm3d", "bm3d2", "dejpeg"],
                    help="A classical filter applied to the denoised image on the device (default: none).")
parser.add_argument("--bm3d_sigma", default=25, type=int, help="The noise level --post bm3d / bm3d2 is set for (1..40).")
parser.add_argument("--dejpeg_quality", default=50, type=int,
                    help="The JPEG quality --post dejpeg re-applies (1..100).")
parser.add_argument("--format", default="keep", choices=["keep", "jpg", "png"],
                    help="keep: Pillow writes every image under its own name; jpg / png: baseline JPEG or PNG files "
                         "encoded on the device.")
parser.add_argument("--jpeg_quality", default=90, type=int, help="Quality of --format jpg (1..100).")
parser.add_argument("--decode", default="pillow", choices=["pillow", "device"],
                    help="device: baseline 4:2:0 .jpg / .jpeg files are decoded on the device; every other file through Pillow.")
parser.add_argument("--resize", default=None, type=str,
                    help="WxH: resize the output frame on the device, as Pillow's Image.resize does, before it is written.")
parser.add_argument("--resize_filter", default="bicubic", choices=["box", "bilinear", "hamming", "bicubic", "lanczos"],
                    help="The filter of --resize.")


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


def read_image(image_path, decode):
    """-> uint8 [1,h,w,3]: a device tensor from dgan.jpeg.jpeg_decode for --decode device and a file
    it reads, else the numpy array Pillow decodes."""
    from PIL import Image
    if decode == "device":
        from dgan.jpeg import JpegUnsupported, jpeg_decode, jpeg_parse
        why = "not a .jpg / .jpeg file"
        if image_path.lower().endswith((".jpg", ".jpeg")):
            with open(image_path, "rb") as f:
                data = f.read()
            try:
                jpeg_parse(data)
                return jpeg_decode([data])
            except JpegUnsupported as e:
                why = str(e)
        print(f"{image_path}: decoded by Pillow ({why})")
    with Image.open(image_path) as im:
        return np.asarray(im.convert("RGB"), np.uint8)[None]


def parse_size(text):
    """'WxH' -> (W, H), both at least 1; None for None."""
    if text is None:
        return None
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        w = h = 0
    if min(w, h) < 1:
        parser.error(f"--resize expects WxH with both at least 1, got {text!r}")
    return w, h


def resized(frame, size, filter):
    """The device frame [1,h,w,3] at `size` = (W, H) (dgan.resize.resize_pil), or itself for None."""
    if size is None:
        return frame
    from dgan.resize import resize_pil
    return resize_pil(frame.contiguous(), size[1], size[0], filter)


def post_filtered(frame, args):
    """The device frame through --post (dgan.filters), or itself."""
    if args.post == "median3":
        from dgan.filters import median3
        return median3(frame)
    if args.post == "bm3d":
        from dgan.filters import bm3d
        return bm3d(frame.contiguous(), args.bm3d_sigma)
    if args.post == "bm3d2":
        from dgan.filters import bm3d2
        return bm3d2(frame.contiguous(), args.bm3d_sigma)
    if args.post == "dejpeg":
        from dgan.filters import dejpeg
        return dejpeg(frame.contiguous(), args.dejpeg_quality)
    return frame


def main(argv=None):
    from PIL import Image
    from dgan.infer import Denoiser
    args = parser.parse_args(argv)
    if not 1 <= args.jpeg_quality <= 100:
        parser.error(f"--jpeg_quality must be in 1..100, got {args.jpeg_quality}")
    if not 1 <= args.bm3d_sigma <= 40:
        parser.error(f"--bm3d_sigma must be in 1..40, got {args.bm3d_sigma}")
    size = parse_size(args.resize)
    image_dir = os.path.expanduser(os.path.expandvars(args.image_dir))
    output_dir = os.path.expanduser(os.path.expandvars(args.output_dir))
    model_path = os.path.expanduser(os.path.expandvars(args.model))
    image_paths = [os.path.join(image_dir, x) for x in sorted(os.listdir(image_dir))]
    os.makedirs(output_dir, exist_ok=True)
    denoiser = Denoiser(load_generator(model_path), tile=args.tile or None, margin=args.margin, pad=args.pad,
                        batch=args.batch)
    for image_path in image_paths:
        noisy = read_image(image_path, args.decode)
        if args.format != "keep":
            frame = post_filtered(denoiser.run(noisy).u8_out, args)
            frame = resized(frame, size, args.resize_filter)
            out_path = os.path.join(output_dir, os.path.splitext(os.path.basename(image_path))[0] + "." + args.format)
            if args.format == "jpg":
                from dgan.jpeg import jpeg_encode
                data = jpeg_encode(frame, args.jpeg_quality)[0]
            else:
                from dgan.png import png_encode
                data = png_encode(frame)[0]
            with open(out_path, "wb") as f:
                f.write(data)
            print(f"{image_path} -> {out_path} {frame.shape[2]}x{frame.shape[1]}")
            continue
        frame = post_filtered(denoiser.run(noisy).u8_out, args)
        clean = resized(frame, size, args.resize_filter).cpu().numpy()[0]
        out_path = os.path.join(output_dir, os.path.basename(image_path))
        Image.fromarray(clean, "RGB").save(out_path)
        print(f"{image_path} -> {out_path} {clean.shape[1]}x{clean.shape[0]}")


if __name__ == "__main__":
    main()
