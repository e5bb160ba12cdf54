"""Score a directory of noisy images against their clean targets: PSNR and SSIM per image, before
and after the trained pix2pix generator.

    python evaluate.py --image_dir noisy/ --target_dir clean/ --model models/pix2pix.npz --json scores.json
    python evaluate.py --jpeg_quality 50 --target_dir clean/ --model models/pix2pix.npz --json scores.json

Files pair by stem (noisy/a.png with clean/a.jpg); a file without a partner, a pair of different
sizes, or an image smaller than the 11x11 SSIM window is refused by name.  With --model every
noisy image is denoised as infer.py does it (--tile / --margin / --pad / --batch) and scored on
the device where the frames already are (dgan.metrics.Evaluator): psnr_noisy, psnr_denoised,
ssim_noisy, ssim_denoised.  An evaluation keeps the buffers of the few most recent image sizes
only (dgan.metrics MAX_PLANS, Evaluator.MAX_SHAPES).  Without --model
the two directories are compared directly: psnr, ssim.  With --jpeg_quality Q in place of
--image_dir the noisy images are made here: every clean image goes through a JPEG round trip at
quality Q with 4:2:0 subsampling on the device (dgan.jpeg, the degradation the training pipeline
applies, bit for bit what Pillow's codec returns), and the scores are the same.  The metrics are
the tf.image.psnr / tf.image.ssim defaults on uint8 RGB (max_val 255), accumulated in fp64.
"""
import json
import os
from argparse import ArgumentParser

import numpy as np

parser = ArgumentParser(description="PSNR / SSIM of a directory of images against their targets.  One line per image, "
                                    "then the means: every mean, PSNR included, is the mean of the per-image values "
                                    "(the mean of the dB values, not the PSNR of the pooled error).")
parser.add_argument("--image_dir", type=str, default=None,
                    help="Directory of the noisy images (this or --jpeg_quality, not both).")
parser.add_argument("--jpeg_quality", type=int, default=None,
                    help="Make the noisy images from the clean ones instead: a JPEG round trip at this quality (1..100).")
parser.add_argument("--target_dir", type=str, required=True, help="Directory of the clean images, paired by file stem.")
parser.add_argument("--model", default=None, type=str,
                    help="Path to a Generator.save export (.npz): score the images before and after denoising.  "
                         "Without it the two directories are compared directly.")
parser.add_argument("--tile", default=0, type=int, help="Tile size, a multiple of 256 (0: whole image).")
parser.add_argument("--margin", default=0, type=int, help="Context pixels on each side of a tile.")
parser.add_argument("--pad", default="black", choices=["black", "reflect"], help="Values outside the image.")
parser.add_argument("--batch", default=8, type=int, help="Tiles per forward.")
parser.add_argument("--json", default=None, type=str, help="Also write the scores and their means to this file.")


def pair_by_stem(image_names, target_names):
    """[(stem, image name, target name)] in stem order.  ValueError naming every file whose stem
    has no partner on the other side, or that shares its stem with another file of its side."""
    def by_stem(names, side):
        out = {}
        for name in sorted(names):
            stem = os.path.splitext(name)[0]
            if stem in out:
                raise ValueError(f"{side}: {out[stem]} and {name} share the stem {stem!r}")
            out[stem] = name
        return out

    images, targets = by_stem(image_names, "image_dir"), by_stem(target_names, "target_dir")
    lonely = ([f"{images[s]} has no target" for s in sorted(set(images) - set(targets))] +
              [f"{targets[s]} has no image" for s in sorted(set(targets) - set(images))])
    if lonely:
        raise ValueError("unpaired files: " + "; ".join(lonely))
    return [(s, images[s], targets[s]) for s in sorted(images)]


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), np.uint8)


def summarize(rows):
    """{"images": rows, "mean": the mean of each score over the images}."""
    keys = [k for k in (rows[0] if rows else {}) if k != "name"]
    return {"images": rows, "mean": {k: float(np.mean([r[k] for r in rows])) for k in keys}}


def main(argv=None):
    import torch
    from dgan import metrics
    from dgan.jpeg import jpeg_roundtrip
    args = parser.parse_args(argv)
    if (args.image_dir is None) == (args.jpeg_quality is None):
        parser.error("give exactly one of --image_dir and --jpeg_quality")
    if args.jpeg_quality is not None and not 1 <= args.jpeg_quality <= 100:
        parser.error(f"--jpeg_quality must be in 1..100, got {args.jpeg_quality}")
    target_dir = os.path.expanduser(os.path.expandvars(args.target_dir))
    if args.image_dir is None:
        image_dir = None
        pairs = [(os.path.splitext(name)[0], name, name) for name in sorted(os.listdir(target_dir))]
    else:
        image_dir = os.path.expanduser(os.path.expandvars(args.image_dir))
        try:
            pairs = pair_by_stem(os.listdir(image_dir), os.listdir(target_dir))
        except ValueError as e:
            raise SystemExit(str(e))
    evaluator = None
    if args.model:
        from dgan.infer import Denoiser
        from infer import load_generator
        model_path = os.path.expanduser(os.path.expandvars(args.model))
        evaluator = metrics.Evaluator(Denoiser(load_generator(model_path), tile=args.tile or None, margin=args.margin,
                                               pad=args.pad, batch=args.batch))
    rows = []
    for stem, image_name, target_name in pairs:
        clean = _read_rgb(os.path.join(target_dir, target_name))
        noisy = clean if image_dir is None else _read_rgb(os.path.join(image_dir, image_name))
        if noisy.shape != clean.shape:
            raise SystemExit(f"{image_name} is {noisy.shape[1]}x{noisy.shape[0]} but its target {target_name} is "
                             f"{clean.shape[1]}x{clean.shape[0]}")
        if min(noisy.shape[:2]) < metrics.SSIM_TAPS:
            raise SystemExit(f"{image_name} is {noisy.shape[1]}x{noisy.shape[0]}: smaller than the "
                             f"{metrics.SSIM_TAPS}x{metrics.SSIM_TAPS} SSIM window")
        if evaluator is not None:
            r = evaluator.evaluate(noisy, clean) if image_dir is not None else evaluator.evaluate_degraded(
                clean, args.jpeg_quality)
            row = {k: float(r[k][0]) for k in metrics.SCORES}
        else:
            b = torch.from_numpy(clean[None]).cuda()
            a = torch.from_numpy(noisy[None]).cuda() if image_dir is not None else jpeg_roundtrip(b, args.jpeg_quality)
            row = {"psnr": float(metrics.psnr(a, b).item()), "ssim": float(metrics.ssim(a, b).item())}
        rows.append({"name": image_name, **row})
        print(image_name + "".join(f" {k} {v:.4f}" for k, v in row.items()))
    result = summarize(rows)
    print("mean" + "".join(f" {k} {v:.4f}" for k, v in result["mean"].items()) + f" ({len(rows)} images)")
    if args.json:
        with open(os.path.expanduser(os.path.expandvars(args.json)), "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
