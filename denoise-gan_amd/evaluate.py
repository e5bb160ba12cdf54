"""Score a directory of noisy images against their clean targets: PSNR and SSIM per image, before
and after the trained pix2pix generator.

    python evaluate.py --image_dir noisy/ --target_dir clean/ --model models/pix2pix.npz --json scores.json
    python evaluate.py --jpeg_quality 50 --target_dir clean/ --model models/pix2pix.npz --json scores.json
    python evaluate.py --image_dir noisy/ --target_dir clean/ --model models/pix2pix.npz --baseline nlm

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
--baseline median3 | nlm | bm3d | bm3d2 | dejpeg also puts every noisy image through that classical filter on the
device (dgan.filters; --nlm_h / --nlm_template / --nlm_search, --bm3d_sigma / --bm3d_search /
--bm3d_group, --dejpeg_quality, which defaults to --jpeg_quality when that is given and to 50
otherwise) and scores the result the same way:
psnr_baseline, ssim_baseline, with and without --model.
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
parser.add_argument("--baseline", default=None, choices=["median3", "nlm", "bm3d", "bm3d2", "dejpeg"],
                    help="Also score a classical filter of the noisy image: the 3x3 median, non-local means, BM3D's "
                         "first stage or both stages (bm3d2, which takes the --bm3d_* flags too), or JPEG artifact "
                         "removal by shift-averaged re-application (dejpeg).")
parser.add_argument("--nlm_h", default=10, type=int, help="Non-local means: the filter strength (1..40).")
parser.add_argument("--nlm_template", default=7, type=int, help="Non-local means: the patch size (3, 5 or 7).")
parser.add_argument("--nlm_search", default=21, type=int, help="Non-local means: the search window (odd, 3..21).")
parser.add_argument("--bm3d_sigma", default=25, type=int, help="BM3D: the noise level it is set for (1..40).")
parser.add_argument("--bm3d_search", default=21, type=int, help="BM3D: the search window (odd, 3..21).")
parser.add_argument("--bm3d_group", default=16, type=int, help="BM3D: the most patches of a group (2, 4, 8 or 16).")
parser.add_argument("--dejpeg_quality", default=None, type=int,
                    help="dejpeg: the quality the noisy images were coded with (1..100; default: --jpeg_quality, else 50).")
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


def baseline_args(args):
    """The keywords of dgan.filters.nlm / bm3d / bm3d2 that --baseline nlm / bm3d / bm3d2 asks for ({} for the other
    baselines).  ValueError naming a bad --nlm_* / --bm3d_* value, or one given without its baseline.
    A namespace without the --bm3d_* attributes has their defaults."""
    from dgan.filters import check_bm3d, check_dejpeg, check_nlm
    given = (args.nlm_h, args.nlm_template, args.nlm_search)
    bm3d = tuple(d if v is None else v for v, d in ((getattr(args, "bm3d_sigma", None), 25),
                                                    (getattr(args, "bm3d_search", None), 21),
                                                    (getattr(args, "bm3d_group", None), 16)))
    if args.baseline != "nlm" and given != (10, 7, 21):
        raise ValueError("--nlm_h / --nlm_template / --nlm_search need --baseline nlm")
    if args.baseline not in ("bm3d", "bm3d2") and bm3d != (25, 21, 16):
        raise ValueError("--bm3d_sigma / --bm3d_search / --bm3d_group need --baseline bm3d or bm3d2")
    quality = getattr(args, "dejpeg_quality", None)
    if args.baseline != "dejpeg" and quality is not None:
        raise ValueError("--dejpeg_quality needs --baseline dejpeg")
    if args.baseline == "dejpeg":
        quality = next((q for q in (quality, getattr(args, "jpeg_quality", None)) if q is not None), 50)
        check_dejpeg(quality, None, "--baseline dejpeg")
        return {"quality": int(quality)}
    if args.baseline == "nlm":
        return dict(zip(("h", "template", "search"), check_nlm(*given, what="--baseline nlm")))
    if args.baseline in ("bm3d", "bm3d2"):
        return dict(zip(("sigma", "search", "group"), check_bm3d(*bm3d, what=f"--baseline {args.baseline}")))
    return {}


def summarize(rows):
    """{"images": rows, "mean": the mean of each score over the images}."""
    keys = [k for k in (rows[0] if rows else {}) if k != "name"]
    return {"images": rows, "mean": {k: float(np.mean([r[k] for r in rows])) for k in keys}}


def main(argv=None):
    import torch
    from dgan import filters, metrics
    from dgan.jpeg import jpeg_roundtrip
    args = parser.parse_args(argv)
    try:
        nlm_args = baseline_args(args)
    except ValueError as e:
        parser.error(str(e))
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
                                               pad=args.pad, batch=args.batch),
                                      baseline=args.baseline, baseline_args=nlm_args)
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
            row = {k: float(r[k][0]) for k in evaluator.scores}
        else:
            b = torch.from_numpy(clean[None]).cuda()
            a = torch.from_numpy(noisy[None]).cuda() if image_dir is not None else jpeg_roundtrip(b, args.jpeg_quality)
            row = {"psnr": float(metrics.psnr(a, b).item()), "ssim": float(metrics.ssim(a, b).item())}
            if args.baseline:
                c = getattr(filters, args.baseline)(a, **nlm_args)
                row.update(psnr_baseline=float(metrics.psnr(c, b).item()), ssim_baseline=float(metrics.ssim(c, b).item()))
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
