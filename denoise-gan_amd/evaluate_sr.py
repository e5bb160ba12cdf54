"""Score a trained SR-family generator on a directory of high-resolution images: PSNR and SSIM of
its output, and of the bicubic baseline, against the originals.

    python evaluate_sr.py --image_dir hr/ --model models/fsrgan_generator.npz --json scores.json

Every image is degraded as the training pipeline degrades it (a bicubic resize to 1/scale with TF's
float -> uint8 conversion, dataloader.py scale_image; --jpeg_quality Q adds the JPEG round trip),
upscaled by the generator as upscale.py does it (--arch / --scale / --fp16 / --tile / --margin /
--pad / --batch) and, beside it, by a bicubic resize of the same low-resolution frame; both are
scored against the original on the device (dgan.metrics.SREvaluator): psnr_bicubic, psnr_upscaled,
ssim_bicubic, ssim_upscaled.  An image whose sides are not multiples of the scale is centre-cropped
to the largest multiple (the crop is printed); one with a side below the 11x11 SSIM window after the
crop is refused by name.  The metrics are the tf.image.psnr / tf.image.ssim defaults on uint8 RGB
(max_val 255), accumulated in fp64.
"""
import json
import os
from argparse import ArgumentParser

from evaluate import _read_rgb, summarize
from upscale import load_network

parser = ArgumentParser(description="PSNR / SSIM of an SR generator and of the bicubic baseline against high-resolution "
                                    "originals.  One line per image, then the means of the per-image values.")
parser.add_argument("--image_dir", type=str, required=True, help="Directory of the high-resolution images.")
parser.add_argument("--model", default="./models/fsrgan_generator.npz", type=str, help="Path to a GraphNetwork.save export (.npz).")
parser.add_argument("--arch", default="fsrgan", choices=["fsrgan", "srgan", "autoencoder"], help="Which generator the weights belong to.")
parser.add_argument("--scale", default=4, type=int, help="Upscale factor (srgan: 2 or 4; fsrgan: 4; autoencoder: 1).")
parser.add_argument("--fp16", default=0, type=int, help="Run the conv GEMMs on the mixed_float16 policy.")
parser.add_argument("--tile", default=0, type=int, help="Tile size (0: whole image).")
parser.add_argument("--margin", default=0, type=int, help="Context pixels on each side of a tile.")
parser.add_argument("--pad", default="black", choices=["black", "reflect"], help="Values outside the image.")
parser.add_argument("--batch", default=8, type=int, help="Tiles per forward.")
parser.add_argument("--jpeg_quality", default=0, type=int, help="JPEG quality of the low-resolution frame (0: no JPEG step).")
parser.add_argument("--json", default=None, type=str, help="Also write the scores and their means to this file.")


def centre_crop(image, scale):
    """[H,W,C] -> (the centred [H',W',C] window with H', W' the largest multiples of scale,
    (y0, x0, H', W') or None when nothing was cut)."""
    H, W = image.shape[:2]
    Hc, Wc = H - H % scale, W - W % scale
    if (Hc, Wc) == (H, W):
        return image, None
    y0, x0 = (H - Hc) // 2, (W - Wc) // 2
    return image[y0:y0 + Hc, x0:x0 + Wc], (y0, x0, Hc, Wc)


def main(argv=None):
    from dgan import metrics
    from dgan.sr_infer import Upscaler
    args = parser.parse_args(argv)
    image_dir = os.path.expanduser(os.path.expandvars(args.image_dir))
    model_path = os.path.expanduser(os.path.expandvars(args.model))
    net, scale, multiple = load_network(args.arch, model_path, args.scale, bool(args.fp16))
    evaluator = metrics.SREvaluator(Upscaler(net, scale, multiple=multiple, tile=args.tile or None, margin=args.margin,
                                             pad=args.pad, batch=args.batch), jpeg_quality=args.jpeg_quality or None)
    rows = []
    for name in sorted(os.listdir(image_dir)):
        hr, box = centre_crop(_read_rgb(os.path.join(image_dir, name)), scale)
        if box is not None:
            print(f"{name}: cropped to {box[3]}x{box[2]} at ({box[1]}, {box[0]}): a multiple of {scale}")
        if min(hr.shape[:2]) < metrics.SSIM_TAPS:
            raise SystemExit(f"{name} is {hr.shape[1]}x{hr.shape[0]}: smaller than the "
                             f"{metrics.SSIM_TAPS}x{metrics.SSIM_TAPS} SSIM window")
        r = evaluator.evaluate(hr)
        row = {k: float(r[k][0]) for k in metrics.SR_SCORES}
        rows.append({"name": name, **row})
        print(name + "".join(f" {k} {v:.4f}" for k, v in row.items()))
    result = summarize(rows)
    print("mean" + "".join(f" {k} {v:.4f}" for k, v in result["mean"].items()) + f" ({len(rows)} images)")
    if args.json:
        with open(os.path.expanduser(os.path.expandvars(args.json)), "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
