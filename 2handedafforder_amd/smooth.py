#!/usr/bin/env python3
"""Mask smoothing over a tree of images, in place: the command line (--input_dir, --threshold) and the effect of the reference's
ActAffordance/scripts/utils/gaussian.py, step 2 of its benchmark workflow between inference.py and the scoring. Every image file
below --input_dir is read as grey scale, blurred as cv2.GaussianBlur(img, (7, 7), 0) blurs it, compared with
`blurred / 255.0 > --threshold` and written back over itself as 0 / 255.

  python -m 2handedafforder_amd.smooth --input_dir vis_output0.5 [--threshold 0.5]

This is the files route, on the host: for trees that already exist and for inputs that are not 0 / 255 planes. A run that still has
its masks on the device smooths them there (`inference.py --smooth_masks`) and leaves the bytes this tool would leave.
Images are read and written with PIL and blurred by cvlite.gaussian_blur7_u8 (cv2 is not a dependency here); the grey-scale
conversion of a colour input is PIL's convert("L"), which can differ from cv2.imread's by one level.
"""
import argparse
import os
import sys

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import haff  # noqa: F401
    from haff import cvlite
else:
    from . import cvlite

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")   # the files gaussian.py touches, by lower-cased suffix


def smooth_plane(plane, threshold=0.5):
    """A 2-D uint8 image -> uint8 of 0 / 255: blur, divide by 255.0 in double, strict compare."""
    return (cvlite.gaussian_blur7_u8(plane) / 255.0 > threshold).astype(np.uint8) * 255


def smooth_file(path, threshold=0.5):
    """Smooth one image file over itself; False (and a warning, as the reference prints one) when it cannot be read."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            plane = np.asarray(im.convert("L"))
    except (OSError, ValueError):
        print(f"Warning: Failed to load image {path}")
        return False
    options = {"quality": 95} if path.lower().endswith((".jpg", ".jpeg")) else {}   # cv2.imwrite's JPEG default
    Image.fromarray(smooth_plane(plane, threshold)).save(path, **options)
    return True


def smooth_tree(input_dir, threshold=0.5):
    """Every image file below input_dir, in os.walk's order. Returns how many were rewritten."""
    done = 0
    for root, _, names in os.walk(input_dir):
        for name in names:
            if name.lower().endswith(EXTENSIONS):
                done += smooth_file(os.path.join(root, name), threshold)
    return done


def main(argv=None):
    parser = argparse.ArgumentParser(description="7x7 Gaussian smoothing + threshold of every image under a directory, in place")
    parser.add_argument("--input_dir", type=str, required=True, help="root of the tree of images to rewrite")
    parser.add_argument("--threshold", type=float, default=0.5, help="a pixel stays on where blurred / 255 exceeds this (default 0.5)")
    args = parser.parse_args(argv)
    return smooth_tree(args.input_dir, args.threshold)


if __name__ == "__main__":
    main()
