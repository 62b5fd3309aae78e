"""Mint tests/golden/image_prep_pil.npz: small seeded uint8 images and what PIL makes of them.

    python tools/make_image_goldens.py [--check]

Needs Pillow (the tests that read the fixture do not).  For every case the fixture holds the input `in_<name>` and
`out_<name>`, the uint8 result of `Image.resize(..., BILINEAR)` at torchvision's `Resize(res)` size followed by `CenterCrop(res)`
(Python's round for the offsets), or of an explicit `resize=(h, w)` with no crop; `cases` is the JSON list of
{name, h, w, res | resize} and `pillow_version` the version that produced the outputs.  The archive is written with fixed
timestamps, so the same Pillow gives the same file byte for byte; --check compares a fresh mint with the committed file.
"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "image_prep_pil.npz")

CASES = [
    dict(name="down_landscape", h=37, w=53, res=16),
    dict(name="down_portrait", h=53, w=37, res=16),
    dict(name="up_landscape", h=17, w=40, res=32),
    dict(name="up_square", h=33, w=33, res=64),
    dict(name="ratio8", h=128, w=192, res=16),
    dict(name="crop_only_left2", h=16, w=21, res=16),        # (21 - 16) / 2 = 2.5 -> 2
    dict(name="crop_only_left4", h=16, w=23, res=16),        # (23 - 16) / 2 = 3.5 -> 4
    dict(name="horizontal_only", h=32, w=48, resize=[32, 24]),
    dict(name="vertical_only", h=32, w=48, resize=[16, 48]),
    dict(name="multi_tile", h=100, w=150, res=72),           # 72 x 108 resized; the 72 x 72 crop spans 5 x 2 tiles of 16 x 64
    dict(name="all_255", h=37, w=53, res=16, fill=255),
    dict(name="all_0", h=53, w=37, res=16, fill=0),
]


def resize_size(h, w, res):
    short, long = (w, h) if w <= h else (h, w)
    if short == res:
        return h, w
    new_long = int(res * long / short)
    return (new_long, res) if w <= h else (res, new_long)


def mint():
    import PIL
    from PIL import Image
    arrays = {}
    for i, c in enumerate(CASES):
        rng = np.random.default_rng(1000 + i)
        if "fill" in c:
            img = np.full((c["h"], c["w"], 3), c["fill"], np.uint8)
        else:
            # white noise: every byte value occurs and neighbouring pixels differ, so a wrong tap or weight shows
            img = rng.integers(0, 256, (c["h"], c["w"], 3), dtype=np.uint8)
        pil = Image.fromarray(img, "RGB")
        if "resize" in c:
            oh, ow = c["resize"]
            out = np.asarray(pil.resize((ow, oh), Image.BILINEAR))
        else:
            res = c["res"]
            oh, ow = resize_size(c["h"], c["w"], res)
            if (oh, ow) != (c["h"], c["w"]):
                pil = pil.resize((ow, oh), Image.BILINEAR)
            top, left = int(round((oh - res) / 2.0)), int(round((ow - res) / 2.0))
            out = np.asarray(pil)[top:top + res, left:left + res]
        arrays["in_" + c["name"]] = img
        arrays["out_" + c["name"]] = np.ascontiguousarray(out)
    arrays["cases"] = np.frombuffer(json.dumps(CASES).encode(), np.uint8)
    arrays["pillow_version"] = np.frombuffer(PIL.__version__.encode(), np.uint8)
    return arrays


def write(arrays, path):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="mint to memory and compare with the committed fixture")
    a = ap.parse_args()
    arrays = mint()
    if a.check:
        tmp = io.BytesIO()
        write(arrays, tmp)
        same = tmp.getvalue() == open(OUT, "rb").read()
        print("identical" if same else "DIFFERENT")
        return 0 if same else 1
    write(arrays, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
