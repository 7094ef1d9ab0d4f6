"""Writes tests/golden/jpeg/: small baseline JPEG files and, for each, Pillow's (libjpeg-turbo's) decoded pixels as an .npz.

Run on a development machine with Pillow; the tests read only the files written here.  The images mix gradients with seeded
noise so that blocks have short and long coefficient runs.  The set is the smallest shapes at which each mechanism of the
decoder can go wrong:
  1x1, 8x8, 17x9 (less than one 4:2:0 MCU in one direction), 37x53, 64x48 (whole MCUs) in GRAY, 444, 422 and 420;
  37x53 420 at quality 5 and quality 100 (large coefficients, long runs), with restart markers every 2 MCUs, with a COM and
  an APP1 segment in front of SOF, and as a progressive file (which the decoder must refuse).
The .npz holds `pixels`: [H, W, 3] u8 RGB, or [H, W] u8 for a grey file.

    python tests/golden/make_jpeg_golden.py
"""
import io
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg")
SIZES = [(1, 1), (8, 8), (17, 9), (37, 53), (64, 48)]          # (width, height)
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def make_image(w, h, seed):
    """[h, w, 3] u8 RGB: a gradient per channel in steps of 6 pixels (flat steps keep the stored pixels small); the right 40 % of
    the columns carry noise of growing strength"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x // 6 * 6, y // 6 * 6
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), 255.0 - (x + y) * 255.0 / max(w + h - 2, 1)], -1)
    noise = rng.normal(0.0, 1.0, (h, w, 3)) * np.maximum(0.0, 160.0 * (x / max(w - 1, 1) - 0.6))[..., None]
    return np.clip(np.rint(base + noise), 0, 255).astype(np.uint8)


def encode(rgb, sampling, quality=90, **kw):
    buf = io.BytesIO()
    if sampling == "GRAY":
        Image.fromarray(rgb, "RGB").convert("L").save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[sampling], **kw)
    return buf.getvalue()


def decoded(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode in ("L", "RGB"), im.mode
    return np.asarray(im).copy()


def write(name, data, with_pixels=True):
    with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
        f.write(data)
    if with_pixels:
        np.savez_compressed(os.path.join(OUT, name + ".npz"), pixels=decoded(data))


def main():
    os.makedirs(OUT, exist_ok=True)
    for i, (w, h) in enumerate(SIZES):
        for j, s in enumerate(("GRAY", "444", "422", "420")):
            write("%dx%d_%s" % (w, h, s), encode(make_image(w, h, 100 + 10 * i + j), s))
    rgb = make_image(37, 53, 7)
    write("37x53_420_q5", encode(rgb, "420", quality=5))
    write("37x53_420_q100", encode(rgb, "420", quality=100))
    write("37x53_420_rst2", encode(rgb, "420", restart_marker_blocks=2))
    exif = Image.Exif()
    exif[0x010e] = "rfd golden"                                  # ImageDescription: makes an APP1 segment
    write("37x53_420_com_app1", encode(rgb, "420", comment=b"rfd golden file", exif=exif.tobytes()))
    write("37x53_420_progressive", encode(rgb, "420", progressive=True), with_pixels=False)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("%d files, %d bytes in %s" % (len(os.listdir(OUT)), total, OUT))


if __name__ == "__main__":
    main()
