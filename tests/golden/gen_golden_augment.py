"""Writes tests/golden/augment_cases.npz: small uint8 sources, parameter rows of mudpt_augment and the bytes Pillow gives for them --
crop(box).resize((S, S), BICUBIC) (+ FLIP_LEFT_RIGHT) for the training rows, resize((Wr, Hr), BICUBIC).crop(centre) for the evaluation rows.
Run from the repository root with Pillow installed:  python tests/golden/gen_golden_augment.py

Every case is held to tests/augment_reference.py before anything is written, so a source on which Pillow departs from its
horizontal-then-vertical order (seen on sources 8 pixels wide and >= 900 rows high, Pillow 12.2.0) cannot get in."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import augment_reference as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment_cases.npz")
SIZES = (16, 24)


def sources(rng):
    yy, xx = np.mgrid[0:64, 0:48]
    smooth = np.stack([(yy * 3 + xx) % 256, (255 - yy * 2 - xx) % 256, (yy * xx // 13) % 256], axis=-1).astype(np.uint8)
    return [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), smooth, (rng.integers(0, 2, (20, 33, 3)) * 255).astype(np.uint8),
            rng.integers(0, 256, (12, 200, 3), dtype=np.uint8), rng.integers(0, 256, (150, 10, 3), dtype=np.uint8)]


def rows(images, S):
    train = [R.train_row(0, 0, 3, 5, 30, 41, S), R.train_row(0, 1, 0, 0, 37, 53, S), R.train_row(0, 0, 36, 52, 1, 1, S),
             R.train_row(0, 1, 2, 10, 1, 33, S), R.train_row(1, 0, 7, 9, 5, 7, S), R.train_row(1, 1, 11, 13, S, S, S),
             R.train_row(1, 0, 0, 0, 64, 48, S), R.train_row(2, 1, 0, 0, 20, 33, S), R.train_row(2, 0, 3, 4, 9, 11, S),
             R.train_row(3, 0, 0, 0, 12, 200, S), R.train_row(3, 1, 1, 17, 10, 163, S), R.train_row(4, 0, 0, 0, 150, 10, S),
             R.train_row(4, 1, 20, 1, 101, 7, S)]
    evaluation = [R.eval_row(i, im.shape[0], im.shape[1], S) for i, im in enumerate(images)]
    return np.array(train, dtype=np.int32), np.array(evaluation, dtype=np.int32)


def pillow_bytes(images, params, S, evaluation):
    from PIL import Image
    out = np.empty((len(params), 3, S, S), dtype=np.uint8)
    for n, (image, flip, x_lo, x_len, x_out, x_off, y_lo, y_len, y_out, y_off) in enumerate(params.tolist()):
        im = Image.fromarray(images[image], "RGB")
        if evaluation:
            im = im.resize((x_out, y_out), Image.BICUBIC).crop((x_off, y_off, x_off + S, y_off + S))
        else:
            im = im.crop((x_lo, y_lo, x_lo + x_len, y_lo + y_len)).resize((S, S), Image.BICUBIC)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        out[n] = np.asarray(im).transpose(2, 0, 1)
    return out


def main():
    import PIL
    images = sources(np.random.default_rng(20))
    arrays = {f"image_{i}": im for i, im in enumerate(images)}
    for S in SIZES:
        for kind, params in zip(("train", "eval"), rows(images, S)):
            want = pillow_bytes(images, params, S, kind == "eval")
            got = R.augment_bytes(images, params, S)
            assert np.array_equal(got, want), (S, kind, np.argwhere(got != want)[:5])
            arrays[f"{kind}_params_{S}"], arrays[f"{kind}_bytes_{S}"] = params, want
    arrays["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
