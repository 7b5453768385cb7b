"""The operation of mudpt_augment (include/mudpt.h) restated in NumPy integers: Pillow's 8-bit bicubic resample of a crop box, the flip and
ToTensor + Normalize.  Weights are computed with Python floats (IEEE fp64, one rounding per operation, sums in ascending tap order); the
two passes are integer.  No Pillow here: tests/test_augment_cpu.py and tests/golden/gen_golden_augment.py hold this file to Pillow, the GPU
tests hold the kernel to this file."""
import numpy as np

PRECISION_BITS = 22
COLUMNS = ("image", "flip", "x_lo", "x_len", "x_out", "x_off", "y_lo", "y_len", "y_out", "y_off")
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def cubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_weights(in_len, out_len, out_off, size, fixed=True):
    """[(first tap, int32 weights)] for the outputs o in [0, size) of one axis.  fixed=False: float64 weights, not rounded to 22 bits."""
    scale = in_len / out_len
    fs = max(scale, 1.0)
    support = 2.0 * fs
    out = []
    for o in range(size):
        center = (o + out_off + 0.5) * scale
        lo, hi = max(0, int(center - support + 0.5)), min(in_len, int(center + support + 0.5))
        raw = [cubic((t - center + 0.5) / fs) for t in range(lo, hi)]
        total = 0.0
        for w in raw:
            total += w
        w = [r / total for r in raw]
        out.append((lo, np.array([int(v * (1 << PRECISION_BITS) + (-0.5 if v < 0 else 0.5)) for v in w], dtype=np.int64) if fixed else np.array(w)))
    return out


def one_pass(src, weights):
    """src [rows, in_len, C] uint8 -> [rows, len(weights), C] uint8 along axis 1."""
    out = np.empty((src.shape[0], len(weights), src.shape[2]), dtype=np.uint8)
    wide = src.astype(np.int64)
    for o, (lo, k) in enumerate(weights):
        if k.dtype == np.int64:
            acc = (1 << (PRECISION_BITS - 1)) + (wide[:, lo:lo + len(k), :] * k[None, :, None]).sum(axis=1)
            assert np.abs(acc).max() < 2 ** 31  # the kernel's accumulators are int32
            out[:, o, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
        else:
            out[:, o, :] = np.clip(np.floor((wide[:, lo:lo + len(k), :] * k[None, :, None]).sum(axis=1) + 0.5), 0, 255)
    return out


def resample(image, row, size, fixed=True):
    """One params row on its HWC uint8 image -> [size, size, 3] uint8, before the flip: horizontal pass, bytes, vertical pass."""
    _, _, x_lo, x_len, x_out, x_off, y_lo, y_len, y_out, y_off = (int(v) for v in row)
    box = image[y_lo:y_lo + y_len, x_lo:x_lo + x_len, :]
    assert box.shape[:2] == (y_len, x_len), "box outside the image"
    horizontal = one_pass(box, axis_weights(x_len, x_out, x_off, size, fixed))
    return one_pass(horizontal.transpose(1, 0, 2), axis_weights(y_len, y_out, y_off, size, fixed)).transpose(1, 0, 2)


def augment_bytes(images, params, size):
    """[B, 3, size, size] uint8: every row of params [B, 10] resampled and flipped."""
    out = np.empty((len(params), 3, size, size), dtype=np.uint8)
    for n, row in enumerate(params):
        r = resample(images[int(row[0])], row, size)
        out[n] = (r[:, ::-1] if row[1] else r).transpose(2, 0, 1)
    return out


def normalize(batch_bytes, mean=CLIP_MEAN, std=CLIP_STD):
    """ToTensor + Normalize on the CPU in fp32: (b / 255 - mean) / std, a torch tensor."""
    import torch
    m, s = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in (mean, std))
    return (torch.from_numpy(np.ascontiguousarray(batch_bytes)).float() / 255 - m) / s


def train_row(image, flip, i, j, h, w, size):
    """RandomResizedCrop's box (top i, left j, height h, width w) resized to size x size."""
    return [image, flip, j, w, size, 0, i, h, size, 0]


def eval_row(image, H, W, size):
    """Resize(size) on the short side, then CenterCrop(size) (torchvision's rounding)."""
    Wr, Hr = (size, int(size * H / W)) if W <= H else (int(size * W / H), size)
    return [image, 0, 0, W, Wr, int(round((Wr - size) / 2.0)), 0, H, Hr, int(round((Hr - size) / 2.0))]


def pack(images, gap=1, odd=False):
    """Flat uint8 buffer + [N, 3] int64 table (byte offset, height, width), `gap` spare bytes in front of every image (odd: one more where
    that makes the offset odd)."""
    table, chunks, off = [], [], 0
    for im in images:
        pad = gap + (1 if odd and (off + gap) % 2 == 0 else 0)
        chunks.append(np.full(pad, 0xA5, dtype=np.uint8))
        off += pad
        table.append((off, im.shape[0], im.shape[1]))
        chunks.append(np.ascontiguousarray(im).reshape(-1))
        off += im.size
    return np.concatenate(chunks), np.array(table, dtype=np.int64).reshape(-1, 3)
