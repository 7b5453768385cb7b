"""The training input pipeline on the device: images decoded ONCE into a uint8 store in HBM, a few integers per sample drawn on the host
each step, one HIP launch (mudpt_augment, csrc/augment.hip) that crops, resamples, flips and normalises into the [B, 3, S, S] fp32 batch.

It replaces, for the transforms every shipped yaml uses (INPUT.TRANSFORMS random_resized_crop + random_flip + normalize, INTERPOLATION
"bicubic"), Dassl's per-step Pillow pipeline on the loader's CPU workers and the 154 MB host -> device copy of a B = 256 batch
(DESIGN.md 5).  The kernel reproduces Pillow's 8-bit bicubic arithmetic, so the bytes are the ones the reference's pipeline feeds the
model; which crops are drawn follows torchvision's RandomResizedCrop.get_params in distribution, from this module's own seeded stream.

Opt-in (trainer.install_loader: MUDPT_DEVICE_DATA=1 or trainer.device_store); nothing here runs otherwise.  The test pass has its own
switch (trainer.install_test_loader: MUDPT_DEVICE_TEST=1 or trainer.device_test_store -> DeviceEvalLoader, the evaluation transform).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import capi, parallel

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)  # INPUT.PIXEL_MEAN / PIXEL_STD of the shipped yamls
COLUMNS = ("image", "flip", "x_lo", "x_len", "x_out", "x_off", "y_lo", "y_len", "y_out", "y_off")
AUGMENT_FORMS = ("TABLE", "DIRECT")  # MUDPT_AUGMENT_*: the low byte of mudpt_augment_form


def check_params(table: torch.Tensor, params: torch.Tensor, size: int):
    """mudpt_augment_check on host copies of the image table [N, 3] int64 and the parameter rows [B, 10] int32: raises (AssertionError, the
    library's MUDPT_ERR_ARG) naming the row and column that fails.  No table reaches the device without passing here: the kernel trusts them."""
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 3 and table.device.type == "cpu" and table.is_contiguous()
    assert params.dtype == torch.int32 and params.dim() == 2 and params.shape[1] == 10 and params.device.type == "cpu" and params.is_contiguous()
    some = lambda t, width, dtype: t if t.numel() else torch.zeros(1, width, dtype=dtype)  # noqa: E731 -- an empty tensor has a null data_ptr
    capi.check(capi.call("mudpt_augment_check", images_host=some(table, 3, torch.int64), n_images=table.shape[0], params_host=some(params, 10, torch.int32),
                         batch=params.shape[0], size=size), "augment_check")


def augment_form(x_len: int, x_out: int, y_len: int, y_out: int, size: int):
    """(form name, output rows per pass) of one sample: host arithmetic of the library."""
    code = capi.call("mudpt_augment_form", x_len=x_len, x_out=x_out, y_len=y_len, y_out=y_out, size=size)
    if code < 0:
        raise ValueError(f"augment_form: lengths must be >= 1, got {(x_len, x_out, y_len, y_out, size)}")
    return AUGMENT_FORMS[code & 0xff], code >> 8


class StoreTooLarge(ValueError):
    """The decoded images exceed the ``max_bytes`` the caller allows the store."""


class DeviceImageStore:
    """N decoded RGB images as ONE flat uint8 HWC buffer on the device, their [N, 3] table (byte offset, height, width) on host and
    device, and their labels on the device.  ``device`` "cpu" holds the same tables for host arithmetic (rrc_params, the loader's index
    math); ``augment`` needs the GPU -- there is no CPU form of the kernel."""

    def __init__(self, pixels: torch.Tensor, table: torch.Tensor, labels: torch.Tensor, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = table.to(torch.int64).contiguous()  # host
        check_params(self.table, torch.zeros(0, 10, dtype=torch.int32), 1)
        assert pixels.dtype == torch.uint8 and pixels.dim() == 1 and labels.shape == (self.table.shape[0],)
        assert self.table.shape[0] == 0 or int(self.table[-1, 0] + 3 * self.table[-1, 1] * self.table[-1, 2]) <= pixels.numel(), "the table runs past the buffer"
        self.pixels = pixels.to(self.device)
        self.table_dev = self.table.to(self.device)
        self.labels = labels.to(torch.int64).to(self.device)

    def __len__(self):
        return self.table.shape[0]

    @property
    def nbytes(self) -> int:
        return self.pixels.numel()

    @classmethod
    def from_arrays(cls, arrays, labels, device=None, max_bytes: int | None = None):
        """arrays: HWC uint8 (numpy arrays or torch tensors; any iterable of them), three channels, any sizes.  max_bytes: StoreTooLarge is
        raised as soon as the images seen so far exceed it, before anything is uploaded."""
        flat, rows, off = [], [], 0
        for a in arrays:
            t = torch.as_tensor(a)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
                raise ValueError(f"DeviceImageStore: an image must be uint8 [H, W, 3] with H, W >= 1, got {t.dtype} {tuple(t.shape)}")
            rows.append((off, t.shape[0], t.shape[1]))
            flat.append(t.contiguous().reshape(-1))
            off += t.numel()
            if max_bytes is not None and off > max_bytes:
                raise StoreTooLarge(f"the first {len(rows)} decoded images take {off} bytes, more than the {max_bytes} allowed")
        pixels = torch.cat(flat) if flat else torch.zeros(0, dtype=torch.uint8)
        device = device if device is not None else f"cuda:{torch.cuda.current_device()}"
        return cls(pixels, torch.tensor(rows, dtype=torch.int64).reshape(-1, 3), torch.as_tensor(labels), device)

    @classmethod
    def from_paths(cls, paths, labels, device=None, max_bytes: int | None = None):
        """Decode every file once, as Dassl's read_image does: PIL.Image.open(path).convert("RGB")."""
        try:
            from PIL import Image
        except ImportError:
            raise RuntimeError("DeviceImageStore.from_paths decodes with Pillow, which is not installed; decode the images yourself and use from_arrays") from None
        import numpy as np
        return cls.from_arrays((np.asarray(Image.open(p).convert("RGB")) for p in paths), labels, device, max_bytes)

    def labels_of(self, indices) -> torch.Tensor:
        return self.labels[torch.as_tensor(indices, dtype=torch.int64).to(self.device)]

    def augment(self, params: torch.Tensor, size: int, mean=CLIP_MEAN, std=CLIP_STD, out: torch.Tensor | None = None) -> torch.Tensor:
        """params [B, 10] int32 on the host (rrc_params / center_crop_params) -> [B, 3, size, size] fp32 on the device, one launch on the
        current stream.  ``out``: a larger preallocated batch whose first B images are written."""
        if self.device.type != "cuda":
            raise capi.MudptError("DeviceImageStore.augment runs a HIP kernel: the store must live on a GPU (there is no CPU form)")
        params = params.contiguous()
        check_params(self.table, params, size)
        return self.launch(params.to(self.device), size, mean, std, out)

    def launch(self, params_dev: torch.Tensor, size: int, mean=CLIP_MEAN, std=CLIP_STD, out: torch.Tensor | None = None) -> torch.Tensor:
        """``augment`` for rows that are on the device already -- and whose HOST copy has passed check_params: the kernel trusts them."""
        B = params_dev.shape[0]
        assert params_dev.dtype == torch.int32 and tuple(params_dev.shape) == (B, 10) and params_dev.is_contiguous() and params_dev.device == self.device
        if out is None:
            out = torch.empty(B, 3, size, size, dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device and out.shape[0] >= B and tuple(out.shape[1:]) == (3, size, size)
        if B == 0:
            return out[:0]
        mean_std = (C.c_float * 6)(*mean, *std)
        with torch.cuda.device(self.device):
            capi.check(capi.call("mudpt_augment", pixels_dev=self.pixels, images_dev=self.table_dev, n_images=len(self), params_dev=params_dev,
                                 batch=B, size=size, mean_std_host=C.addressof(mean_std), out_dev=out,
                                 stream=torch.cuda.current_stream(self.device).cuda_stream), "augment")
        return out[:B]


def _heights_widths(store, indices):
    idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
    return idx, store.table[idx, 1].double(), store.table[idx, 2].double()


def rrc_params(store, indices, size: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p: float = 0.5, generator: torch.Generator | None = None) -> torch.Tensor:
    """torchvision's RandomResizedCrop.get_params + RandomHorizontalFlip for every sample at once, on the host: [B, 10] int32 rows.
    Ten attempts per sample -- area fraction U(scale), aspect log-uniform over ratio, w = round(sqrt(A r)), h = round(sqrt(A / r)) -- the
    first with 0 < w <= W and 0 < h <= H gets uniform integer offsets; if none fits, the central crop clamped to the ratio bounds.  All
    uniforms come from ONE draw of ``generator``, so the rows are a function of its state alone."""
    idx, H, W = _heights_widths(store, indices)
    B = idx.numel()
    u = torch.rand(B, 23, dtype=torch.float64, generator=generator)
    area = (H * W)[:, None] * (scale[0] + (scale[1] - scale[0]) * u[:, :10])
    aspect = torch.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * u[:, 10:20])
    w, h = torch.round(torch.sqrt(area * aspect)), torch.round(torch.sqrt(area / aspect))
    ok = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
    first = torch.where(ok.any(dim=1), ok.double().argmax(dim=1), torch.zeros(B, dtype=torch.int64))
    w, h = w.gather(1, first[:, None])[:, 0], h.gather(1, first[:, None])[:, 0]
    top, left = torch.floor(u[:, 20] * (H - h + 1)), torch.floor(u[:, 21] * (W - w + 1))
    # the fallback (get_params' tail): the whole image, narrowed to the nearest allowed aspect, centred
    in_ratio = W / H
    fw = torch.where(in_ratio > max(ratio), torch.round(H * max(ratio)), W)
    fh = torch.where(in_ratio < min(ratio), torch.round(W / min(ratio)), H)
    fw, fh = fw.clamp(min=1).minimum(W), fh.clamp(min=1).minimum(H)
    fell = ~ok.any(dim=1)
    w, h = torch.where(fell, fw, w), torch.where(fell, fh, h)
    top, left = torch.where(fell, torch.floor((H - h) / 2), top), torch.where(fell, torch.floor((W - w) / 2), left)
    flip = (u[:, 22] < flip_p).double()
    S, zero = torch.full((B,), float(size), dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    return torch.stack([idx.double(), flip, left, w, S, zero, top, h, S, zero], dim=1).to(torch.int32).contiguous()


def center_crop_params(store, indices, size: int) -> torch.Tensor:
    """The evaluation transform, Resize(size) on the short side (the long side int(size * long / short)) then CenterCrop(size), as rows of
    the same operation: the whole image resampled to (Hr, Wr), of which the kernel computes the central size x size window only."""
    idx, H, W = _heights_widths(store, indices)
    rows = []
    for i, h, w in zip(idx.tolist(), H.long().tolist(), W.long().tolist()):
        wr, hr = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
        rows.append([i, 0, 0, w, wr, int(round((wr - size) / 2.0)), 0, h, hr, int(round((hr - size) / 2.0))])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 10)


class DeviceEvalLoader:
    """The test loader over a DeviceImageStore: every image once, in index order, no drop_last, under the evaluation transform
    (center_crop_params).  The rows of the WHOLE store are computed, held to check_params and uploaded once, here; a batch is then a slice
    of those device rows into store.launch plus a slice of store.labels -- no host copy and no sync per batch.  Yields
    {"img", "label", "_mudpt_sharded": True} with device tensors produced on the current stream.  Every rank evaluates the whole
    store, as the reference's test() does.  A "cpu" store holds the same rows for host arithmetic (``params``, ``batch_ranges``);
    iterating needs the GPU."""

    def __init__(self, store, batch_size: int, size: int, mean=CLIP_MEAN, std=CLIP_STD):
        self.store, self.batch_size, self.size, self.mean, self.std = store, int(batch_size), int(size), tuple(mean), tuple(std)
        if self.batch_size < 1:
            raise ValueError(f"a test batch of {batch_size} images")
        if len(store) == 0:
            raise ValueError("a store of 0 images gives no test batch")
        self.params = center_crop_params(store, range(len(store)), self.size).contiguous()  # host
        check_params(store.table, self.params, self.size)
        self.params_dev = self.params.to(store.device)

    def __len__(self):
        return -(-len(self.store) // self.batch_size)

    def batch_ranges(self):
        """[(first, past-the-last)] store index of every batch: the last one may be short."""
        n = len(self.store)
        return [(lo, min(lo + self.batch_size, n)) for lo in range(0, n, self.batch_size)]

    def __iter__(self):
        if self.store.device.type != "cuda":
            raise capi.MudptError("DeviceEvalLoader runs a HIP kernel per batch: the store must live on a GPU (there is no CPU form)")
        for lo, hi in self.batch_ranges():
            yield {"img": self.store.launch(self.params_dev[lo:hi], self.size, self.mean, self.std), "label": self.store.labels[lo:hi], "_mudpt_sharded": True}


class DeviceAugmentLoader:
    """The training loader over a DeviceImageStore.  ``batch_size`` is the GLOBAL batch.  Each epoch draws one permutation of the store
    and the crops of every global batch from generators seeded by (seed, epoch): the same on every rank, so rank r takes the contiguous
    slice parallel.shard gives it -- what nn.DataParallel's scatter, or parallel.shard_batch on a loaded batch, would.  Yields
    {"img", "label", "_mudpt_sharded": True} with device tensors produced on the current stream; ``last_params`` keeps the rows of the
    last batch (this rank's)."""

    def __init__(self, store, batch_size: int, size: int, mean=CLIP_MEAN, std=CLIP_STD, scale=(0.08, 1.0), seed: int = 0, drop_last: bool = True,
                 rank: int | None = None, world: int | None = None):
        self.store, self.batch_size, self.size, self.mean, self.std, self.scale = store, int(batch_size), int(size), tuple(mean), tuple(std), tuple(scale)
        self.seed, self.drop_last, self.epoch, self.last_params = int(seed), drop_last, 0, None
        self.rank = parallel.rank() if rank is None else rank
        self.world = parallel.world_size() if world is None else world
        if self.batch_size < 1 or self.batch_size % self.world != 0:
            raise ValueError(f"global batch {self.batch_size} is not divisible by the {self.world} data-parallel ranks")
        if len(self) == 0:
            raise ValueError(f"a store of {len(store)} images gives no batch of {self.batch_size}")

    def __len__(self):
        n = len(self.store)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _epoch_rows(self, epoch: int):
        """(indices, params) of this rank, batch after batch, drawn in order from the epoch's one generator: host arithmetic only."""
        g = torch.Generator().manual_seed(self.seed * 1000003 + epoch)
        perm = torch.randperm(len(self.store), generator=g)
        for b in range(len(self)):
            idx = perm[b * self.batch_size:(b + 1) * self.batch_size]
            params = rrc_params(self.store, idx, self.size, scale=self.scale, generator=g)  # the GLOBAL batch's rows: every rank draws the same
            r = parallel.shard(idx.numel(), self.rank, self.world)
            yield idx[r.start:r.stop], params[r.start:r.stop].contiguous()

    def epoch_batches(self, epoch: int):
        """[(indices, params)] of this rank for one epoch."""
        return list(self._epoch_rows(epoch))

    def _stage(self, rows):
        """The worker's share of a batch: draw its rows, hold them to check_params, and lay rows and indices out in one (pinned) host
        buffer, so that the consumer pays one asynchronous copy and the launch."""
        item = next(rows, None)
        if item is None:
            return None
        idx, params = item
        check_params(self.store.table, params, self.size)
        staged = torch.cat([params.reshape(-1), idx.to(torch.int32)])
        if self.store.device.type == "cuda":
            with torch.cuda.device(self.store.device):
                staged = staged.pin_memory()
        return params, staged

    def __iter__(self):
        """The next batch's rows are drawn and checked on a worker thread while the trainer's step runs (and waits on its loss): the step
        then pays one small copy and the launch, both on the current stream.  One worker draws them in order, so the rows are those of
        epoch_batches."""
        from concurrent.futures import ThreadPoolExecutor
        rows, self.epoch = self._epoch_rows(self.epoch), self.epoch + 1
        with ThreadPoolExecutor(max_workers=1, thread_name_prefix="mudpt-augment") as pool:
            ahead = pool.submit(self._stage, rows)
            while True:
                item = ahead.result()
                if item is None:
                    return
                ahead = pool.submit(self._stage, rows)
                self.last_params, staged = item
                n = self.last_params.shape[0]
                dev = staged.to(self.store.device, non_blocking=True)
                yield {"img": self.store.launch(dev[:10 * n].view(n, 10), self.size, self.mean, self.std), "label": self.store.labels[dev[10 * n:].long()],
                       "_mudpt_sharded": True}
