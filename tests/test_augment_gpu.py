"""GPU tests of mudpt_augment (mudpt_amd/csrc/augment.hip) through DeviceImageStore: the batch must be BIT-EQUAL to
((bytes.float() / 255 - mean) / std) computed by torch on the CPU from the bytes of tests/augment_reference.py (which the CPU tests hold to
Pillow).  Equality is derived, not a tolerance: the resample is integer arithmetic on weights both sides compute with the same IEEE fp64
operations, and the three fp32 operations are correctly rounded on both sides."""
import os

import numpy as np
import pytest
import torch

from mudpt_amd import augment
from tests import augment_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_cases.npz")
SENTINEL = -12345.5


def sources():
    rng = np.random.default_rng(11)
    rnd = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # noqa: E731
    return {"a": rnd(37, 53), "b": rnd(64, 48), "c": (rng.integers(0, 2, (20, 33, 3)) * 255).astype(np.uint8), "wide": rnd(8, 1300), "tall": rnd(700, 8),
            "photo": rnd(200, 300), "strip": rnd(9, 2400), "pole": rnd(2400, 9)}


NAMES = ("a", "b", "c", "wide", "tall", "photo", "strip", "pole")


def resample_cases(S):
    """(name, row, form) at output size S: one batch that mixes source sizes, repeats image indices and alternates flips."""
    i = {n: k for k, n in enumerate(NAMES)}
    T = R.train_row
    return [
        ("1x1 crop", T(i["a"], 0, 36, 52, 1, 1, S), ("TABLE", 16)),
        ("1x33 crop", T(i["a"], 1, 5, 10, 1, 33, S), ("TABLE", 16)),
        ("5x7 crop upscaled", T(i["b"], 0, 7, 9, 5, 7, S), ("TABLE", 16)),
        ("crop equal to S", T(i["b"], 1, 11, 13, S, S, S), ("TABLE", 16)),
        ("0/255 source, whole", T(i["c"], 0, 0, 0, 20, 33, S), ("TABLE", 16)),
        ("0/255 source, 3x4 crop upscaled (both clamps)", T(i["c"], 1, 3, 4, 3, 4, S), ("TABLE", 16)),
        ("8x1300: 163 horizontal taps at S = 32", T(i["wide"], 0, 0, 0, 8, 1300, S), ("TABLE", 16)),
        ("700x8: 88 vertical taps at S = 32", T(i["tall"], 1, 0, 0, 700, 8, S), ("TABLE", 8)),
        ("300x200 downscale", T(i["photo"], 0, 0, 0, 200, 300, S), ("TABLE", 16)),
        ("300x200, a crop of it flipped", T(i["photo"], 1, 13, 21, 150, 222, S), ("TABLE", 16)),
        ("9x2400: x table too large", T(i["strip"], 0, 0, 0, 9, 2400, S), ("DIRECT", 0)),
        ("2400x9: no band of source rows fits", T(i["pole"], 1, 0, 0, 2400, 9, S), ("DIRECT", 0)),
        ("a again", T(i["a"], 0, 2, 3, 30, 41, S), ("TABLE", 16)),
    ] + ([  # fewer output rows per pass over the source rows, down to one (tests/test_augment_cpu.py lds_bytes: 39 200, 36 640, 36 448 bytes)
        ("1200x9: 4 rows per pass", T(i["pole"], 0, 100, 0, 1200, 9, S), ("TABLE", 4)),
        ("1400x9: 2 rows per pass", T(i["pole"], 1, 1000, 0, 1400, 9, S), ("TABLE", 2)),
        ("1600x9: 1 row per pass", T(i["pole"], 0, 800, 0, 1600, 9, S), ("TABLE", 1)),
    ] if S == 32 else [])


@pytest.fixture(scope="module")
def world():
    """The store (sources packed at odd offsets) and, per size, the reference batch: computed once, shared, never written."""
    src = sources()
    images = [src[n] for n in NAMES]
    pixels, table = R.pack(images, gap=1, odd=True)  # every image at an odd byte offset; odd widths among them
    assert all(int(o) % 2 == 1 for o in table[:, 0]) and {int(o) % 4 for o in table[:, 0]} == {1, 3}
    store = augment.DeviceImageStore(torch.from_numpy(pixels), torch.from_numpy(table), torch.arange(len(images)), "cuda:0")
    ref = {}
    for S in (16, 24, 32):
        params = np.array([row for _, row, _ in resample_cases(S)], dtype=np.int32)
        ref[S] = (torch.from_numpy(params), R.normalize(R.augment_bytes(images, params, S)))
    return store, images, ref


def run(store, params, S, **kw):
    out = store.augment(params, S, **kw)
    torch.cuda.synchronize()
    return out.cpu()


def assert_bit_equal(got, want, what=""):
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    same = got.view(torch.int32) == want.view(torch.int32)
    assert same.all(), (what, int((~same).sum()), (~same).nonzero()[:4].tolist())


@pytest.mark.parametrize("S", [16, 24, 32])
def test_resample_cases_bit_equal(world, S):
    store, _, ref = world
    params, want = ref[S]
    got = run(store, params, S)
    for n, (name, _, _) in enumerate(resample_cases(S)):
        assert_bit_equal(got[n], want[n], name)
    assert want.min() < -1.7 and want.max() > 2.0  # both clamps are in the batch: bytes 0 and 255 after normalisation


def test_every_case_takes_the_form_it_names_and_both_forms_are_reached():
    reached = set()
    for S in (16, 24, 32):
        for name, row, form in resample_cases(S):
            got = augment.augment_form(row[3], row[4], row[7], row[8], S)
            assert got == form, (S, name, got)
            reached.add(got)
    assert {f for f, _ in reached} == set(augment.AUGMENT_FORMS) and {r for _, r in reached} >= {16, 8, 4, 2, 1}
    # the tap counts the case names promise: 2 * support + 1 taps in the interior
    assert [len(k) for _, k in R.axis_weights(1300, 32, 0, 32)][16] == 163 and [len(k) for _, k in R.axis_weights(700, 32, 0, 32)][16] == 88


def test_both_forms_write_the_same_bytes(world):
    """The same crop geometry at two output sizes' worth of LDS need: a 9 x 2400 strip takes DIRECT at S = 32; the same strip cut to 2176
    columns takes TABLE.  Both equal the reference (above and here), and rows of one batch take different forms side by side."""
    store, images, _ = world
    strip = NAMES.index("strip")
    params = np.array([R.train_row(strip, 0, 0, 0, 9, 2400, 32), R.train_row(strip, 1, 0, 0, 9, 2176, 32), R.train_row(strip, 0, 0, 7, 9, 2209, 32)], dtype=np.int32)
    assert [augment.augment_form(r[3], r[4], r[7], r[8], 32)[0] for r in params] == ["DIRECT", "TABLE", "DIRECT"]
    assert_bit_equal(run(store, torch.from_numpy(params), 32), R.normalize(R.augment_bytes(images, params, 32)))


def test_size_224(world):
    """The production size, B = 2: a random crop and a whole image of sources of 250 - 400 pixels a side, one flipped; other mean / std."""
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (300, 400, 3), dtype=np.uint8), rng.integers(0, 256, (251, 263, 3), dtype=np.uint8)]
    pixels, table = R.pack(images, gap=3)
    store = augment.DeviceImageStore(torch.from_numpy(pixels), torch.from_numpy(table), torch.zeros(2), "cuda:0")
    params = np.array([R.train_row(0, 1, 17, 40, 231, 305, 224), R.train_row(1, 0, 0, 0, 251, 263, 224)], dtype=np.int32)
    assert [augment.augment_form(r[3], r[4], r[7], r[8], 224) for r in params] == [("TABLE", 16), ("TABLE", 16)]
    want_bytes = R.augment_bytes(images, params, 224)
    assert_bit_equal(run(store, torch.from_numpy(params), 224), R.normalize(want_bytes))
    mean, std = (0.5, 0.25, 0.125), (0.3, 1.0, 7.0)
    assert_bit_equal(run(store, torch.from_numpy(params), 224, mean=mean, std=std), R.normalize(want_bytes, mean, std))


def test_batch_of_300_and_guard_rows(world):
    """B = 300 at S = 16 (more workgroups than compute units, more samples than any 8-bit or 256-entry assumption holds) into a batch buffer
    with two sentinel-filled images past B: those stay untouched."""
    store, images, _ = world
    g = torch.Generator().manual_seed(9)
    idx = torch.randint(0, 3, (300,), generator=g)  # the three small sources, each many times
    params = augment.rrc_params(store, idx, 16, generator=g)
    out = torch.full((302, 3, 16, 16), SENTINEL, device="cuda:0")
    got = store.augment(params, 16, out=out)
    torch.cuda.synchronize()
    assert got.shape[0] == 300 and got.data_ptr() == out.data_ptr()
    assert_bit_equal(got.cpu(), R.normalize(R.augment_bytes(images, params.numpy(), 16)))
    assert (out[300:] == SENTINEL).all()
    assert store.augment(params[:0], 16).shape == (0, 3, 16, 16)


@pytest.mark.parametrize("S", [17, 18])
def test_sizes_that_are_no_multiple_of_four_and_an_unaligned_batch(world, S):
    """S % 4 != 0, or a batch that does not start on 16 bytes: the scalar-store path of the vertical pass."""
    store, images, _ = world
    params = np.array([row for _, row, _ in resample_cases(S)][:6] + [resample_cases(S)[9][1]], dtype=np.int32)
    want = R.normalize(R.augment_bytes(images, params, S))
    assert_bit_equal(run(store, torch.from_numpy(params), S), want)
    if S == 18:
        p16 = np.array([row for _, row, _ in resample_cases(16)][:6], dtype=np.int32)
        flat = torch.full((6 * 3 * 16 * 16 + 8,), SENTINEL, device="cuda:0")
        out = flat[1:1 + 6 * 3 * 16 * 16].view(6, 3, 16, 16)
        assert out.data_ptr() % 16 == 4
        store.augment(torch.from_numpy(p16), 16, out=out)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), R.normalize(R.augment_bytes(images, p16, 16)))
        assert flat[0].item() == SENTINEL and (flat[-7:] == SENTINEL).all()


def test_fixture_rows_equal_pillows_bytes():
    """tests/golden/augment_cases.npz: Pillow's own bytes for training rows and for the evaluation geometry (Resize + CenterCrop)."""
    z = np.load(GOLDEN)
    images = [z[f"image_{i}"] for i in range(5)]
    pixels, table = R.pack(images, gap=1)
    store = augment.DeviceImageStore(torch.from_numpy(pixels), torch.from_numpy(table), torch.zeros(5), "cuda:0")
    for S in (16, 24):
        for kind in ("eval", "train"):
            assert_bit_equal(run(store, torch.from_numpy(z[f"{kind}_params_{S}"]), S), R.normalize(z[f"{kind}_bytes_{S}"]), (kind, S))
        assert torch.equal(augment.center_crop_params(store, range(5), S), torch.from_numpy(z[f"eval_params_{S}"]))


def test_trainer_end_to_end_on_the_synthetic_store(tmp_path, monkeypatch):
    """MUDPT_DEVICE_DATA=1 with the shipped transforms: a dassl_lite MuDPT trainer takes its batches from the DeviceAugmentLoader over the
    synthetic uint8 store; two steps run, and each step's images are the kernel's output for the loader's rows.  Without the opt-in (or
    with another interpolation) the loader is the DevicePrefetcher as before."""
    from mudpt_amd import dassl_lite, trainer
    from mudpt_amd.prefetch import DevicePrefetcher
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_DEVICE_DATA"):
        monkeypatch.delenv(var, raising=False)

    def make():
        cfg = dassl_lite.default_cfg()
        cfg.OUTPUT_DIR = str(tmp_path)
        cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.LR = 1, 0, 0.01
        cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 10, 4
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 4, 4
        cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH = 4, 12
        cfg.INPUT.TRANSFORMS, cfg.INPUT.INTERPOLATION = ("random_resized_crop", "random_flip", "normalize"), "bicubic"
        return dassl_lite.build_trainer(cfg)

    plain = make()
    assert isinstance(plain.train_loader_x, DevicePrefetcher) and not hasattr(plain, "device_store")
    plain.cfg.INPUT.INTERPOLATION = "bilinear"  # the opt-in under a configuration the kernel does not reproduce: refused, host loader
    monkeypatch.setenv("MUDPT_DEVICE_DATA", "1")
    assert trainer.device_data_loader(plain, plain.train_loader_x, 0) is None
    plain.cfg.INPUT.INTERPOLATION = "bicubic"
    with monkeypatch.context() as m:  # ... and when the store would not fit a quarter of the free device memory
        m.setattr(torch.cuda, "mem_get_info", lambda *a: (400000, 10 ** 9))
        assert trainer.device_data_loader(plain, plain.train_loader_x, 0) is None and not hasattr(plain, "device_store")
    plain.model.close()

    t = make()
    loader = t.train_loader_x
    assert isinstance(loader, augment.DeviceAugmentLoader) and len(loader) == 10 // 4 and len(t.device_store) == 10
    assert len({tuple(r[1:]) for r in t.device_store.table.tolist()}) > 5  # varied sizes
    t.set_model_mode("train")
    t.num_batches = len(loader)
    losses, seen = [], []
    for t.batch_idx, batch in enumerate(loader):
        assert batch["img"].is_cuda and batch["img"].shape == (4, 3, 224, 224) and batch["label"].is_cuda and batch["_mudpt_sharded"]
        assert torch.equal(batch["img"], t.device_store.augment(loader.last_params, 224))
        assert torch.equal(batch["label"], t.device_store.labels_of(loader.last_params[:, 0].long()))
        seen += loader.last_params[:, 0].tolist()
        losses.append(t.forward_backward(batch)["loss"])
    assert len(losses) == 2 and all(np.isfinite(l) for l in losses) and len(set(seen)) == 8
    # one image of the last batch against the reference: the loader's rows on the store's own bytes
    n = int(loader.last_params[0, 0])
    off, H, W = t.device_store.table[n].tolist()
    image = t.device_store.pixels[off:off + 3 * H * W].cpu().numpy().reshape(H, W, 3)
    row = loader.last_params[0].clone()
    row[0] = 0
    assert_bit_equal(batch["img"][0].cpu(), R.normalize(R.augment_bytes([image], row[None].numpy(), 224))[0])
    t.model.close()
