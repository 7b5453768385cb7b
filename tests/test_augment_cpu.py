"""No-GPU checks of the device-resident input path (mudpt_amd/augment.py, include/mudpt.h at mudpt_augment): the NumPy restatement against
Pillow byte for byte, the crop-box arithmetic, the host-side table check, the form decision and the loader's index arithmetic."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from mudpt_amd import augment, build, capi, synth
from tests import augment_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_cases.npz")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    images = [z[f"image_{i}"] for i in range(sum(k.startswith("image_") for k in z.files))]
    return z, images


def host_store(shapes, labels=None):
    """A store on the host (tables only matter) of zero images of the given (H, W)."""
    return augment.DeviceImageStore.from_arrays([np.zeros((h, w, 3), dtype=np.uint8) for h, w in shapes], labels if labels is not None else [0] * len(shapes), device="cpu")


def test_fixture_is_small_and_keeps_pillows_oddity_out(golden):
    z, images = golden
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert not any(im.shape[1] == 8 and im.shape[0] >= 900 for im in images)
    assert {int(k.rsplit("_", 1)[1]) for k in z.files if k.startswith("train_params_")} == {16, 24}


def test_restatement_equals_the_fixture(golden):
    """The archive holds Pillow's bytes (tests/golden/gen_golden_augment.py): no Pillow needed to hold the restatement to them."""
    z, images = golden
    for S in (16, 24):
        for kind in ("train", "eval"):
            params, want = z[f"{kind}_params_{S}"], z[f"{kind}_bytes_{S}"]
            got = R.augment_bytes(images, params, S)
            assert np.array_equal(got, want), (S, kind, np.argwhere(got != want)[:5])


def test_restatement_equals_pillow_on_fresh_cases(golden):
    """Fresh random sources and boxes, training and evaluation geometry: equality on every byte with the installed Pillow."""
    pytest.importorskip("PIL")
    from tests.golden.gen_golden_augment import pillow_bytes
    z, images = golden
    rng = np.random.default_rng(7)
    fresh = [rng.integers(0, 256, (int(h), int(w), 3), dtype=np.uint8) for h, w in rng.integers(9, 90, (6, 2))]
    fresh.append((rng.integers(0, 2, (31, 17, 3)) * 255).astype(np.uint8))
    for S in (16, 20):
        train = []
        for i, im in enumerate(fresh):
            for _ in range(3):
                h, w = int(rng.integers(1, im.shape[0] + 1)), int(rng.integers(1, im.shape[1] + 1))
                train.append(R.train_row(i, int(rng.integers(0, 2)), int(rng.integers(0, im.shape[0] - h + 1)), int(rng.integers(0, im.shape[1] - w + 1)), h, w, S))
        train = np.array(train, dtype=np.int32)
        evaluation = np.array([R.eval_row(i, im.shape[0], im.shape[1], S) for i, im in enumerate(fresh)], dtype=np.int32)
        for params, is_eval in ((train, False), (evaluation, True)):
            got, want = R.augment_bytes(fresh, params, S), pillow_bytes(fresh, params, S, is_eval)
            assert np.array_equal(got, want), (S, is_eval, np.argwhere(got != want)[:5])
    # the fixture's own cases against the installed Pillow too
    for S in (16, 24):
        assert np.array_equal(pillow_bytes(images, z[f"train_params_{S}"], S, False), z[f"train_bytes_{S}"])


def test_fixed_point_is_part_of_the_operation(golden):
    """Why 22-bit fixed point is specified: float64 weights give other bytes somewhere on the fixture's sources, never by more than a level."""
    z, images = golden
    worst = 0
    for row, want in zip(z["train_params_24"], z["train_bytes_24"]):
        r = R.resample(images[int(row[0])], row, 24, fixed=False)
        got = (r[:, ::-1] if row[1] else r).transpose(2, 0, 1).astype(int)
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1


def test_rrc_params_pass_the_check_and_are_deterministic(lib):
    shapes = [(37, 53), (64, 48), (4, 400), (400, 4), (1, 1), (300, 500), (224, 224)]
    store = host_store(shapes)
    idx = torch.arange(len(shapes)).repeat(40)
    g = torch.Generator().manual_seed(3)
    p = augment.rrc_params(store, idx, 32, generator=g)
    assert p.dtype == torch.int32 and p.shape == (idx.numel(), 10)
    augment.check_params(store.table, p, 32)  # every box is inside its image
    assert torch.equal(p, augment.rrc_params(store, idx, 32, generator=torch.Generator().manual_seed(3)))
    assert not torch.equal(p, augment.rrc_params(store, idx, 32, generator=torch.Generator().manual_seed(4)))
    assert torch.equal(p[:, 0], idx.int()) and set(p[:, 1].tolist()) == {0, 1}
    assert (p[:, [4, 8]] == 32).all() and (p[:, [5, 9]] == 0).all()
    H, W = store.table[idx, 1], store.table[idx, 2]
    w, h = p[:, 3].double(), p[:, 7].double()
    # the fallback: no attempt fits a 4 x 400 strip (h <= 4 would need an aspect above 4/3), so it is the central crop at the nearest allowed aspect
    wide, tall = p[(H == 4) & (W == 400)], p[(H == 400) & (W == 4)]
    assert len(wide) == 40 and (wide[:, [2, 3, 6, 7]] == torch.tensor([197, 5, 0, 4], dtype=torch.int32)).all()  # w = round(4 * 4/3) = 5, centred
    assert len(tall) == 40 and (tall[:, [2, 3, 6, 7]] == torch.tensor([0, 4, 197, 5], dtype=torch.int32)).all()  # h = round(4 / (3/4)) = 5
    # area fraction and aspect inside their bounds, up to the rounding of w and h to integers (each moves by at most 1/2)
    ordinary = (H >= 37) & (W >= 37)
    for wi, hi, Wi, Hi in zip(w[ordinary].tolist(), h[ordinary].tolist(), W[ordinary].tolist(), H[ordinary].tolist()):
        assert (wi - 0.5) * (hi - 0.5) <= 1.0 * Wi * Hi and (wi + 0.5) * (hi + 0.5) >= 0.08 * Wi * Hi
        assert (wi - 0.5) / (hi + 0.5) <= 4 / 3 and (wi + 0.5) / (hi - 0.5) >= 3 / 4
    assert len({(a, b) for a, b in zip(w[ordinary].tolist(), h[ordinary].tolist())}) > 100  # the boxes do vary
    # flip_p is honoured at both ends
    assert augment.rrc_params(store, idx, 32, flip_p=0.0, generator=g)[:, 1].sum() == 0
    assert augment.rrc_params(store, idx, 32, flip_p=1.0, generator=g)[:, 1].sum() == idx.numel()
    # a narrower scale narrows the boxes
    small = augment.rrc_params(store, torch.full((200,), 5), 32, scale=(0.08, 0.1), generator=g)
    assert (small[:, 3].double() * small[:, 7].double()).max() <= 0.1 * 300 * 500 * 1.02


def test_center_crop_params_on_odd_sizes(lib):
    shapes = [(37, 53), (53, 37), (31, 31), (20, 33), (150, 10), (10, 151), (17, 17)]
    store = host_store(shapes)
    for S in (16, 17, 24):
        p = augment.center_crop_params(store, range(len(shapes)), S)
        augment.check_params(store.table, p, S)
        for row, (H, W) in zip(p.tolist(), shapes):
            assert row == R.eval_row(row[0], H, W, S)
            _, flip, x_lo, x_len, x_out, x_off, y_lo, y_len, y_out, y_off = row
            assert (flip, x_lo, y_lo, x_len, y_len) == (0, 0, 0, W, H) and min(x_out, y_out) == S
            assert max(x_out, y_out) == int(S * max(H, W) / min(H, W))
            assert abs((x_out - S - x_off) - x_off) <= 1 and abs((y_out - S - y_off) - y_off) <= 1  # centred to within a pixel


GOOD_IMAGES = [[1, 5, 7], [1 + 105, 4, 4], [400, 1, 1]]
GOOD_ROW = [0, 1, 1, 6, 16, 0, 2, 3, 16, 0]


def _check(lib, images, rows, size=16):
    im, p = np.array(images, dtype=np.int64).reshape(-1, 3), np.array(rows, dtype=np.int32).reshape(-1, 10)
    rc = lib.mudpt_augment_check(C.c_void_p(im.ctypes.data), len(im), C.c_void_p(p.ctypes.data), len(p), size)
    return rc, lib.mudpt_last_error().decode()


def test_augment_check_refuses_each_bad_column_by_name(lib):
    assert _check(lib, GOOD_IMAGES, [GOOD_ROW, [2, 0, 0, 1, 20, 4, 0, 1, 16, 0]])[0] == 0
    bad = [("image", 0, 3), ("image", 0, -1), ("flip", 1, 2), ("flip", 1, -1), ("x_lo", 2, -1), ("x_len", 3, 0), ("x_len", 3, 7), ("x_out", 4, 0), ("x_off", 5, -1),
           ("x_off", 5, 1), ("y_lo", 6, -1), ("y_len", 7, 0), ("y_len", 7, 4), ("y_out", 8, 0), ("y_out", 8, 15), ("y_off", 9, -1), ("y_off", 9, 1)]
    for name, column, value in bad:
        row = list(GOOD_ROW)
        row[column] = value
        rc, msg = _check(lib, GOOD_IMAGES, [GOOD_ROW, row])
        assert rc == 1 and "params row 1, column " + name + " = " in msg, (name, value, msg)
    # x_out below size shows as the offset that no longer fits; the out length itself is refused below 1
    for name, column, value in (("offset", 0, 105), ("height", 1, 0), ("width", 2, 0), ("width", 2, 2 ** 31)):
        images = [list(r) for r in GOOD_IMAGES]
        images[1][column] = value
        rc, msg = _check(lib, images, [GOOD_ROW])
        assert rc == 1 and "images row 1, column " + name + " = " in msg, (name, msg)
    assert _check(lib, [[-1, 5, 7]], [])[0] == 1 and "images row 0, column offset" in lib.mudpt_last_error().decode()
    assert lib.mudpt_augment_check(None, 0, None, 0, 16) == 1 and b"null" in lib.mudpt_last_error()
    assert _check(lib, GOOD_IMAGES, [GOOD_ROW], size=0)[0] == 1
    # the Python layer raises with that message
    with pytest.raises(AssertionError, match="params row 0, column x_len"):
        augment.check_params(torch.tensor(GOOD_IMAGES), torch.tensor([[0, 0, 0, 8, 16, 0, 0, 5, 16, 0]], dtype=torch.int32), 16)


def test_augment_refuses_bad_arguments_without_a_gpu(lib):
    x = (C.c_float * 6)(*R.CLIP_MEAN, *R.CLIP_STD)
    some = C.c_void_p(C.addressof(x))  # never dereferenced: every case fails its argument check first
    args = dict(pixels_dev=some, images_dev=some, n_images=1, params_dev=some, batch=1, size=16, mean_std_host=some, out_dev=some)
    for name in ("pixels_dev", "images_dev", "params_dev", "mean_std_host", "out_dev"):
        assert capi.call("mudpt_augment", **{**args, name: None}) == 1 and b"null" in lib.mudpt_last_error(), name
    assert capi.call("mudpt_augment", **{**args, "batch": -1}) == 1 and b"batch" in lib.mudpt_last_error()
    assert capi.call("mudpt_augment", **{**args, "size": 0}) == 1 and b"size" in lib.mudpt_last_error()
    assert capi.call("mudpt_augment", **{**args, "batch": 0}) == 0  # nothing to do, nothing launched
    assert lib.mudpt_abi_version() == 7
    with pytest.raises(capi.MudptError, match="no CPU form"):
        host_store([(5, 5)]).augment(torch.tensor([R.train_row(0, 0, 0, 0, 5, 5, 16)], dtype=torch.int32), 16)


def lds_bytes(x_len, x_out, y_len, y_out, S, R_):
    """include/mudpt.h at mudpt_augment_form, by hand."""
    sx, sy = max(x_len / x_out, 1.0), max(y_len / y_out, 1.0)
    kx, ky = 2 * math.ceil(2 * sx) + 1, 2 * math.ceil(2 * sy) + 1
    rows = int((R_ - 1) * (y_len / y_out) + 4 * sy + 1) + 2
    return 3072 + 8 * S + 4 * S * kx + 128 + 64 * ky + rows * 3 * ((S + 3) // 4 * 4)


# (x_len, x_out, y_len, y_out, size) -> (form, rows per pass); every threshold of R and the TABLE / DIRECT one bracketed on both sides
AUGMENT_FORM_TABLE = [
    ((300, 224, 300, 224, 224), ("TABLE", 16)), ((5, 16, 7, 16, 16), ("TABLE", 16)), ((1, 32, 1, 32, 32), ("TABLE", 16)),
    # a 500-wide crop at size 224 (kx = 11: 13 248 bytes of tables and lookup), ever taller: rows(R) * 672 bytes on top
    ((500, 224, 400, 224, 224), ("TABLE", 16)), ((500, 224, 401, 224, 224), ("TABLE", 8)),    # R = 16: rows 39 | 40 -> 39 616 | 40 288 bytes
    ((500, 224, 692, 224, 224), ("TABLE", 8)), ((500, 224, 693, 224, 224), ("TABLE", 4)),     # R = 8 at 693: 40 672
    ((500, 224, 1055, 224, 224), ("TABLE", 4)), ((500, 224, 1056, 224, 224), ("TABLE", 2)),   # R = 4 at 1056: 40 384
    ((500, 224, 1433, 224, 224), ("TABLE", 2)), ((500, 224, 1434, 224, 224), ("TABLE", 1)),   # R = 2 at 1434: 40 096
    ((500, 224, 1791, 224, 224), ("TABLE", 1)), ((500, 224, 1792, 224, 224), ("DIRECT", 0)),  # R = 1 at 1792: 40 480
    # a 9-row strip ever wider at size 32: the x table alone, 128 kx bytes
    ((2176, 32, 9, 32, 32), ("TABLE", 16)), ((2177, 32, 9, 32, 32), ("TABLE", 8)),            # kx = 273 | 275: 40 032 at R = 16
    ((2208, 32, 9, 32, 32), ("TABLE", 8)), ((2209, 32, 9, 32, 32), ("DIRECT", 0)),            # kx = 277 | 279: 40 160 at R = 1
    # the shapes of tests/test_augment_gpu.py
    ((1300, 32, 8, 32, 32), ("TABLE", 16)), ((8, 32, 700, 32, 32), ("TABLE", 8)), ((2400, 32, 9, 32, 32), ("DIRECT", 0)), ((9, 32, 2400, 32, 32), ("DIRECT", 0)),
    ((2000, 224, 1500, 224, 224), ("DIRECT", 0)), ((1000, 224, 1000, 224, 224), ("TABLE", 1)),
]


def test_augment_form_table(lib):
    """Which form a sample takes is host arithmetic (augment_plan, exported as mudpt_augment_form): both forms write the same bytes, so only
    this table notices a wrong edit to the decision."""
    header = open(capi.HEADER_PATH).read()
    assert "#define MUDPT_AUGMENT_TABLE 0 " in header and "#define MUDPT_AUGMENT_DIRECT 1 " in header
    for args, want in AUGMENT_FORM_TABLE:
        assert augment.augment_form(*args) == want, (args, want, augment.augment_form(*args))
    assert {want[0] for _, want in AUGMENT_FORM_TABLE} == set(augment.AUGMENT_FORMS)
    # the decision is the header's formula: the largest R of 16 .. 1 whose bytes fit 40 000, over a sweep of both axes
    for S in (16, 32, 224):
        for x_len in (1, S, 3 * S, 9 * S, 40 * S, 80 * S):
            for y_len in (1, S, 2 * S + 1, 7 * S, 30 * S, 100 * S):
                fits = [R_ for R_ in (16, 8, 4, 2, 1) if lds_bytes(x_len, S, y_len, S, S, R_) <= 40000]
                assert augment.augment_form(x_len, S, y_len, S, S) == (("TABLE", fits[0]) if fits else ("DIRECT", 0)), (S, x_len, y_len)
    for args in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0)):
        assert lib.mudpt_augment_form(*args) == -1


def test_loader_arithmetic():
    images, labels = synth.synthetic_uint8_images(23, 5, seed=1, lo=8, hi=20)
    assert len({tuple(im.shape) for im in images}) > 10 and all(im.dtype == torch.uint8 for im in images)
    again, _ = synth.synthetic_uint8_images(23, 5, seed=1, lo=8, hi=20)
    assert all(torch.equal(a, b) for a, b in zip(images, again))
    store = augment.DeviceImageStore.from_arrays(images, labels, device="cpu")
    assert len(store) == 23 and store.nbytes == sum(im.numel() for im in images)
    assert torch.equal(store.labels_of([3, 1]), labels[[3, 1]])
    whole = augment.DeviceAugmentLoader(store, 6, 16, seed=5, rank=0, world=1)
    assert len(whole) == 3 and len(augment.DeviceAugmentLoader(store, 6, 16, seed=5, drop_last=False, rank=0, world=1)) == 4
    e0, e1 = whole.epoch_batches(0), whole.epoch_batches(1)
    seen = torch.cat([idx for idx, _ in e0])
    assert seen.numel() == 18 and seen.unique().numel() == 18  # drop_last: three whole batches of distinct images
    assert not torch.equal(seen, torch.cat([idx for idx, _ in e1]))  # a new permutation per epoch
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(e0, whole.epoch_batches(0)))  # ... and the same one per (seed, epoch)
    last = augment.DeviceAugmentLoader(store, 6, 16, seed=5, drop_last=False, rank=0, world=1).epoch_batches(0)[-1]
    assert last[0].numel() == 5 and last[1].shape == (5, 10)
    # two ranks' slices tile the global batch, in order, crops included
    halves = [augment.DeviceAugmentLoader(store, 6, 16, seed=5, rank=r, world=2).epoch_batches(0) for r in (0, 1)]
    for (idx, params), (i0, p0), (i1, p1) in zip(e0, *halves):
        assert torch.equal(torch.cat([i0, i1]), idx) and torch.equal(torch.cat([p0, p1]), params) and i0.numel() == 3
        assert torch.equal(params[:, 0], idx.int())
        augment.check_params(store.table, params, 16)
    with pytest.raises(ValueError, match="not divisible"):
        augment.DeviceAugmentLoader(store, 5, 16, rank=0, world=2)
    with pytest.raises(ValueError, match="no batch"):
        augment.DeviceAugmentLoader(store, 24, 16, rank=0, world=1)
    with pytest.raises(augment.StoreTooLarge, match="first 2 decoded images"):
        augment.DeviceImageStore.from_arrays(images, labels, device="cpu", max_bytes=images[0].numel() + 1)
    with pytest.raises(ValueError, match="uint8"):
        augment.DeviceImageStore.from_arrays([np.zeros((4, 4, 3), dtype=np.float32)], [0], device="cpu")
