"""GPU tests of the fused convolution (conv.hip) through its single-kernel export ``mudpt_conv2d``: against float64 under a derived bound, bit for
bit on integers, what it reads and writes, one answer per pixel whatever the batch and the tile form, and overwriting.

Destinations sit between guard rows of SENT; the source channels behind C and the weight columns behind k k C are NaN, so anything read outside
the contract shows in the output.  The float64 bound is

    |got - want| <= eps_T |want| + (K + 3) 2^-24 S,   S = |P| |W|^T + |bias| + |res|,   K = k k C,

one rounding to T plus the worst case of an fp32 sum of K exact products and two more additions in any order.  Largest ratio of error to bound
measured on an MI355X: 0.996 (tile_128x64, bf16; 0.73 .. 0.98 on the issue's six shapes in fp16, 0.95 .. 0.98 in bf16) -- eps_T is the
half-ulp of T, which a rounding reaches; DESIGN.md 4.9."""
import pytest
import torch

from mudpt_amd import capi
from tests.helpers import SENT, ok
from tests.test_resnet_gpu import DTYPES, bits, guarded, nhwc, patch_rows, untouched

pytestmark = pytest.mark.gpu
EPS = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}

# B, H, W, C, lds, k, stride, N, ldk, and per dtype (bias, residual, relu): across the rows every combination occurs with each dtype
CASES = {
    "under_one_tile": ((2, 5, 7, 8, 8, 3, 1, 16, 128), {"fp16": (1, 0, 0), "bf16": (0, 0, 1)}),       # M 70; a tap narrower than a K-step; K tail
    "channel_stride": ((2, 6, 6, 32, 48, 3, 1, 64, 320), {"fp16": (0, 1, 1), "bf16": (1, 1, 0)}),     # lds above C; a tail behind 288
    "stride2_odd": ((2, 7, 6, 16, 16, 3, 2, 48, 192), {"fp16": (1, 1, 0), "bf16": (0, 1, 1)}),        # Ho 4, Wo 3
    "many_tiles": ((3, 20, 20, 64, 64, 3, 1, 192, 576), {"fp16": (0, 0, 1), "bf16": (1, 0, 0)}),      # M 1200: ragged last row tile, 3 column tiles, no tail
    "one_by_one_res": ((2, 5, 7, 64, 64, 1, 1, 256, 64), {"fp16": (1, 1, 1), "bf16": (1, 1, 1)}),     # residual at ldres 264, ldo 272
    "one_by_one_k32": ((2, 5, 7, 32, 64, 1, 1, 64, 64), {"fp16": (0, 0, 0), "bf16": (0, 0, 0)}),      # K ends inside a K-step; NaN channels 32..63
    "one_by_one_nores": ((1, 3, 3, 16, 16, 1, 1, 32, 16), {"fp16": (0, 1, 0), "bf16": (1, 0, 1)}),    # the remaining combinations: 9 pixels
    "tile_128x128": ((1, 128, 129, 8, 8, 3, 1, 144, 72), {"fp16": (1, 1, 1), "bf16": (1, 1, 1)}),     # M 16 512 = 129 row tiles x 2 ragged column tiles
    "tile_128x64": ((2, 128, 129, 8, 16, 1, 1, 48, 8), {"fp16": (1, 0, 1), "bf16": (0, 1, 0)}),       # M 33 024 = 258 row tiles of 128 x 64
}
FORMS = {"tile_128x128": "T128x128", "tile_128x64": "T128x64"}  # every other case: T64x64
LDO = {"one_by_one_res": (264, 272)}


def make(name, dtype, integers=False, seed=0):
    """The operands of a case on the device: storage with NaN behind C / behind k k C, and the float64 reference of the T-rounded values."""
    (B, H, W, C, lds, k, stride, N, ldk), flags = CASES[name]
    has_bias, has_res, relu = flags[dtype]
    code, T = DTYPES[dtype]
    g = torch.Generator().manual_seed(1000 + seed)
    K = k * k * C
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * Ho * Wo
    ldres, ldo = LDO.get(name, (N + 8, N + 16))
    store, x = nhwc(B, H, W, C, lds, T, seed + 1)
    wst = torch.full((N, ldk), float("nan"), dtype=T, device="cuda")
    if integers:
        store[:, :C] = torch.randint(-2, 3, (B * H * W, C), generator=g).to(T).cuda()
        wst[:, :K] = torch.randint(-1, 2, (N, K), generator=g).to(T).cuda()
        bias = torch.randint(-8, 9, (N,), generator=g).float().cuda()
        rs = torch.randint(-8, 9, (M, N), generator=g).to(T)
    else:
        wst[:, :K] = (torch.randn(N, K, generator=g) / K ** 0.5).to(T).cuda()
        bias = torch.randn(N, generator=g).cuda()
        rs = torch.randn(M, N, generator=g).to(T)
    res = torch.full((M, ldres), float("nan"), dtype=T, device="cuda")
    res[:, :N] = rs.cuda()
    x = store[:, :C].reshape(B, H, W, C)
    P = (patch_rows(x, stride, 9 * C) if k == 3 else x.reshape(-1, C)).double()
    Wd = wst[:, :K].double()
    want, S = P @ Wd.T, P.abs() @ Wd.abs().T
    if has_bias:
        want, S = want + bias.double(), S + bias.double().abs()
    if has_res:
        want, S = want + res[:, :N].double(), S + res[:, :N].double().abs()
    if relu:
        want = want.clamp_min(0)
    args = dict(dtype=code, src=store, B=B, H=H, W=W, C=C, lds=lds, k=k, stride=stride, w=wst, ldk=ldk, bias=bias if has_bias else None,
                residual=res if has_res else None, ldres=ldres if has_res else 0, ldo=ldo, N=N, relu=relu)
    return args, want, S, (M, N, K, ldo, T)


_cache = {}


def run(name, dtype, integers=False):
    """One launch of a case into a guarded destination; computed once and shared (nothing changes it)."""
    key = (name, dtype, integers)
    if key not in _cache:
        args, want, S, (M, N, K, ldo, T) = make(name, dtype, integers)
        buf, dst = guarded(M, ldo, T)
        ok(capi.load(), capi.call("mudpt_conv2d", out=dst, **args))
        _cache[key] = (args, want, S, buf, dst, (M, N, K, ldo, T))
    return _cache[key]


def test_cases_reach_every_tile_form_and_epilogue():
    lib = capi.load()
    seen = {}
    for name, ((B, H, W, C, lds, k, stride, N, ldk), flags) in CASES.items():
        M = B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        form = lib.mudpt_conv2d_form(M, N)
        assert form == capi._DEFINES["CONV_" + FORMS.get(name, "T64x64")], name
        seen[form] = seen.get(form, 0) + 1
    assert sorted(seen) == [0, 1, 2]
    for dtype in DTYPES:
        assert {flags[dtype] for _, flags in CASES.values()} == {(b, r, a) for b in (0, 1) for r in (0, 1) for a in (0, 1)}, dtype


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_against_float64_reads_and_writes(name, dtype):
    """Within one rounding to T plus the fp32 sum's worst case of the float64 result of the same T operands; the guard rows and the columns from
    N on still hold SENT; no NaN in the output: no channel behind C, no weight column behind k k C, nothing outside the image was read."""
    args, want, S, buf, dst, (M, N, K, ldo, T) = run(name, dtype)
    got = dst[:, :N].double()
    assert torch.isfinite(got).all()
    err, bound = (got - want).abs(), EPS[dtype] * want.abs() + (K + 3) * 2.0 ** -24 * S
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"conv2d {name} {dtype}: M {M} N {N} K {K}, largest |error| / bound {ratio:.3f}")
    assert (err <= bound).all(), ratio
    untouched(buf, M, N)
    if args["relu"]:
        assert (got >= 0).all() and (got == 0).any()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["many_tiles", "stride2_odd", "tile_128x128", "one_by_one_res"])
def test_exact_on_integers(name, dtype):
    """x in {-2 .. 2}, w in {-1, 0, 1}, integer bias and residual: every partial sum is an integer below 2^24, exact in fp32 in any order, so the
    output is T(want) bit for bit -- a wrong tap, border or tile seam cannot hide in rounding."""
    args, want, S, buf, dst, (M, N, K, ldo, T) = run(name, dtype, integers=True)
    assert want.abs().max().item() < 2 ** 24
    assert torch.equal(bits(dst[:, :N]), bits(want.to(T)))
    untouched(buf, M, N)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_one_pixel_one_answer(dtype):
    """Image 1 of the 20 x 20 case alone (B = 1: 400 pixels, other tiles) gives the bits it had in the batch; a second run of the whole call gives
    the same bits; and a batch large enough for the 128 x 128 tile gives every image the bits the 64 x 64 tile gave it."""
    lib = capi.load()
    args, want, S, buf, dst, (M, N, K, ldo, T) = run("many_tiles", dtype)
    B, H, W, lds = args["B"], args["H"], args["W"], args["lds"]
    buf2, dst2 = guarded(M, ldo, T)
    ok(lib, capi.call("mudpt_conv2d", out=dst2, **args))
    assert torch.equal(bits(dst2[:, :N]), bits(dst[:, :N]))
    one = dict(args, B=1, src=args["src"][H * W:2 * H * W])
    buf1, dst1 = guarded(H * W, ldo, T)
    ok(lib, capi.call("mudpt_conv2d", out=dst1, **one))
    assert torch.equal(bits(dst1[:, :N]), bits(dst[H * W:2 * H * W, :N]))
    untouched(buf1, H * W, N)
    rep = 44  # 132 images: M 52 800 = 413 row tiles x 2 column tiles of 128 x 128
    assert lib.mudpt_conv2d_form(rep * M, N) == capi._DEFINES["CONV_T128x128"] and lib.mudpt_conv2d_form(M, N) == capi._DEFINES["CONV_T64x64"]
    big = dict(args, B=rep * B, src=args["src"].repeat(rep, 1))
    bufb, dstb = guarded(rep * M, ldo, T)
    ok(lib, capi.call("mudpt_conv2d", out=dstb, **big))
    assert torch.equal(bits(dstb[:, :N].reshape(rep, M, N)), bits(dst[:, :N])[None].expand(rep, M, N))
    untouched(bufb, rep * M, N)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_a_smaller_second_call_overwrites_its_own_rows_only(dtype):
    args, want, S, buf, dst, (M, N, K, ldo, T) = run("channel_stride", dtype)
    lib = capi.load()
    first = dst.clone()
    buf2, dst2 = guarded(M, ldo, T)
    dst2.copy_(first)
    store2, x2 = nhwc(1, 3, 3, args["C"], args["lds"], T, 77)
    small = dict(args, B=1, H=3, W=3, src=store2)
    ok(lib, capi.call("mudpt_conv2d", out=dst2, **small))
    alone_buf, alone = guarded(9, ldo, T)
    ok(lib, capi.call("mudpt_conv2d", out=alone, **small))
    assert torch.equal(bits(dst2[:9, :N]), bits(alone[:, :N])) and not torch.equal(bits(dst2[:9, :N]), bits(first[:9, :N]))
    assert torch.equal(bits(dst2[9:]), bits(first[9:])) and torch.equal(bits(dst2[:9, N:]), bits(first[:9, N:]))
    untouched(buf2, M, N)
    assert torch.isfinite(alone[:, :N]).all()


def test_refusals_leave_the_destination_alone():
    lib = capi.load()
    args, want, S, (M, N, K, ldo, T) = make("under_one_tile", "fp16")
    buf, dst = guarded(M, ldo, T)
    for change, word in (({"k": 2}, "k 2"), ({"stride": 3}, "stride 3"), ({"C": 12}, "C 12"), ({"ldk": 64}, "ldk 64"), ({"N": 24}, "N 24"), ({"ldo": 8}, "ldo 8"),
                         ({"src": None}, "null")):
        rc = capi.call("mudpt_conv2d", out=dst, **dict(args, **change))
        torch.cuda.synchronize()
        assert rc == 1 and word in lib.mudpt_last_error().decode(), (change, lib.mudpt_last_error())
    assert (buf == SENT).all()
