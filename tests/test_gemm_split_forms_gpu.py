"""The second pass of a split-operand GEMM (common.h LoMode; mudpt_gemm_split) in every form a split operand can take, at strides, ragged edges
and K depths, through the C ABI -- the harness of test_gemm_forms_gpu.py with two more operands.

The GEMM does not care that A_lo is a remainder, so the exact cases give it an INDEPENDENT small-integer matrix: A_lo in [-3, 3] (as T for
lo_mode 1, as e4m3 codes for lo_mode 2: small integers are exact in e4m3) and B8 = e4m3 codes of an integer matrix in [-4, 4] that differs
from B, so that a second pass that reads B, or B's stride, shows.  The kernel scales the e4m3 activations by 2^-12; with the E8M0 weight scale
137 (2^10) the second pass adds exactly (A_lo . B8^T) / 4: every product and partial sum is a multiple of 1/4 below 2^22, and the results are
compared for equality.  Every operand is a column-offset window with guard rows; pads and guards hold NaN (T), 0x7F (e4m3 NaN: bytes K .. 2 ld
of every window row among them) or a sentinel (outputs) that must survive bit for bit.  Each case names its form (helpers.GEMM_SPLIT_CASES;
tests/test_capi_cpu.py holds the table at 256 units without a GPU) and mudpt_gemm_form confirms it before the launch."""
import functools
import math

import pytest
import torch

from mudpt_amd import capi
from tests.helpers import (EPS, GEMM_GUARD_ROWS, GEMM_SPLIT_B8_SCALE, GEMM_SPLIT_B8_SCALE_ONE, GEMM_SPLIT_CASES, GEMM_SPLIT_GELU_ALL_PAIRS,
                           GEMM_SPLIT_GELU_CASES, GEMM_SPLIT_PATCH_CASES, GEMM_SPLIT_SCALE_CASES, SENT, check_split_pair, gemm_split_gelu_case,
                           gemm_windows, ok, refused)
from tests.test_gemm_forms_gpu import DT, assert_outside_untouched, device_cus, exact_operands, lib, on_this_device, windowed  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

G = GEMM_GUARD_ROWS
NAN8 = 0x7F   # e4m3 NaN: pads and guards of the byte operands
SENT_LO = 0x5A  # every byte of an out1_lo buffer before the launch
BY_NAME = {c.name: c for c in GEMM_SPLIT_CASES}


def e4m3_codes(x):
    """OCP e4m3 bytes of a float tensor (exact for the small integers of the exact cases)."""
    return x.float().to(torch.float8_e4m3fn).view(torch.uint8)


def byte_window(pad_off, width):
    """(pad, off) in BYTES of a byte operand of `width` bytes that keeps the row stride of its T counterpart (2 (width + pad) bytes)."""
    return 2 * pad_off[0] + width, 2 * pad_off[1]


def lo_output(rows, N, pad_off, mode, tt):
    """The out1_lo buffer, every byte SENT_LO, rows of 2 (N + pad) bytes, and its window: N values of T (mode 1) or N bytes (mode 2) per row."""
    pad, off = pad_off
    buf = torch.full((rows + 2 * G, 2 * (N + pad)), SENT_LO, dtype=torch.uint8, device="cuda")
    win = buf.view(tt)[G:G + rows, off:off + N] if mode == 1 else buf[G:G + rows, 2 * off:2 * off + N]
    return buf, win


def run_split(lib, dtype, epi, case, ops, b8_scale=GEMM_SPLIT_B8_SCALE, windows=True, out1_lo_mode=0):
    """Launch epilogue `epi` of `case` on the operands `ops` (CPU tensors: A, B, and by case.lo_mode A_lo (T values) or A_lo8 / B8 (codes);
    bias, aux, pos as test_gemm_forms_gpu.run_windowed), every operand a guarded window (windows=False: contiguous, still guarded).  Asserts the
    form before the launch and that nothing outside the output windows changed; returns the output windows (out0, out1, out1_lo)."""
    dt, tt = DT[dtype]
    M, N, K, lo = case.M, case.N, case.K, case.lo_mode
    w = gemm_windows(case, windows)
    f32_out = epi in (capi.EPI_RESIDUAL, capi.EPI_PATCH, capi.EPI_STORE_F32)
    out_rows, written = M, None
    patches = seq_len = 0
    if epi == capi.EPI_PATCH:
        patches, seq_len = case.patch
        assert M % patches == 0
        out_rows = M // patches * seq_len
        written = (torch.arange(out_rows) % seq_len - 1).remainder(seq_len) < patches  # rows 1 .. P of every sequence
    _, A = windowed(M, K, w["A"], tt, float("nan"), ops["A"])
    _, B = windowed(N, K, w["B"], tt, float("nan"), ops["B"])
    A_lo = B8 = None
    if lo == 1:
        _, A_lo = windowed(M, K, w["A_lo"], tt, float("nan"), ops["A_lo"])
        assert A_lo.stride(0) == A.stride(0)
    elif lo == 2:
        _, A_lo = windowed(M, K, byte_window(w["A_lo"], K), torch.uint8, NAN8, ops["A_lo8"])
        _, B8 = windowed(N, K, byte_window(w["B8"], K), torch.uint8, NAN8, ops["B8"])
        assert A_lo.stride(0) == 2 * A.stride(0) and B8.stride(0) == 2 * B.stride(0)
    buf0, out0 = windowed(out_rows, N, w["out0"], torch.float32 if f32_out else tt, SENT)
    buf1, out1 = windowed(M, N, w["out1"], tt, SENT) if epi == capi.EPI_GELU else (None, None)
    bufl, out1_lo = lo_output(M, N, w["out1_lo"], out1_lo_mode, tt) if out1_lo_mode else (None, None)
    aux = None
    if epi == capi.EPI_RESIDUAL:
        _, aux = windowed(M, N, w["aux"], torch.float32, float("nan"), ops["aux"])
    bias = ops["bias"].cuda() if ops.get("bias") is not None and epi != capi.EPI_PATCH else None
    pos = ops["pos"].cuda() if epi == capi.EPI_PATCH else None
    ldo1 = out1.stride(0) if out1 is not None else N + w["out1"][0]
    ldaux = aux.stride(0) if aux is not None else N + w["aux"][0]
    got = lib.mudpt_gemm_form(epi, M, N, K, out0.stride(0), ldo1, ldaux, lo, case.variant, device_cus())
    want = capi.GEMM_FORMS.index(case.form) | 1 << 8
    assert got == want, f"{case.name} epilogue {epi}: form {capi.GEMM_FORMS[got & 0xff] if got >= 0 else got}, the case is there for {case.form}"
    patch = dict(patches=patches, seq_len=seq_len, pos=pos) if epi == capi.EPI_PATCH else {}
    ok(lib, capi.call("mudpt_gemm_split_patch" if patch else "mudpt_gemm_split", dtype=dt, epilogue=epi, M=M, N=N, K=K, A=A, A_lo=A_lo, lo_mode=lo, lda=A.stride(0), B=B,
                      B8=B8, b8_scale=b8_scale, ldb=B.stride(0), bias=bias, out0=out0, ldo0=out0.stride(0), out1=out1, out1_lo=out1_lo, out1_lo_mode=out1_lo_mode,
                      ldo1=out1.stride(0) if out1 is not None else 0, aux=aux, ldaux=aux.stride(0) if aux is not None else 0, variant=case.variant, **patch))
    assert_outside_untouched(buf0, out_rows, N, w["out0"], SENT, written)
    if buf1 is not None:
        assert_outside_untouched(buf1, M, N, w["out1"], SENT)
    if bufl is not None:  # in bytes: 2 N per window row (T remainders) or N (e4m3: bytes N .. 2 ldo1 of every row keep the sentinel)
        assert_outside_untouched(bufl, M, 2 * N if out1_lo_mode == 1 else N, (0, 2 * w["out1_lo"][1]), SENT_LO)
    return out0, out1, out1_lo


@functools.lru_cache(maxsize=1)  # the dtypes of a case run back to back and share it
def split_exact_operands(M, N, K, patches, lo_mode):
    """exact_operands plus an independent integer low half A_lo in [-3, 3] and, for the e4m3 pass, integer weights B8 in [-4, 4] that differ
    from B; "second" = the exact product the second pass adds at net scale 1: A_lo . B^T (lo_mode 1) or A_lo . B8^T (lo_mode 2)."""
    ops = dict(exact_operands(M, N, K, patches))
    g = torch.Generator().manual_seed(M + N + K + 1)
    ops["A_lo"] = torch.randint(-3, 4, (M, K), generator=g).float()
    assert not torch.equal(ops["A_lo"], ops["A"])
    if lo_mode == 2:
        b8 = ((2 * torch.arange(N).view(N, 1) + torch.arange(K).view(1, K)) % 9 - 4).float()
        assert (b8 != ops["B"]).float().mean().item() > 0.5
        ops["A_lo8"], ops["B8"] = e4m3_codes(ops["A_lo"]), e4m3_codes(b8)
        assert torch.equal(ops["B8"].view(torch.float8_e4m3fn).float(), b8) and torch.equal(ops["A_lo8"].view(torch.float8_e4m3fn).float(), ops["A_lo"])
        ops["second"] = ops["A_lo"] @ b8.t()
    else:
        ops["second"] = ops["A_lo"] @ ops["B"].t()
    assert 4 * (ops["acc"].abs().max().item() + ops["second"].abs().max().item() + 16) < 2 ** 24  # multiples of 1/4, all exact in fp32
    return ops


def assert_exact(case, dtype, epi, ops, out0, factor):
    """out0 == first pass + factor * second pass (+ bias / aux / pos), element for element."""
    got = out0.cpu()
    acc = ops["acc"] + ops["second"] * factor
    if epi == capi.EPI_PATCH:
        Pn, L = case.patch
        ref = (acc.view(-1, Pn, case.N) + ops["pos"][1:]).reshape(-1, case.N)  # no bias: the patch embedding has none
        got = got.view(-1, L, case.N)[:, 1:1 + Pn].reshape(-1, case.N)
    elif epi == capi.EPI_RESIDUAL:
        ref = ops["aux"] + acc + ops["bias"]
    else:
        ref = acc + ops["bias"]
        if epi == capi.EPI_STORE:
            ref = ref.to(DT[dtype][1])
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, (f"{case.name} {dtype} epilogue {epi}: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}: "
                              f"{got[tuple(bad[0])].item()} != {ref[tuple(bad[0])].item()}")


def second_pass_factor(case, b8_scale=GEMM_SPLIT_B8_SCALE):
    """Net scale of the second pass: 1 for T remainders; 2^(b8_scale - 127) on the weights x 2^-12 on the activations for e4m3."""
    return 1.0 if case.lo_mode == 1 else 2.0 ** (b8_scale - 127 - 12)


def dtypes_of(lo_mode):
    return ("bf16", "fp16") if lo_mode == 1 else ("fp16",)  # the e4m3 pass exists for fp16 operands only


EXACT = [pytest.param(c, d, id=f"{c.name}-{d}") for c in GEMM_SPLIT_CASES for d in dtypes_of(c.lo_mode)]


@pytest.mark.parametrize("case,dtype", EXACT)
def test_split_gemm_form_exact_strided_guarded(lib, case, dtype):
    """Bit-exact two-pass results of every form on windowed operands with ragged M and N, nothing written outside the output window."""
    case = on_this_device(case)
    ops = split_exact_operands(case.M, case.N, case.K, 0, case.lo_mode)
    for epi in case.epis:
        out0, _, _ = run_split(lib, dtype, epi, case, ops)
        assert_exact(case, dtype, epi, ops, out0, second_pass_factor(case))


@pytest.mark.parametrize("name", GEMM_SPLIT_SCALE_CASES)
def test_split_gemm_weight_scale_is_read(lib, name):
    """One case per kernel family again with the E8M0 weight scale 139 (net factor 1): a scale that is ignored, or taken from the wrong
    operand, shows against the run at 137 (net factor 1/4)."""
    case = on_this_device(BY_NAME[name])
    ops = split_exact_operands(case.M, case.N, case.K, 0, case.lo_mode)
    assert second_pass_factor(case, GEMM_SPLIT_B8_SCALE_ONE) == 1.0 and second_pass_factor(case) == 0.25
    for epi in case.epis:
        out0, _, _ = run_split(lib, "fp16", epi, case, ops, b8_scale=GEMM_SPLIT_B8_SCALE_ONE)
        assert_exact(case, "fp16", epi, ops, out0, 1.0)


@pytest.mark.parametrize("case", GEMM_SPLIT_PATCH_CASES, ids=lambda c: c.name)
def test_split_gemm_patch_epilogue_exact(lib, case):
    """The patch-embed epilogue behind a split operand (mudpt_gemm_split_patch; what the parity mode's vision tower runs after the split
    patchify), exact and guarded: rows 1 .. P of every sequence are written, row 0 and everything else keep the sentinel."""
    ops = split_exact_operands(case.M, case.N, case.K, case.patch[0], case.lo_mode)
    out0, _, _ = run_split(lib, "fp16", capi.EPI_PATCH, case, ops)
    assert_exact(case, "fp16", capi.EPI_PATCH, ops, out0, second_pass_factor(case))


# ---- QuickGELU epilogue with a split input and a split output ------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def split_random_operands(M, N, K, dtype, lo_mode):
    """Random operands with A_lo a TRUE remainder (as _split_operand of test_exact_gpu.py, for either T) and u_ref = the float64 contraction of
    the operands as quantised: hi . W^T + decoded(lo) . (W or its e4m3 copy)^T + bias."""
    tt = DT[dtype][1]
    g = torch.Generator().manual_seed(M + N + K + lo_mode)
    A32 = torch.randn(M, K, generator=g) * 1.5
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(tt)
    ops = {"A": A32.to(tt), "B": W, "bias": torch.randn(N, generator=g), "b8_scale": 127}
    rem = A32 - ops["A"].float()
    u = ops["A"].double() @ W.double().t()
    if lo_mode == 1:
        ops["A_lo"] = rem.to(tt)
        u += ops["A_lo"].double() @ W.double().t()
    elif lo_mode == 2:
        q = (rem * 4096.0).clamp(-448, 448).to(torch.float8_e4m3fn)
        shift = int(math.floor(math.log2(448.0 / W.float().abs().max().item())))
        w8 = (W.float() * 2.0 ** shift).to(torch.float8_e4m3fn)
        ops["A_lo8"], ops["B8"], ops["b8_scale"] = q.view(torch.uint8), w8.view(torch.uint8), 127 - shift
        u += (q.float().double() / 4096.0) @ (w8.float().double() / 2.0 ** shift).t()
    ops["u"] = u + ops["bias"].double()
    return ops


GELU = [pytest.param(c, lo, d, id=f"{c.name}-lo{lo}-{d}") for c in GEMM_SPLIT_GELU_CASES
        for lo in ((0, 1, 2) if c.name in GEMM_SPLIT_GELU_ALL_PAIRS else (1, 2)) for d in (("fp16",) if lo == 2 else ("bf16", "fp16"))]


@pytest.mark.parametrize("case,lo_mode,dtype", GELU)
def test_split_gemm_gelu_split_output_strided(lib, case, lo_mode, dtype):
    """Epilogue 1 reading a split operand (lo_mode) and writing QuickGELU(u) as one, in both output forms, on one ragged, strided case per form:
    u within 4 EPS of float64; hi + decoded(lo) against QuickGELU(u_ref) at test_split_operand_gemm's bounds -- 1e-5 relative for a T remainder
    (bf16: EPS^2 + 1e-5: |lo| <= EPS |v| rounded once more, plus the allowance for the hardware exp / rcp) and EPS 2^-4 for e4m3 (half a step of
    3 mantissa bits on a remainder of at most EPS |v|: 2^-15 in fp16), with clamp_min(1); the windowed launch equals the contiguous one bit for
    bit in out0, out1 and out1_lo; out1 does not depend on the form of out1_lo; the remainder itself is held to check_split_pair."""
    case = on_this_device(gemm_split_gelu_case(case, lo_mode))
    tt = DT[dtype][1]
    ops = split_random_operands(case.M, case.N, case.K, dtype, lo_mode)
    uref = ops["u"]
    gref = uref * torch.sigmoid(1.702 * uref)
    outs = {}
    for mode in (1, 2):
        win = run_split(lib, dtype, capi.EPI_GELU, case, ops, b8_scale=ops["b8_scale"], out1_lo_mode=mode)
        flat = run_split(lib, dtype, capi.EPI_GELU, case, ops, b8_scale=ops["b8_scale"], out1_lo_mode=mode, windows=False)
        for a, b, what in zip(win, flat, ("out0", "out1", "out1_lo")):
            assert torch.equal(a, b), f"{case.name} lo_mode {lo_mode} -> {mode}: {what} of the windowed and the contiguous launch differ"
        u, hi, lo = (t.cpu() for t in win)
        torch.testing.assert_close(u.double(), uref, atol=4 * EPS[dtype], rtol=4 * EPS[dtype])
        dec = lo.double() if mode == 1 else lo.contiguous().view(torch.float8_e4m3fn).float().double() / 4096.0
        tol = (1e-5 if dtype == "fp16" else EPS[dtype] ** 2 + 1e-5) if mode == 1 else EPS[dtype] * 2.0 ** -4
        e = ((hi.double() + dec - gref).abs() / gref.abs().clamp_min(1.0)).max().item()
        print(f"{case.name} {dtype} lo_mode {lo_mode} -> {mode}: hi + lo against QuickGELU(u_ref): max relative err {e:.2e} (bound {tol:.2e})")
        assert e <= tol
        outs[mode] = (hi, lo)
    assert torch.equal(outs[1][0].view(torch.int16), outs[2][0].view(torch.int16)), "out1 must not depend on the form of out1_lo"
    check_split_pair(dtype, outs[1][0], outs[1][1], outs[2][1], gref)


# ---- refusals on the host ---------------------------------------------------------------------------------------------------------------
def test_split_gemm_refusals(lib):
    """Arguments launch_gemm refuses for a split operand: MUDPT_ERR_ARG with the reason, every output untouched."""
    M, N, K = 64, 64, 128
    A = torch.zeros(M, K, device="cuda", dtype=torch.float16)
    Ab = torch.zeros(M, K, device="cuda", dtype=torch.bfloat16)
    lo16 = torch.zeros(M * K + 8, device="cuda", dtype=torch.float16)
    lo8 = torch.zeros(M, 2 * K, device="cuda", dtype=torch.uint8)
    B = torch.zeros(N, K, device="cuda", dtype=torch.float16)
    B8 = torch.zeros(N, 2 * K, device="cuda", dtype=torch.uint8)
    out = torch.full((M, N), SENT, device="cuda", dtype=torch.float32)

    def call(word, dt=1, k=K, a=A, a_lo=lo8, lo_mode=2, b8=B8, scale=127):
        refused(lib, capi.call("mudpt_gemm_split", dtype=dt, epilogue=capi.EPI_STORE_F32, M=M, N=N, K=k, A=a, A_lo=a_lo, lo_mode=lo_mode, lda=K, B=B, B8=b8, b8_scale=scale, ldb=K,
                               out0=out, ldo0=N), word)
        assert bool((out == SENT).all())

    call("fp16 operands only", dt=0, a=Ab)          # lo_mode 2 with bf16
    call("K % 128", k=64)                           # lo_mode 2 at K % 128 != 0 (the operands are K = 128 wide: nothing could be read past them)
    call("needs its low half", a_lo=None)
    call("needs its low half", a_lo=None, lo_mode=1)
    call("16-byte aligned", a_lo=lo16[1:], lo_mode=1)  # 2 bytes off
    call("16-byte aligned", a_lo=lo8.view(-1)[4:])
    call("needs B8", b8=None)
    call("bad E8M0 weight scale 0", scale=0)
    call("bad E8M0 weight scale 255", scale=255)
    call("bad lo_mode 3", lo_mode=3)
    # K = 192 itself, with operands that wide
    A192, lo192, B192, B8192 = (torch.zeros(64, w, device="cuda", dtype=t) for w, t in ((192, torch.float16), (384, torch.uint8), (192, torch.float16), (384, torch.uint8)))
    refused(lib, capi.call("mudpt_gemm_split", dtype=1, epilogue=capi.EPI_STORE_F32, M=M, N=N, K=192, A=A192, A_lo=lo192, lo_mode=2, lda=192, B=B192, B8=B8192, b8_scale=127,
                           ldb=192, out0=out, ldo0=N), "K % 128")
    assert bool((out == SENT).all())
    # at a persistent-kernel shape the e4m3 second pass is built for the forward epilogues only
    M, N = 8003, 1008
    assert lib.mudpt_gemm_form(capi.EPI_GELU_BWD, M, N, K, N, N, N, 2, 0, device_cus()) == capi.GEMM_FORMS.index("PP") | 1 << 8
    A, lo8 = torch.zeros(M, K, device="cuda", dtype=torch.float16), torch.zeros(M, 2 * K, device="cuda", dtype=torch.uint8)
    B, B8 = torch.zeros(N, K, device="cuda", dtype=torch.float16), torch.zeros(N, 2 * K, device="cuda", dtype=torch.uint8)
    aux = torch.zeros(M, N, device="cuda", dtype=torch.float16)
    out = torch.full((M, N), SENT, device="cuda", dtype=torch.float16)
    refused(lib, capi.call("mudpt_gemm_split", dtype=1, epilogue=capi.EPI_GELU_BWD, M=M, N=N, K=K, A=A, A_lo=lo8, lo_mode=2, lda=K, B=B, B8=B8, b8_scale=127, ldb=K, out0=out, ldo0=N,
                           aux=aux, ldaux=N), "not built with the e4m3 second pass")
    assert bool((out == SENT).all())
