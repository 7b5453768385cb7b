"""Every MFMA GEMM kernel form (capi.GEMM_FORMS) at strides, ragged edges and K depths, through the C ABI.

All operands are column-offset WINDOWS of wider buffers with guard rows around them: operand pads and guards hold NaN (a read outside
[rows, K] poisons the result), output pads and guards hold a sentinel that must survive the launch bit for bit.  Small-integer operands
make every fp32 sum exact (|A| <= 3, |B| <= 4: 12 K <= 36 864 < 2^24), so the store, residual and patch epilogues are compared for equality;
the QuickGELU epilogues use random operands against float64 with the tolerances of test_gemm_epilogues, and a windowed launch must equal the
contiguous launch of the same operands bit for bit.  Each case names the form it must take; mudpt_gemm_form confirms it at the device's CU
count (tests/test_capi_cpu.py holds the same cases to it at 256 units without a GPU)."""
import functools

import pytest
import torch

from mudpt_amd import capi
from tests.helpers import (GEMM_FORM_CASES, GEMM_GELU_CASES, GEMM_GUARD_ROWS, GEMM_REFUSAL_CASES, SENT, gemm_form_args, gemm_windows, ok,
                           pp_case_for, refused)

pytestmark = pytest.mark.gpu

DT = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16)}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # half ulp relative
Q8 = 0x20000   # mudpt_gemm's variant bit 17: QuickGELU' in 8 bits
SENT8 = 0xA5   # sentinel of the byte-code output
G = GEMM_GUARD_ROWS
BY_NAME = {c.name: c for c in GEMM_FORM_CASES}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return capi.load()


@functools.lru_cache(maxsize=None)
def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def on_this_device(case):
    """The case itself on 256 compute units; a persistent case rebuilt for its grid regime elsewhere (helpers.pp_case_for)."""
    c = pp_case_for(case, device_cus())
    if c is None:
        pytest.skip(f"no shape reaches the '{case.grid}' regime of the persistent kernel on {device_cus()} compute units")
    return c


def windowed(rows, width, pad_off, dtype, fill, values=None):
    """A [rows + 2 G, width + pad] device buffer of `fill` and its window [G : G + rows, off : off + width], holding `values` if given."""
    pad, off = pad_off
    buf = torch.full((rows + 2 * G, width + pad), fill, dtype=dtype, device="cuda")
    win = buf[G:G + rows, off:off + width]
    if values is not None:
        win.copy_(values.to(dtype))
    return buf, win


def assert_outside_untouched(buf, win_rows, width, pad_off, sentinel, written_rows=None):
    """Every element of an output buffer outside its window (and, patch epilogue, on the window rows the scatter skips) still is the sentinel."""
    chk = buf.clone()
    w = chk[G:G + win_rows, pad_off[1]:pad_off[1] + width]
    if written_rows is None:
        w.fill_(sentinel)
    else:
        w[written_rows.to(w.device)] = sentinel
    bad = (chk != sentinel).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements outside the output window were written, first at buffer (row, column) {bad[0].tolist()} (window from row {G}, column {pad_off[1]})"


def run_windowed(lib, dtype, epi, case, ops, variant=None, windows=True, q8=False):
    """Launch epilogue `epi` of `case` on the operands `ops` (CPU tensors: A [M, K], B [N, K], bias [N] | None, aux [M, N] | None, pos
    [1 + P, N] | None), every operand a guarded window (windows=False: contiguous, still guarded).  Asserts the form the launch takes and that
    nothing outside the output windows changed; returns the output windows (out0, out1) as they are on the device."""
    dt, tt = DT[dtype]
    variant = case.variant if variant is None else variant
    M, N, K = case.M, case.N, case.K
    w = gemm_windows(case, windows)
    f32_out = epi in (capi.EPI_RESIDUAL, capi.EPI_PATCH, capi.EPI_STORE_F32)
    codes_out = q8 and epi == capi.EPI_GELU
    out_rows, written = M, None
    patches = seq_len = 0
    if epi == capi.EPI_PATCH:
        patches, seq_len = case.patch
        assert M % patches == 0
        out_rows = M // patches * seq_len
        written = (torch.arange(out_rows) % seq_len - 1).remainder(seq_len) < patches  # rows 1 .. P of every sequence
    _, A = windowed(M, K, w["A"], tt, float("nan"), ops["A"])
    _, B = windowed(N, K, w["B"], tt, float("nan"), ops["B"])
    sent0 = SENT8 if codes_out else SENT
    buf0, out0 = windowed(out_rows, N, w["out0"], torch.uint8 if codes_out else (torch.float32 if f32_out else tt), sent0)
    buf1, out1 = windowed(M, N, w["out1"], tt, SENT) if epi == capi.EPI_GELU else (None, None)
    aux = None
    if epi in (capi.EPI_RESIDUAL, capi.EPI_GELU_BWD):
        aux_t = torch.float32 if epi == capi.EPI_RESIDUAL else (torch.uint8 if q8 else tt)
        _, aux = windowed(M, N, w["aux"], aux_t, 0 if aux_t == torch.uint8 else float("nan"), ops["aux"])
    bias = ops["bias"].cuda() if ops.get("bias") is not None and epi != capi.EPI_PATCH else None
    pos = ops["pos"].cuda() if epi == capi.EPI_PATCH else None
    ldo1 = out1.stride(0) if out1 is not None else N + w["out1"][0]
    ldaux = aux.stride(0) if aux is not None else N + w["aux"][0]
    assert (out0.stride(0), ldo1, ldaux) == gemm_form_args(case, epi, 0, windows)[4:7]
    got = lib.mudpt_gemm_form(epi, M, N, K, out0.stride(0), ldo1, ldaux, 0, variant, device_cus())
    want = capi.GEMM_FORMS.index(case.form) | case.slices << 8
    assert got == want, f"{case.name} epilogue {epi}: form {capi.GEMM_FORMS[got & 0xff] if got >= 0 else got} x {got >> 8}, the case is there for {case.form} x {case.slices}"
    ok(lib, capi.call("mudpt_gemm", dtype=dt, epilogue=epi, M=M, N=N, K=K, A=A, lda=A.stride(0), B=B, ldb=B.stride(0), bias=bias, out0=out0, ldo0=out0.stride(0), out1=out1,
                      ldo1=out1.stride(0) if out1 is not None else 0, aux=aux, ldaux=aux.stride(0) if aux is not None else 0, patches=patches, seq_len=seq_len, pos=pos,
                      variant=variant | (Q8 if q8 else 0)))
    assert_outside_untouched(buf0, out_rows, N, w["out0"], sent0, written)
    if buf1 is not None:
        assert_outside_untouched(buf1, M, N, w["out1"], SENT)
    return out0, out1


@functools.lru_cache(maxsize=1)  # the two dtypes of a case run back to back (dtype is the fastest-varying parameter) and share it
def exact_operands(M, N, K, patches):
    """Small-integer operands and their exact fp32 product: A in [-3, 3], the asymmetric B of test_gemm_exact_integers, integer bias / aux / pos."""
    g = torch.Generator().manual_seed(M + N + K)
    ops = {"A": torch.randint(-3, 4, (M, K), generator=g).float(),
           "B": (torch.arange(N).view(N, 1) % 5 - 2 + (torch.arange(K).view(1, K) % 3)).float(),
           "bias": torch.randint(-4, 5, (N,), generator=g).float(),
           "aux": torch.randint(-8, 9, (M, N), generator=g).float(),
           "pos": torch.randint(-4, 5, (1 + patches, N), generator=g).float() if patches else None}
    ops["acc"] = ops["A"] @ ops["B"].t()
    assert ops["acc"].abs().max().item() <= 12 * K < 2 ** 24
    return ops


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", GEMM_FORM_CASES, ids=lambda c: c.name)
def test_gemm_form_exact_strided_guarded(lib, dtype, case):
    """Bit-exact results of every form on windowed operands with ragged M and N, nothing written outside the output window."""
    case = on_this_device(case)
    tt = DT[dtype][1]
    ops = exact_operands(case.M, case.N, case.K, case.patch[0] if case.patch else 0)
    for epi in case.epis:
        out0, _ = run_windowed(lib, dtype, epi, case, ops)
        got = out0.cpu()
        if epi == capi.EPI_PATCH:
            Pn, L = case.patch
            ref = (ops["acc"].view(-1, Pn, case.N) + ops["pos"][1:]).reshape(-1, case.N)  # no bias: the patch embedding has none
            got = got.view(-1, L, case.N)[:, 1:1 + Pn].reshape(-1, case.N)
        elif epi == capi.EPI_RESIDUAL:
            ref = ops["aux"] + ops["acc"] + ops["bias"]
        else:
            ref = ops["acc"] + ops["bias"]
            if epi == capi.EPI_STORE:
                ref = ref.to(tt)
        bad = (got != ref).nonzero()
        assert bad.numel() == 0, f"{case.name} epilogue {epi}: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}: {got[tuple(bad[0])].item()} != {ref[tuple(bad[0])].item()}"


@functools.lru_cache(maxsize=1)
def random_operands(M, N, K, dtype):
    tt = DT[dtype][1]
    g = torch.Generator().manual_seed(M + N + K)
    ops = {"A": torch.randn(M, K, generator=g).to(tt), "B": (torch.randn(N, K, generator=g) * K ** -0.5).to(tt), "bias": torch.randn(N, generator=g),
           "u": torch.randn(M, N, generator=g).to(tt), "codes": torch.randint(0, 255, (M, N), generator=g, dtype=torch.uint8)}
    ops["acc"] = ops["A"].double() @ ops["B"].double().t()
    return ops


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GEMM_GELU_CASES)
def test_gemm_form_gelu_epilogues_strided(lib, dtype, name):
    """The QuickGELU epilogues (forward, backward, and both with QuickGELU' in 8 bits) of every form that builds them, on one ragged, strided
    case each: float64 parity at test_gemm_epilogues' tolerances, and the windowed launch equals the contiguous one bit for bit."""
    case = on_this_device(BY_NAME[name])
    ops = random_operands(case.M, case.N, case.K, dtype)
    tol = dict(atol=4 * EPS[dtype], rtol=4 * EPS[dtype])
    acc, uref = ops["acc"], ops["acc"] + ops["bias"].double()
    sr = torch.sigmoid(1.702 * uref)

    def both(epi, aux=None, q8=False):
        o = dict(ops, aux=aux)
        if epi == capi.EPI_GELU_BWD:
            o["bias"] = None
        win = run_windowed(lib, dtype, epi, case, o, q8=q8)
        flat = run_windowed(lib, dtype, epi, case, o, q8=q8, windows=False)
        for a, b in zip(win, flat):
            assert (a is None and b is None) or torch.equal(a, b), f"{case.name} epilogue {epi}: windowed and contiguous launches differ"
        return [None if t is None else t.cpu().double() for t in win]

    u, gl = both(capi.EPI_GELU)
    torch.testing.assert_close(u, uref, **tol)
    torch.testing.assert_close(gl, uref * sr, **tol)
    du, _ = both(capi.EPI_GELU_BWD, aux=ops["u"])
    ud = ops["u"].double()
    s = torch.sigmoid(1.702 * ud)
    torch.testing.assert_close(du, acc * (s * (1 + 1.702 * ud * (1 - s))), **tol)
    # QuickGELU' in 8 bits: the forward writes byte codes rint((g' + 0.1) * 212) (row stride in BYTES), the backward multiplies by the decoded value
    codes, gl8 = both(capi.EPI_GELU, q8=True)
    assert torch.equal(gl8, gl)
    gp = sr * (1 + 1.702 * uref * (1 - sr))
    want = torch.round((gp + 0.1) * 212.0)
    assert (codes - want).abs().max().item() <= 1 and ((codes - want).abs() > 0).double().mean().item() < 0.02  # ties / 1-ulp exp
    assert ((codes / 212.0 - 0.1) - gp).abs().max().item() <= 0.5 / 212 + 1e-3
    du8, _ = both(capi.EPI_GELU_BWD, aux=ops["codes"], q8=True)
    torch.testing.assert_close(du8, acc * (ops["codes"].double() / 212.0 - 0.1), **tol)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_output_stride_the_persistent_kernel_cannot_take(lib, dtype):
    """ldo0 % 8 != 0 at a shape the persistent kernel would take: the launch falls to a simple tile (the form table pins which) and is still
    exact and in bounds.  lda / ldb that are no multiple of 8 are refused on the host, the output untouched."""
    case, = GEMM_REFUSAL_CASES
    tt = DT[dtype][1]
    ops = exact_operands(case.M, case.N, case.K, 0)
    for epi in case.epis:
        out0, _ = run_windowed(lib, dtype, epi, case, ops)
        ref = ops["acc"] + ops["bias"]
        assert torch.equal(out0.cpu(), ref.to(tt) if epi == capi.EPI_STORE else ref)
    M, N, K = case.M, case.N, case.K
    out = torch.full((M, N), SENT, device="cuda")
    for pads in ((4, 0), (0, 4)):  # lda = K + 4, then ldb = K + 4
        A = torch.zeros(M, K + pads[0], device="cuda", dtype=tt)
        B = torch.zeros(N, K + pads[1], device="cuda", dtype=tt)
        refused(lib, capi.call("mudpt_gemm", dtype=DT[dtype][0], epilogue=capi.EPI_STORE_F32, M=M, N=N, K=K, A=A, lda=A.stride(0), B=B, ldb=B.stride(0), out0=out, ldo0=N),
                "bad lda/ldb")
        assert bool((out == SENT).all())
