"""GPU parity of the single HIP kernels against the CPU oracle, called through the C ABI (ctypes)."""
import ctypes as C

import pytest
import torch

from mudpt_amd import capi
from oracle import mudpt_oracle as O
from tests.helpers import (ATTN_CASES, ATTN_LONG_FWD_CASES, ATTN_LONG_FWD_FLAGS, ATTN_SEL_CASES, ATTN_SEL_COMPARE, ATTN_WINDOW_CASES,
                           ATTN_WINDOW_FULL_FLAG, SENT, P, attn64, attn_bwd_form_flags, attn_window_flags, check_split_pair, ok, refused)

pytestmark = pytest.mark.gpu

DT = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16)}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # half ulp relative


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return capi.load()


def gemm(lib, dt, epi, A, B, bias=None, out0=None, out1=None, aux=None, patches=0, seq_len=0, pos=None, variant=0):
    M, K = A.shape
    N = B.shape[0]
    ok(lib, capi.call("mudpt_gemm", dtype=dt, epilogue=epi, M=M, N=N, K=K, A=A, lda=A.stride(0), B=B, ldb=B.stride(0), bias=bias, out0=out0, ldo0=out0.stride(0),
                      out1=out1, ldo1=out1.stride(0) if out1 is not None else 0, aux=aux, ldaux=aux.stride(0) if aux is not None else 0,
                      patches=patches, seq_len=seq_len, pos=pos, variant=variant))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_exact_integers(lib, dtype):
    """Small-integer operands: every product and sum is exact in fp32, so the result must be bit-exact.
    A is a shifted identity-like pattern and B is asymmetric, which catches swapped row/col maps."""
    dt, tt = DT[dtype]
    M, N, K = 200, 144, 128
    g = torch.Generator().manual_seed(0)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    B = (torch.arange(N).view(N, 1) % 5 - 2 + (torch.arange(K).view(1, K) % 3)).float()  # asymmetric
    ref = A @ B.t()
    out = torch.empty(M, N, device="cuda", dtype=torch.float32)
    gemm(lib, dt, 5, A.cuda().to(tt), B.cuda().to(tt), out0=out)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_exact_integers_full_size(lib, dtype):
    """BASELINE config 2's row count (M = 256 x 201): 603 tiles = two full waves + 91 tiles run as 182 half tiles.
    Small-integer operands make every fp32 sum exact, so full and half tiles must be bit-exact."""
    dt, tt = DT[dtype]
    M, N, K = 51456, 768, 256
    g = torch.Generator().manual_seed(1)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    B = (torch.arange(N).view(N, 1) % 7 - 3 + (torch.arange(K).view(1, K) % 4)).float()
    ref = A @ B.t()
    out = torch.empty(M, N, device="cuda", dtype=torch.float32)
    gemm(lib, dt, 5, A.cuda().to(tt), B.cuda().to(tt), out0=out)
    assert torch.equal(out.cpu(), ref)
    outT = torch.empty(M, N, device="cuda", dtype=tt)  # |values| <= 3 * 6 * 256 is exact in bf16? no: compare after the same rounding
    gemm(lib, dt, 0, A.cuda().to(tt), B.cuda().to(tt), out0=outT)
    assert torch.equal(outT.cpu(), ref.to(tt))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(804, 2304, 768), (847, 512, 2048), (77, 128, 64), (4096, 768, 3072), (33000, 768, 768),
                                   (22100, 768, 768), (51400, 768, 192), (99, 512, 192), (99, 2048, 512)])
def test_gemm_epilogues(lib, dtype, shape):
    """All fused epilogues against a float64 product.  The last two shapes leave a partial last wave of 256 x 256 tiles on 256
    CUs (261 = 256 + 5 and 603 = 2 * 256 + 91 tiles), which the persistent kernel runs as half tiles; both have a ragged
    last row panel (22100: the lower half tile is entirely out of range).  The 99-row shapes are the trimmed text tower's: small grids,
    which run the 64 x 64 kernel (t64 = 16 tiles; K = 512 in 128-deep K-tiles).  The 4-deep operand ring those shapes once ran is reachable
    through gemm_variant 6 only: tests/test_gemm_forms_gpu.py runs it."""
    dt, tt = DT[dtype]
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(tt)
    B = (torch.randn(N, K, generator=g) * K ** -0.5).to(tt)
    bias = torch.randn(N, generator=g)
    acc = A.double() @ B.double().t()
    Ad, Bd, bd = A.cuda(), B.cuda(), bias.cuda()
    tol = dict(atol=4 * EPS[dtype], rtol=4 * EPS[dtype])
    # 0: store T with bias
    out = torch.empty(M, N, device="cuda", dtype=tt)
    gemm(lib, dt, 0, Ad, Bd, bias=bd, out0=out)
    torch.testing.assert_close(out.cpu().double(), acc + bias.double(), **tol)
    # 5: fp32 store, no bias
    o32 = torch.empty(M, N, device="cuda", dtype=torch.float32)
    gemm(lib, dt, 5, Ad, Bd, out0=o32)
    torch.testing.assert_close(o32.cpu().double(), acc, atol=2e-5 * K ** 0.5, rtol=1e-5)
    # 1: bias + QuickGELU, both outputs
    u, gl = torch.empty(M, N, device="cuda", dtype=tt), torch.empty(M, N, device="cuda", dtype=tt)
    gemm(lib, dt, 1, Ad, Bd, bias=bd, out0=u, out1=gl)
    uref = acc + bias.double()
    torch.testing.assert_close(u.cpu().double(), uref, **tol)
    torch.testing.assert_close(gl.cpu().double(), uref * torch.sigmoid(1.702 * uref), **tol)
    # 2: residual fp32
    res = torch.randn(M, N, generator=g)
    gemm(lib, dt, 2, Ad, Bd, bias=bd, out0=o32, aux=res.cuda())
    torch.testing.assert_close(o32.cpu().double(), res.double() + uref, atol=2e-5 * K ** 0.5, rtol=1e-5)
    # 3: QuickGELU backward
    upre = torch.randn(M, N, generator=g).to(tt)
    gemm(lib, dt, 3, Ad, Bd, out0=out, aux=upre.cuda())
    ud = upre.double()
    s = torch.sigmoid(1.702 * ud)
    torch.testing.assert_close(out.cpu().double(), acc * (s * (1 + 1.702 * ud * (1 - s))), **tol)
    # 1 / 3 with QuickGELU' in 8 bits (variant bit 17; what the bf16 mode keeps for the backward instead of u): the forward writes byte codes
    # rint((g' + 0.1) * 212), the backward multiplies by the decoded value -- absolute error <= 0.5 / 212 on a factor in [-0.1, 1.1]
    Q8 = 0x20000
    codes = torch.zeros(M, N, device="cuda", dtype=torch.uint8)
    gl2 = torch.empty(M, N, device="cuda", dtype=tt)
    gemm(lib, dt, 1, Ad, Bd, bias=bd, out0=codes, out1=gl2, variant=Q8)
    assert torch.equal(gl2, gl)
    sr = torch.sigmoid(1.702 * uref)
    gp = sr * (1 + 1.702 * uref * (1 - sr))
    want = torch.round((gp + 0.1) * 212.0)
    assert (codes.cpu().double() - want).abs().max().item() <= 1 and ((codes.cpu().double() - want).abs() > 0).double().mean().item() < 0.02  # ties / 1-ulp exp
    assert ((codes.cpu().double() / 212.0 - 0.1) - gp).abs().max().item() <= 0.5 / 212 + 1e-3
    out8 = torch.empty(M, N, device="cuda", dtype=tt)
    cq = torch.randint(0, 255, (M, N), generator=g, dtype=torch.uint8)
    gemm(lib, dt, 3, Ad, Bd, out0=out8, aux=cq.cuda(), variant=Q8)
    torch.testing.assert_close(out8.cpu().double(), acc * (cq.double() / 212.0 - 0.1), **tol)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_rows_do_not_depend_on_the_kernel_that_ran_them(lib, dtype):
    """A row of a GEMM must come out bit-identical whichever kernel ran the shape -- the small-tile kernel (64 x 64 or 128 x 128 tiles) or the
    persistent one: every kernel contracts k in the same order, and (round 4) every T conversion of an epilogue rounds the fp32 VALUE
    (common.h round_to: with -ffp-contract=fast the compiler folded the QuickGELU multiply into the conversion in one kernel and not in the
    other, one ulp apart).  That is what makes a trimmed / bucketed text tower equal the untrimmed one (tests/test_manyclass_gpu.py).
    The text tower's shapes at 208 class prompts: 5 408 rows (trimmed) against 16 016 (untrimmed); and 450 rows, a grid small enough for the
    128-deep K-tiles of round 4 (two workgroups per CU: gemm.hip deep_k_tiles)."""
    dt, tt = DT[dtype]
    M2, M1, M0 = 450, 5408, 16016
    g = torch.Generator().manual_seed(11)
    for name, N, K, epi in (("qkv", 1536, 512, 0), ("out", 512, 512, 5), ("fc", 2048, 512, 1), ("proj", 512, 2048, 5), ("dgelu", 2048, 512, 3), ("dfc", 512, 2048, 0)):
        A = torch.randn(M0, K, generator=g).to(tt).cuda()
        B = (torch.randn(N, K, generator=g) * K ** -0.5).to(tt).cuda()
        bias = torch.randn(N, generator=g).cuda()
        auxf = torch.randn(M0, N, generator=g).to(tt).cuda()
        res = {}
        for M in (M2, M1, M0):
            out0 = torch.zeros(M, N, device="cuda", dtype=torch.float32 if epi == 5 else tt)
            out1 = torch.zeros(M, N, device="cuda", dtype=tt) if epi == 1 else None
            gemm(lib, dt, epi, A[:M], B, bias=bd_or_none(bias, epi), out0=out0, out1=out1, aux=auxf[:M] if epi == 3 else None)
            res[M] = (out0[:M1].clone(), out1[:M1].clone() if out1 is not None else None)
        assert torch.equal(res[M1][0], res[M0][0]), name
        assert torch.equal(res[M2][0], res[M0][0][:M2]), name
        if epi == 1:
            assert torch.equal(res[M1][1], res[M0][1]), name
            assert torch.equal(res[M2][1], res[M0][1][:M2]), name


def bd_or_none(bias, epi):
    return None if epi == 3 else bias


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(804, 768, 3072), (804, 768, 2304), (450, 512, 2048), (201, 768, 3072), (1000, 768, 1536)])
def test_gemm_split_k(lib, dtype, shape):
    """Small grids with a long contraction (the reference's training batch of 4: M = 804) split K over up to 4 slices whose fp32 partials are
    summed in slice order.  Small-integer operands make every sum exact, so the split result is BIT-exact (both store epilogues, bias
    included); random operands agree with the unsplit kernel to fp32 rounding; run to run bit for bit."""
    dt, tt = DT[dtype]
    M, N, K = shape
    g = torch.Generator().manual_seed(M + K)
    A = torch.randint(-2, 3, (M, K), generator=g).float()
    B = (torch.arange(N).view(N, 1) % 5 - 2 + (torch.arange(K).view(1, K) % 3)).float()
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    ref = A @ B.t() + bias
    Ad, Bd, bd = A.cuda().to(tt), B.cuda().to(tt), bias.cuda()
    o32 = torch.empty(M, N, device="cuda")
    gemm(lib, dt, 5, Ad, Bd, bias=bd, out0=o32, variant=0x10000)
    assert torch.equal(o32.cpu(), ref)
    oT = torch.empty(M, N, device="cuda", dtype=tt)
    gemm(lib, dt, 0, Ad, Bd, bias=bd, out0=oT, variant=0x10000)
    assert torch.equal(oT.cpu(), ref.to(tt))
    Ar, Br = torch.randn(M, K, generator=g).to(tt).cuda(), (torch.randn(N, K, generator=g) * K ** -0.5).to(tt).cuda()
    a32, b32, c32 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    gemm(lib, dt, 5, Ar, Br, out0=a32)
    gemm(lib, dt, 5, Ar, Br, out0=b32, variant=0x10000)
    gemm(lib, dt, 5, Ar, Br, out0=c32, variant=0x10000)
    torch.cuda.synchronize()
    torch.testing.assert_close(b32, a32, atol=2e-5 * K ** 0.5, rtol=1e-5)
    assert torch.equal(b32, c32)
    assert not torch.equal(b32, a32) or K < 1536  # the split path really ran (a different summation order shows in the last bits)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_patch_epilogue(lib, dtype):
    """Patch-embed GEMM: row m of the im2col matrix lands on token row (m / P) * L + 1 + m % P, plus pos-emb."""
    dt, tt = DT[dtype]
    Bn, Pn, L, N, K = 3, 4, 7, 192, 768
    g = torch.Generator().manual_seed(5)
    A = torch.randn(Bn * Pn, K, generator=g).to(tt)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(tt)
    pos = torch.randn(1 + Pn, N, generator=g)
    out = torch.full((Bn * L, N), 7.0, device="cuda")
    gemm(lib, dt, 4, A.cuda(), W.cuda(), out0=out, patches=Pn, seq_len=L, pos=pos.cuda())
    ref = torch.full((Bn, L, N), 7.0, dtype=torch.float64)
    ref[:, 1:1 + Pn] = (A.double() @ W.double().t()).view(Bn, Pn, N) + pos[1:].double()
    torch.testing.assert_close(out.cpu().double().view(Bn, L, N), ref, atol=1e-4, rtol=1e-5)


def test_gemm_rejects_bad_shapes(lib):
    A = torch.zeros(64, 96, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
    rc = capi.call("mudpt_gemm", dtype=0, epilogue=0, M=64, N=64, K=96, A=A, lda=96, B=A, ldb=96, out0=out, ldo0=64)
    assert rc == 1 and b"multiple of 64" in lib.mudpt_last_error()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("rows,d", [(804, 768), (847, 512), (21, 192), (5, 128), (4, 1024)])
def test_layernorm_fwd_bwd(lib, dtype, rows, d):
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    xr = x.clone().requires_grad_(True)
    y = O.layer_norm(xr, gamma, beta)
    out = torch.empty(rows, d, device="cuda", dtype=tt)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    xc, gc, bc = x.cuda(), gamma.cuda(), beta.cuda()  # keep device tensors alive across the async launches
    ok(lib, capi.call("mudpt_layernorm_fwd", dtype=dt, x=xc, ldx=d, gamma=gc, beta=bc, out=out, ldo=d, out_f32=0, mean=mean, rstd=rstd, rows=rows, d=d))
    torch.testing.assert_close(out.cpu().float(), y.detach(), atol=4 * EPS[dtype], rtol=4 * EPS[dtype])
    o32 = torch.empty(rows, d, device="cuda")
    ok(lib, capi.call("mudpt_layernorm_fwd", dtype=dt, x=xc, ldx=d, gamma=gc, beta=bc, out=o32, ldo=d, out_f32=1, rows=rows, d=d))
    torch.testing.assert_close(o32.cpu(), y.detach(), atol=2e-5, rtol=1e-5)
    # backward: dx = dres + LN'(dy), dy in T
    dy = torch.randn(rows, d, generator=g).to(tt)
    dres = torch.randn(rows, d, generator=g)
    (dx_ref,) = torch.autograd.grad(y, xr, dy.float())
    dx = torch.empty(rows, d, device="cuda")
    dx_lp = torch.empty(rows, d, device="cuda", dtype=tt)
    dyc, drc = dy.cuda(), dres.cuda()
    ok(lib, capi.call("mudpt_layernorm_bwd", dtype=dt, dy=dyc, lddy=d, dy_f32=0, x=xc, ldx=d, mean=mean, rstd=rstd, gamma=gc, dres=drc, lddres=d, dx=dx, lddx=d,
                      dx_lp=dx_lp, lddx_lp=d, rows=rows, d=d))
    torch.testing.assert_close(dx.cpu(), dx_ref + dres, atol=2e-5, rtol=2e-5)
    torch.testing.assert_close(dx_lp.cpu().float(), dx_ref + dres, atol=4 * EPS[dtype] * 4, rtol=4 * EPS[dtype])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("add_kind", ["f32", "lp", "none"])
def test_layernorm_fused_add_and_prompt_splice(lib, dtype, add_kind):
    """What block_fwd fuses into LayerNorm (clip/model.py:281-301): v = x + add (fp32 addend, or the T-precision update stream),
    rows 1..n of every L-row sequence REPLACED by the deep-prompt rows (no add on those), v written back as the block input
    (bit-exact: one fp32 add), then normalised."""
    dt, tt = DT[dtype]
    nseq, L, d, row0, n = 5, 13, 512, 9, 4   # vision-style: the last n rows of every sequence
    rows = nseq * L
    g = torch.Generator().manual_seed(17)
    x = torch.randn(rows, d, generator=g) * 1.5 + 0.3
    add = torch.randn(rows, d, generator=g) * 0.5
    add_t = add.to(tt)
    ov = torch.randn(n, d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    v = x + (add if add_kind == "f32" else add_t.float() if add_kind == "lp" else 0)
    v = v.view(nseq, L, d).clone()
    v[:, row0:row0 + n] = ov
    v = v.view(rows, d)
    y = O.layer_norm(v, gamma, beta)
    xc, gc, bc, oc = x.cuda(), gamma.cuda(), beta.cuda(), ov.cuda()
    a32 = add.cuda() if add_kind == "f32" else None
    alp = add_t.cuda() if add_kind == "lp" else None
    xout = torch.full((rows, d), float("nan"), device="cuda")
    out = torch.empty(rows, d, device="cuda", dtype=tt)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ok(lib, capi.call("mudpt_layernorm_fwd_fused", dtype=dt, x=xc, ldx=d, add=a32, add_lp=alp, ldadd=d, ov_rows=oc, ov_row0=row0, ov_n=n, ov_L=L, xout=xout, ldxout=d,
                      gamma=gc, beta=bc, out=out, ldo=d, out_f32=0, mean=mean, rstd=rstd, rows=rows, d=d))
    assert torch.equal(xout.cpu(), v)                      # the saved block input: exact
    torch.testing.assert_close(out.cpu().float(), y, atol=4 * EPS[dtype], rtol=4 * EPS[dtype])
    torch.testing.assert_close(mean.cpu(), v.mean(-1), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(rstd.cpu(), (v.var(-1, unbiased=False) + 1e-5).rsqrt(), atol=1e-5, rtol=2e-5)
    # fp32 output and no splice: every row is x + add
    o32 = torch.empty(rows, d, device="cuda")
    ok(lib, capi.call("mudpt_layernorm_fwd_fused", dtype=dt, x=xc, ldx=d, add=a32, add_lp=alp, ldadd=d, ov_L=1, gamma=gc, beta=bc, out=o32, ldo=d, out_f32=1, rows=rows, d=d))
    v2 = x + (add if add_kind == "f32" else add_t.float() if add_kind == "lp" else 0)
    torch.testing.assert_close(o32.cpu(), O.layer_norm(v2, gamma, beta), atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("B,C,e", [(4, 11, 512), (256, 1000, 512), (5, 3, 128), (3, 1, 64)])
def test_head_matches_torch_cross_entropy(lib, B, C, e):
    """Cosine logits + mean cross-entropy, forward and backward (trainers/mudpt.py:178-182,250) against torch autograd in float64,
    at the benchmark's C = 11 and at BASELINE configs[2]'s C = 1000 (CE over 1000 columns)."""
    g = torch.Generator().manual_seed(B * 1000 + C)
    img, txt = torch.randn(B, e, generator=g) * 3, torch.randn(C, e, generator=g) * 0.2
    labels = torch.randint(0, C, (B,), generator=g)
    scale, gscale = 14.2857, 0.5
    i64, t64 = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    ref_logits = scale * torch.nn.functional.normalize(i64, dim=-1) @ torch.nn.functional.normalize(t64, dim=-1).t()
    ref_loss = torch.nn.functional.cross_entropy(ref_logits, labels)
    (gscale * ref_loss).backward()
    ic, tc, lc = img.cuda(), txt.cuda(), labels.cuda()
    logits, loss = torch.empty(B, C, device="cuda"), torch.empty(1, device="cuda")
    dimg, dtxt = torch.empty(B, e, device="cuda"), torch.empty(C, e, device="cuda")
    ok(lib, lib.mudpt_head(P(ic), P(tc), P(lc), scale, gscale, B, C, e, P(logits), P(loss), P(dimg), P(dtxt), None))
    torch.testing.assert_close(logits.cpu().double(), ref_logits.detach(), atol=2e-5, rtol=1e-5)
    assert abs(loss.item() - ref_loss.item()) <= 2e-6 * max(1.0, abs(ref_loss.item()))
    for got, ref in ((dimg, i64.grad), (dtxt, t64.grad)):
        rms = ref.pow(2).mean().sqrt().item()
        assert (got.cpu().double() - ref).abs().max().item() <= 2e-5 * rms + 1e-12
    # forward only (model_inference): no labels
    logits2 = torch.empty(B, C, device="cuda")
    ok(lib, lib.mudpt_head(P(ic), P(tc), None, scale, 1.0, B, C, e, P(logits2), None, None, None, None))
    assert torch.equal(logits2, logits)


def test_head_label_out_of_range_gives_nan_loss_not_a_fault(lib):
    B, C, e = 4, 7, 64
    img, txt = torch.randn(B, e).cuda(), torch.randn(C, e).cuda()
    labels = torch.tensor([0, 7, 3, -1]).cuda()  # 7 and -1 are outside [0, C)
    logits, loss = torch.empty(B, C, device="cuda"), torch.empty(1, device="cuda")
    dimg, dtxt = torch.empty(B, e, device="cuda"), torch.empty(C, e, device="cuda")
    ok(lib, lib.mudpt_head(P(img), P(txt), P(labels), 10.0, 1.0, B, C, e, P(logits), P(loss), P(dimg), P(dtxt), None))
    assert torch.isnan(loss).all() and torch.isfinite(logits).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,d,row0,n", [(256, 201, 768, 197, 4), (1000, 20, 512, 1, 4), (3, 7, 64, 2, 1), (33, 5, 128, 0, 2)])
def test_reduce_rows(lib, dtype, B, L, d, row0, n):
    """Backward of the prompt splice: sum over the batch of the n prompt rows.  Against a float64 sum, bit for bit run to run,
    from the fp32 stream and from its T copy, with accumulate and with clearing of the summed rows."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(B + d)
    src = torch.randn(B, L, d, generator=g)
    ref = src[:, row0:row0 + n].double().sum(0)
    sc = src.cuda()
    out = torch.empty(n, d, device="cuda")
    ok(lib, lib.mudpt_reduce_rows(dt, P(sc), None, B, L, d, row0, n, P(out), 0, 0, 0.25, None))
    torch.cuda.synchronize()
    tol = 4e-6 * B ** 0.5  # fp32 summation of B unit-variance values: a few ulp of sqrt(B)
    assert (out.cpu().double() - 0.25 * ref).abs().max().item() <= tol
    again = torch.empty(n, d, device="cuda")
    for _ in range(3):
        ok(lib, lib.mudpt_reduce_rows(dt, P(sc), None, B, L, d, row0, n, P(again), 0, 0, 0.25, None))
        torch.cuda.synchronize()
        assert torch.equal(again, out)   # fixed-order tree: bitwise reproducible
    # accumulate: out += sum
    ok(lib, lib.mudpt_reduce_rows(dt, P(sc), None, B, L, d, row0, n, P(again), 0, 1, 0.25, None))
    torch.cuda.synchronize()
    torch.testing.assert_close(again, 2 * out, atol=1e-6, rtol=1e-6)
    # T-precision source (the bf16 gradient stream), cleared afterwards together with the fp32 copy
    lp = src.to(tt).cuda()
    ref_lp = lp.cpu().float()[:, row0:row0 + n].double().sum(0)
    out2 = torch.empty(n, d, device="cuda")
    ok(lib, lib.mudpt_reduce_rows(dt, None, P(lp), B, L, d, row0, n, P(out2), 1, 0, 1.0, None))
    torch.cuda.synchronize()
    assert (out2.cpu().double() - ref_lp).abs().max().item() <= tol
    assert torch.count_nonzero(lp[:, row0:row0 + n]) == 0
    keep = torch.ones(L, dtype=torch.bool); keep[row0:row0 + n] = False
    assert torch.equal(lp[:, keep.cuda()].cpu(), src.to(tt)[:, keep])  # other rows untouched


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,C,L,d,n", [(64, 11, 9, 512, 4), (3, 100, 20, 512, 4), (2, 5, 7, 128, 2)])
def test_cocoop_dbias(lib, dtype, B, C, L, d, n):
    """Gradient of meta_net's per-image context shift (trainers/cocoop.py:141-146): the sum over an image's C prompts and n context rows
    of the text-input gradient; from the fp32 stream and from its T copy, against a float64 sum, bit for bit run to run."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(B * C + L)
    dx = torch.randn(B * C, L, d, generator=g)
    ref = dx.view(B, C, L, d)[:, :, 1:1 + n].double().sum((1, 2))
    dxc, out = dx.cuda(), torch.empty(B, d, device="cuda")
    ok(lib, lib.mudpt_cocoop_dbias(dt, P(dxc), None, P(out), B, C, L, d, n, 0.5, None))
    torch.cuda.synchronize()
    tol = 4e-6 * (C * n) ** 0.5
    assert (out.cpu().double() - 0.5 * ref).abs().max().item() <= tol
    lp = dx.to(tt).cuda()
    ref_lp = lp.cpu().float().view(B, C, L, d)[:, :, 1:1 + n].double().sum((1, 2))
    out2, out3 = torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda")
    ok(lib, lib.mudpt_cocoop_dbias(dt, None, P(lp), P(out2), B, C, L, d, n, 1.0, None))
    ok(lib, lib.mudpt_cocoop_dbias(dt, None, P(lp), P(out3), B, C, L, d, n, 1.0, None))
    torch.cuda.synchronize()
    assert (out2.cpu().double() - ref_lp).abs().max().item() <= 2 * tol and torch.equal(out2, out3)


@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(4, 768, 512), (44, 512, 768), (17, 33, 70), (256, 11, 512)])
def test_sgemm_all_transpose_forms(lib, tA, tB, M, N, K):
    """fp32 C = alpha op(A) op(B) + bias + beta C: the prompt projections (trainers/mudpt.py:127-128, clip/model.py:539), their
    weight / input gradients and the logit contraction; every transpose form, ragged shapes."""
    g = torch.Generator().manual_seed(M * N + K + 2 * tA + tB)
    A = torch.randn((K, M) if tA else (M, K), generator=g)
    B = torch.randn((N, K) if tB else (K, N), generator=g)
    bias, C0 = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    opA, opB = (A.t() if tA else A).double(), (B.t() if tB else B).double()
    ref = 0.7 * (opA @ opB) + bias.double() + 0.3 * C0.double()
    Ac, Bc, bc, Cc = A.cuda(), B.cuda(), bias.cuda(), C0.clone().cuda()
    ok(lib, lib.mudpt_sgemm(tA, tB, M, N, K, 0.7, P(Ac), A.stride(0), P(Bc), B.stride(0), 0.3, P(Cc), N, P(bc), None))
    torch.cuda.synchronize()
    torch.testing.assert_close(Cc.cpu().double(), ref, atol=3e-5 * K ** 0.5, rtol=1e-5)
    Cd = torch.full((M, N), float("nan"), device="cuda")   # beta = 0 must not read C
    ok(lib, lib.mudpt_sgemm(tA, tB, M, N, K, 1.0, P(Ac), A.stride(0), P(Bc), B.stride(0), 0.0, P(Cd), N, None, None))
    torch.cuda.synchronize()
    torch.testing.assert_close(Cd.cpu().double(), opA @ opB, atol=3e-5 * K ** 0.5, rtol=1e-5)


def test_layernorm_gather_scatter(lib):
    """row_index: LN of selected token rows (ln_post on CLS rows, ln_final on EOT rows) and the scatter of its gradient."""
    rows, d, total = 6, 256, 40
    g = torch.Generator().manual_seed(3)
    x = torch.randn(total, d, generator=g)
    idx = torch.tensor([0, 7, 14, 21, 28, 39], dtype=torch.int32)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    xr = x[idx.long()].clone().requires_grad_(True)
    y = O.layer_norm(xr, gamma, beta)
    out, mean, rstd = torch.empty(rows, d, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    xc, ic, gc, bc = x.cuda(), idx.cuda(), gamma.cuda(), beta.cuda()
    ok(lib, capi.call("mudpt_layernorm_fwd", dtype=0, x=xc, ldx=d, row_index=ic, gamma=gc, beta=bc, out=out, ldo=d, out_f32=1, mean=mean, rstd=rstd, rows=rows, d=d))
    dy = torch.randn(rows, d, generator=g)
    (dref,) = torch.autograd.grad(y, xr, dy)
    dx = torch.zeros(total, d, device="cuda")
    dyc = dy.cuda()
    ok(lib, capi.call("mudpt_layernorm_bwd", dtype=0, dy=dyc, lddy=d, dy_f32=1, x=xc, ldx=d, row_index=ic, mean=mean, rstd=rstd, gamma=gc, dx=dx, lddx=d, rows=rows, d=d))
    torch.testing.assert_close(out.cpu(), y.detach(), atol=2e-5, rtol=1e-5)
    full = torch.zeros(total, d)
    full[idx.long()] = dref
    torch.testing.assert_close(dx.cpu(), full, atol=2e-5, rtol=2e-5)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal", ATTN_CASES)
def test_attention_fwd_bwd(lib, dtype, B, L, H, causal):
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g).to(tt)
    dout = torch.randn(B, L, H * 64, generator=g).to(tt)
    q32 = qkv.float().requires_grad_(True)
    ref = O.attention(q32, H, O.causal_mask(L) if causal else None)
    (dref,) = torch.autograd.grad(ref, q32, dout.float())
    Lp = lib.mudpt_attention_padded_len(L)
    assert Lp % 32 == 0 and Lp >= L
    qc = qkv.cuda()
    out = torch.empty(B, L, H * 64, device="cuda", dtype=tt)
    lse = torch.empty(B, H, Lp, device="cuda")
    ok(lib, capi.call("mudpt_attention_fwd", dtype=dt, qkv=qc, out=out, lse=lse, B=B, L=L, H=H, causal=int(causal)))
    torch.testing.assert_close(out.cpu().float(), ref.detach(), atol=6 * EPS[dtype], rtol=6 * EPS[dtype])
    # LSE against the definition
    q, k, _ = q32.detach().split(H * 64, dim=-1)
    s = (q.view(B, L, H, 64).transpose(1, 2) @ k.view(B, L, H, 64).transpose(1, 2).transpose(-1, -2)) / 8
    if causal:
        s = s + O.causal_mask(L)
    torch.testing.assert_close(lse.cpu()[:, :, :L], torch.logsumexp(s, dim=-1), atol=1e-3, rtol=1e-4)
    dqkv = torch.zeros(B, L, 3 * H * 64, device="cuda", dtype=tt)
    delta = torch.empty(B, H, Lp, device="cuda")
    doc = dout.cuda()
    ok(lib, capi.call("mudpt_attention_bwd", dtype=dt, qkv=qc, out=out, dout=doc, lse=lse, delta=delta, dqkv=dqkv, B=B, L=L, H=H, causal=int(causal)))
    scale = dref.abs().max().item()
    torch.testing.assert_close(dqkv.cpu().float(), dref, atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype])
    # Every form (fixed summation order, no atomics) is bit for bit the same run to run.  The two-kernel form (bit 1), the fused single
    # pass (bit 3: Q, K, V, dO resident once) and the fused pass with two blocks per wave (bit 2) do the same per-block arithmetic in the
    # same order, compiled separately (fma contraction may differ): the same gradients to T-precision rounding.
    again = torch.zeros_like(dqkv)
    ok(lib, capi.call("mudpt_attention_bwd", dtype=dt, qkv=qc, out=out, dout=doc, lse=lse, delta=delta, dqkv=again, B=B, L=L, H=H, causal=int(causal)))
    assert torch.equal(again, dqkv)
    # bit 4: the single-sweep kernel (non-causal, L <= 224): S / dP / exp computed once, dS rounded to T crosses LDS for dQ -- the same
    # rounding point as the other forms (they round dS to T for the dQ product too)
    for form in attn_bwd_form_flags(L, causal):
        other = torch.full_like(dqkv, float("nan"))
        ok(lib, capi.call("mudpt_attention_bwd", dtype=dt, qkv=qc, out=out, dout=doc, lse=lse, delta=delta, dqkv=other, B=B, L=L, H=H, causal=int(causal) | form))
        torch.testing.assert_close(other.cpu().float(), dref, atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype])
        torch.testing.assert_close(other.float(), dqkv.float(), atol=2 * EPS[dtype] * scale, rtol=2 * EPS[dtype])
        twice = torch.zeros_like(dqkv)
        ok(lib, capi.call("mudpt_attention_bwd", dtype=dt, qkv=qc, out=out, dout=doc, lse=lse, delta=delta, dqkv=twice, B=B, L=L, H=H, causal=int(causal) | form))
        assert torch.equal(twice, other), form


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal,gain", ATTN_LONG_FWD_CASES)
def test_attention_long_forward_forms(lib, dtype, B, L, H, causal, gain):
    """224 < L <= 640: the resident forward (32 queries per wave, rescale deferred until a row's maximum outgrows its reference by 2^6)
    against the staged 16-query-block kernel (flag bit 1) and the definition.  gain 3: scores of +-100 and more, the reference moves at
    most steps and by far more than the threshold; gain 0.05: it never moves after the first step."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(L + int(gain * 10))
    qkv = (torch.randn(B, L, 3 * H * 64, generator=g) * gain)
    qkv[..., 2 * H * 64:] /= gain  # values stay O(1)
    qkv = qkv.to(tt)
    Lp = lib.mudpt_attention_padded_len(L)
    qc = qkv.cuda()
    outs, lses = [], []
    for flag in ATTN_LONG_FWD_FLAGS:
        out = torch.full((B, L, H * 64), float("nan"), device="cuda", dtype=tt)
        lse = torch.full((B, H, Lp), float("nan"), device="cuda")
        ok(lib, capi.call("mudpt_attention_fwd", dtype=dt, qkv=qc, out=out, lse=lse, B=B, L=L, H=H, causal=int(causal) | flag))
        outs.append(out.cpu().float()); lses.append(lse.cpu())
    ref = O.attention(qkv.float(), H, O.causal_mask(L) if causal else None)
    for out in outs:
        torch.testing.assert_close(out, ref, atol=6 * EPS[dtype], rtol=6 * EPS[dtype])
    torch.testing.assert_close(outs[0], outs[1], atol=3 * EPS[dtype], rtol=3 * EPS[dtype])
    torch.testing.assert_close(lses[0][:, :, :L], lses[1][:, :, :L], atol=2e-4, rtol=1e-5)
    assert (lses[0][:, :, L:] == 0).all()  # the padded tail the backward reads


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal", [(5, 201, 12, False), (11, 26, 8, True), (3, 581, 4, False), (4, 77, 2, True), (2, 7, 1, False)])
def test_attention_single_query(lib, dtype, B, L, H, causal):
    """The last block's single-query attention (one query per sequence: CLS row 0 for the vision tower, a different EOT position per
    sequence under the causal mask for the text tower) against the oracle's full attention restricted to that row: output, log-sum-exp,
    dq, and the dK / dV rows of EVERY key (zeros behind the causal limit); bit for bit run to run."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(B * 100 + L)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g).to(tt)
    pos = torch.randint(1, L, (B,), generator=g) if causal else torch.zeros(B, dtype=torch.long)
    sel = (torch.arange(B) * L + pos).to(torch.int32)
    dsel = torch.randn(B, H * 64, generator=g).to(tt)
    q32 = qkv.float().requires_grad_(True)
    ref = O.attention(q32, H, O.causal_mask(L) if causal else None)      # [B, L, H*64]
    ref_sel = ref[torch.arange(B), pos]
    dout = torch.zeros(B, L, H * 64)
    dout[torch.arange(B), pos] = dsel.float()
    (dref,) = torch.autograd.grad(ref, q32, dout)
    qc, sc = qkv.cuda(), sel.cuda()
    q_sel = qkv[torch.arange(B), pos, :H * 64].contiguous().cuda()
    out_sel, lse_sel = torch.empty(B, H * 64, device="cuda", dtype=tt), torch.empty(B, H, device="cuda")
    ok(lib, capi.call("mudpt_attention_fwd_single", dtype=dt, qkv=qc, q_sel=q_sel, sel_rows=sc, out_sel=out_sel, lse_sel=lse_sel, B=B, L=L, H=H, causal=int(causal)))
    torch.testing.assert_close(out_sel.cpu().float(), ref_sel.detach(), atol=6 * EPS[dtype], rtol=6 * EPS[dtype])
    qh, kh = q32.detach()[..., :H * 64].view(B, L, H, 64), q32.detach()[..., H * 64:2 * H * 64].view(B, L, H, 64)
    sco = torch.einsum("bhd,blhd->bhl", qh[torch.arange(B), pos], kh) / 8
    if causal:
        sco = sco.masked_fill(torch.arange(L).view(1, 1, L) > pos.view(B, 1, 1), float("-inf"))
    torch.testing.assert_close(lse_sel.cpu(), torch.logsumexp(sco, dim=-1), atol=1e-3, rtol=1e-4)
    dqkv = torch.full((B, L, 3 * H * 64), 7.0, device="cuda", dtype=tt)  # the q third must stay untouched
    dq_sel = torch.empty(B, H * 64, device="cuda", dtype=tt)
    dc = dsel.cuda()
    bwd_args = dict(dtype=dt, qkv=qc, q_sel=q_sel, sel_rows=sc, out_sel=out_sel, dout_sel=dc, lse_sel=lse_sel, B=B, L=L, H=H, causal=int(causal))
    ok(lib, capi.call("mudpt_attention_bwd_single", dqkv=dqkv, dq_sel=dq_sel, **bwd_args))
    scale = dref.abs().max().item()
    tol = dict(atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype])
    torch.testing.assert_close(dq_sel.cpu().float(), dref[torch.arange(B), pos, :H * 64], **tol)
    torch.testing.assert_close(dqkv.cpu().float()[..., H * 64:], dref[..., H * 64:], **tol)
    assert (dqkv[..., :H * 64] == 7.0).all()
    again, dq2 = torch.zeros_like(dqkv), torch.empty_like(dq_sel)
    ok(lib, capi.call("mudpt_attention_bwd_single", dqkv=again, dq_sel=dq2, **bwd_args))
    assert torch.equal(again[..., H * 64:], dqkv[..., H * 64:]) and torch.equal(dq2, dq_sel)


@pytest.mark.parametrize("B,L,H,causal,row0,n", ATTN_WINDOW_CASES)
def test_attention_backward_window_form(lib, B, L, H, causal, row0, n):
    """Block 0 of a tower needs d(qkv) on the prompt rows only: the window form computes the 16-row blocks (L > 224: 128-row groups) that hold
    rows row0 .. row0 + n - 1 of every sequence -- dQ from all keys, dK / dV from all queries -- and leaves the other rows unwritten.  The
    wanted rows equal the two-kernel form's bit for bit (same sums, same order); the rest of the buffer keeps its previous contents outside
    the computed blocks."""
    dt, tt = DT["bf16"]
    g = torch.Generator().manual_seed(L * 7 + row0)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g).to(tt).cuda()
    dout = torch.randn(B, L, H * 64, generator=g).to(tt).cuda()
    Lp = lib.mudpt_attention_padded_len(L)
    out, lse, delta = torch.empty(B, L, H * 64, device="cuda", dtype=tt), torch.zeros(B, H, Lp, device="cuda"), torch.zeros(B, H, Lp, device="cuda")
    ok(lib, capi.call("mudpt_attention_fwd", dtype=dt, qkv=qkv, out=out, lse=lse, B=B, L=L, H=H, causal=int(causal)))
    full = torch.empty_like(qkv)
    ok(lib, capi.call("mudpt_attention_bwd", dtype=dt, qkv=qkv, out=out, dout=dout, lse=lse, delta=delta, dqkv=full, B=B, L=L, H=H, causal=int(causal) | ATTN_WINDOW_FULL_FLAG))
    delta_full = delta.clone()
    win = torch.full_like(qkv, 3.0)
    delta.zero_()
    ok(lib, capi.call("mudpt_attention_bwd", dtype=dt, qkv=qkv, out=out, dout=dout, lse=lse, delta=delta, dqkv=win, B=B, L=L, H=H, causal=int(causal) | attn_window_flags(row0, n)))
    assert torch.equal(win[:, row0:row0 + n], full[:, row0:row0 + n])
    assert torch.equal(delta[..., :L], delta_full[..., :L])  # delta of every query feeds the dK / dV pass
    gran = 128 if L > 224 else 16
    lo, hi = row0 // gran * gran, min(L, -(-(row0 + n) // gran) * gran)
    untouched = torch.ones(L, dtype=torch.bool)
    untouched[lo:hi] = False
    assert (win[:, untouched] == 3.0).all(), "rows outside the window's blocks must not be written"


def test_attention_softmax_extremes(lib):
    """Large score spread: one key dominates a row (exp underflow for the rest) -- no NaN, matches the oracle."""
    B, L, H = 1, 201, 1
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, L, 192, generator=g)
    qkv[0, 5, :64] *= 30  # query 5: huge logits
    qkv[0, 17, 64:128] *= 30  # key 17: huge against every query
    qkv = qkv.to(torch.float16)
    ref = O.attention(qkv.float(), H, None)
    out = torch.empty(B, L, 64, device="cuda", dtype=torch.float16)
    lse = torch.empty(B, H, 224, device="cuda")
    qc = qkv.cuda()
    ok(lib, capi.call("mudpt_attention_fwd", dtype=1, qkv=qc, out=out, lse=lse, B=B, L=L, H=H))
    assert torch.isfinite(out).all() and torch.isfinite(lse[:, :, :L]).all()
    torch.testing.assert_close(out.cpu().float(), ref, atol=4e-3, rtol=4e-3)


@pytest.mark.parametrize("variant", [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_variants_exact_integers(lib, variant, dtype):
    """Every large-problem GEMM kernel (0 = default: persistent ping-pong kernel; 1, 2, 4 = simple 256x256, 128x256,
    256x128 tiles): exact small-integer operands, ragged M, asymmetric B, K spanning several tiles -> bit-exact."""
    dt, tt = DT[dtype]
    M, N, K = 16500, 1024, 192
    g = torch.Generator().manual_seed(1)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    B = (torch.arange(N).view(N, 1) % 7 - 3 + (torch.arange(K).view(1, K) % 3)).float()
    ref = A @ B.t()
    out = torch.full((M, N), -1.0, device="cuda", dtype=torch.float32)
    gemm(lib, dt, 5, A.cuda().to(tt), B.cuda().to(tt), out0=out, variant=variant)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(33000, 768, 768), (8200, 2304, 768), (22000, 768, 3072)])
def test_gemm_pingpong_epilogues(lib, dtype, shape):
    dt, tt = DT[dtype]
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(tt)
    B = (torch.randn(N, K, generator=g) * K ** -0.5).to(tt)
    bias = torch.randn(N, generator=g)
    acc = A.float() @ B.float().t()  # fp32 CPU reference (fp64 is too slow at this size); tolerances account for it
    Ad, Bd, bd = A.cuda(), B.cuda(), bias.cuda()
    tol = dict(atol=4 * EPS[dtype], rtol=4 * EPS[dtype])
    f32tol = dict(atol=3e-5 * K ** 0.5, rtol=2e-5)
    # default dispatch (variant 0): ping-pong kernel for store / GELU / GELU' / fp32 store, simple 256x256 for residual
    out = torch.empty(M, N, device="cuda", dtype=tt)
    gemm(lib, dt, 0, Ad, Bd, bias=bd, out0=out)
    torch.testing.assert_close(out.cpu().float(), acc + bias, **tol)
    o32 = torch.empty(M, N, device="cuda", dtype=torch.float32)
    gemm(lib, dt, 5, Ad, Bd, out0=o32)
    torch.testing.assert_close(o32.cpu(), acc, **f32tol)
    u, gl = torch.empty(M, N, device="cuda", dtype=tt), torch.empty(M, N, device="cuda", dtype=tt)
    gemm(lib, dt, 1, Ad, Bd, bias=bd, out0=u, out1=gl)
    uref = acc + bias
    torch.testing.assert_close(u.cpu().float(), uref, **tol)
    torch.testing.assert_close(gl.cpu().float(), uref * torch.sigmoid(1.702 * uref), **tol)
    res = torch.randn(M, N, generator=g)
    resd = res.cuda()
    gemm(lib, dt, 2, Ad, Bd, bias=bd, out0=o32, aux=resd)
    torch.testing.assert_close(o32.cpu(), res + uref, **f32tol)
    upre = torch.randn(M, N, generator=g).to(tt)
    upred = upre.cuda()
    gemm(lib, dt, 3, Ad, Bd, out0=out, aux=upred)
    s = torch.sigmoid(1.702 * upre.float())
    torch.testing.assert_close(out.cpu().float(), acc * (s * (1 + 1.702 * upre.float() * (1 - s))), **tol)
    # repeated launches give identical bits (no race in the DMA / barrier protocol shows up as run-to-run change)
    ref_bits = out.clone()
    for _ in range(5):
        gemm(lib, dt, 3, Ad, Bd, out0=out, aux=upred)
        assert torch.equal(out, ref_bits)


# ======================================================================================================================================
# The launchers' PRODUCTION forms, each on its own against float64 (what the whole-model tests reach only on 2-4 image fixtures).
# References are written here from the operation's definition.
# ======================================================================================================================================


def ln_grad64(x, gamma, dy):
    """(d/dx of LayerNorm(x) . dy, mean, rstd) in float64 from the definition (eps 1e-5, biased variance); beta does not enter."""
    x64 = x.double().requires_grad_(True)
    mu = x64.mean(-1, keepdim=True)
    rstd = ((x64 - mu).pow(2).mean(-1, keepdim=True) + 1e-5).rsqrt()
    y = (x64 - mu) * rstd * gamma.double()
    (dx,) = torch.autograd.grad(y, x64, dy.double())
    return dx, mu.detach().float().flatten(), rstd.detach().float().flatten()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["dres", "dres_lp", "dy_f32"])
@pytest.mark.parametrize("nseq,L,d,row0,n", [(256, 201, 768, 197, 4), (1000, 20, 512, 1, 4), (5, 13, 192, 9, 4)])
def test_layernorm_bwd_fused_splice_backward(lib, dtype, kind, nseq, L, d, row0, n):
    """ln_1's backward as block_bwd launches it: dx = dres + LN'(dy) with the residual gradient in fp32 (dres) or in T (dres_lp, the bf16
    mode's stream), and the splice backward fused in: rows row0 .. row0 + n - 1 of every sequence go, in fp32, to side[seq][n][d] (sequence
    stride side_ldb > n d) and dx / dx_lp get exact zeros there.  The benchmark's vision tower (256 x 201 rows of 768, rows 197..200), the
    text tower (1000 x 20 of 512, rows 1..4) and a ragged shape whose last block of 4 rows is partial; every row of every sequence is checked
    against float64 autograd, and everything outside the written rows must keep its sentinel.  "dy_f32": fp32 dy with the identity row map."""
    dt, tt = DT[dtype]
    rows = nseq * L
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * 2 + 0.5
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g)
    dy = dy if kind == "dy_f32" else dy.to(tt)
    dres = torch.randn(rows, d, generator=g)
    dres = dres.to(tt) if kind == "dres_lp" else dres
    dln, mean, rstd = ln_grad64(x, gamma, dy)
    full = (dln + dres.double()).view(nseq, L, d)
    side_ldb = n * d + 64
    side = torch.full((nseq + 1, side_ldb), SENT, device="cuda")
    dx = torch.full((rows + 1, d), SENT, device="cuda")
    dx_lp = torch.full((rows + 1, d), SENT, device="cuda", dtype=tt)
    xc, gc, dyc, drc, mc, rc_ = x.cuda(), gamma.cuda(), dy.cuda(), dres.cuda(), mean.cuda(), rstd.cuda()
    ok(lib, capi.call("mudpt_layernorm_bwd_ex", dtype=dt, dy=dyc, lddy=d, dy_f32=int(kind == "dy_f32"), x=xc, ldx=d, mean=mc, rstd=rc_, gamma=gc,
                      dres=None if kind == "dres_lp" else drc, dres_lp=drc if kind == "dres_lp" else None, lddres=d, dx=dx, lddx=d, dx_lp=dx_lp, lddx_lp=d,
                      side=side, side_row0=row0, side_n=n, side_L=L, side_ldb=side_ldb, index_mode=0, rows=rows, d=d))
    got, got_lp, sv = dx.cpu(), dx_lp.cpu(), side.cpu()
    assert (got[rows:] == SENT).all() and (got_lp[rows:] == SENT).all()
    got, got_lp = got[:rows].view(nseq, L, d), got_lp[:rows].view(nseq, L, d)
    keep = torch.ones(L, dtype=torch.bool)
    keep[row0:row0 + n] = False
    torch.testing.assert_close(got[:, keep].double(), full[:, keep], atol=2e-5, rtol=2e-5)
    torch.testing.assert_close(got_lp[:, keep].double(), full[:, keep], atol=16 * EPS[dtype], rtol=4 * EPS[dtype])
    assert (got[:, ~keep] == 0).all() and (got_lp[:, ~keep] == 0).all()  # the rows the splice overwrote receive no gradient
    torch.testing.assert_close(sv[:nseq, :n * d].view(nseq, n, d).double(), full[:, ~keep], atol=2e-5, rtol=2e-5)
    assert (sv[:nseq, n * d:] == SENT).all() and (sv[nseq] == SENT).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("total,R,d", [(65, 21, 192), (20000, 4000, 512), (51456, 1024, 768)])
def test_layernorm_bwd_token_index_modes(lib, dtype, mode, total, R, d):
    """row_index with the statistics (mode 2: block 0's ln_1 on the prompt rows) or dy and the statistics (mode 1: ln_pre on the prompt
    rows) indexed by TOKEN row instead of by r, on a permuted, non-contiguous row list: x, dres and the result at row_index[r], reference by
    direct indexing; rows not named keep the sentinel.  bf16 runs the stream forms of that mode (T dy, T dres), fp16 the fp32 ones."""
    dt, tt = DT[dtype]
    lp = dtype == "bf16"
    g = torch.Generator().manual_seed(total + mode)
    idx = torch.randperm(total, generator=g)[:R]
    x = torch.randn(total, d, generator=g) * 2 + 0.5
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(total if mode == 1 else R, d, generator=g)
    dy = dy.to(tt) if lp else dy
    dres = torch.randn(total, d, generator=g)
    dres = dres.to(tt) if lp else dres
    mean = x.double().mean(-1)                                        # statistics of EVERY token row, indexed by token
    rstd = ((x.double() - mean.unsqueeze(-1)).pow(2).mean(-1) + 1e-5).rsqrt().float()
    mean = mean.float()
    dln, _, _ = ln_grad64(x[idx], gamma, dy[idx] if mode == 1 else dy)
    want = dln + dres[idx].double()
    dx = torch.full((total, d), SENT, device="cuda")
    dx_lp = torch.full((total, d), SENT, device="cuda", dtype=tt)
    xc, gc, dyc, drc, mc, rc_, ic = x.cuda(), gamma.cuda(), dy.cuda(), dres.cuda(), mean.cuda(), rstd.cuda(), idx.to(torch.int32).cuda()
    ok(lib, capi.call("mudpt_layernorm_bwd_ex", dtype=dt, dy=dyc, lddy=d, dy_f32=int(not lp), x=xc, ldx=d, row_index=ic, mean=mc, rstd=rc_, gamma=gc,
                      dres=None if lp else drc, dres_lp=drc if lp else None, lddres=d, dx=dx, lddx=d, dx_lp=dx_lp, lddx_lp=d, side_L=1, index_mode=mode, rows=R, d=d))
    got, got_lp = dx.cpu(), dx_lp.cpu()
    torch.testing.assert_close(got[idx].double(), want, atol=2e-5, rtol=2e-5)
    torch.testing.assert_close(got_lp[idx].double(), want, atol=16 * EPS[dtype], rtol=4 * EPS[dtype])
    rest = torch.ones(total, dtype=torch.bool)
    rest[idx] = False
    assert (got[rest] == SENT).all() and (got_lp[rest] == SENT).all()


def run_attn_split(lib, dt, tt, qc, B, L, H, flags, ld, pass_ld, lo_mode, single=None):
    """One forward through the split export: (out [rows + 1, ld] T, lo bytes [rows + 1, 2 ld] or None, lse); sentinel-filled beforehand."""
    rows = B if single else B * L
    out = torch.full((rows + 1, ld), SENT, device="cuda", dtype=tt)
    lo = torch.full((rows + 1, 2 * ld), 0x5A, device="cuda", dtype=torch.uint8) if lo_mode else None
    if single:
        q_sel, sel = single
        lse = torch.full((B, H), float("nan"), device="cuda")
        ok(lib, capi.call("mudpt_attention_fwd_single_split", dtype=dt, qkv=qc, q_sel=q_sel, sel_rows=sel, out_sel=out, out_lo=lo, lo_mode=lo_mode, ld_out=ld, lse_sel=lse,
                          B=B, L=L, H=H, causal=flags))
    else:
        lse = torch.full((B, H, lib.mudpt_attention_padded_len(L)), float("nan"), device="cuda")
        ok(lib, capi.call("mudpt_attention_fwd_split", dtype=dt, qkv=qc, out=out, out_lo=lo, lo_mode=lo_mode, ld_out=pass_ld, lse=lse, B=B, L=L, H=H, causal=flags))
    return out.cpu(), None if lo is None else lo.cpu(), lse.cpu()


def check_split_outputs(dtype, tt, runs, rows, Hd, ld, ref):
    (o0, _, l0), (o1, lo1, l1), (o2, lo2, l2) = runs
    for o, l in ((o1, l1), (o2, l2)):
        ndiff = (o.view(torch.int16) != o0.view(torch.int16)).sum().item()
        codes = (o.view(torch.int16).int() - o0.view(torch.int16).int()).abs().max().item()
        print(f"split output {dtype}: {ndiff} of {o0[:rows, :Hd].numel()} elements of `out` differ from the call without out_lo, at most {codes} code(s)")
        assert torch.equal(o.view(torch.int16), o0.view(torch.int16)), "out must not depend on out_lo"
        assert torch.equal(l.view(torch.int32), l0.view(torch.int32))
    assert (o0[rows:] == SENT).all() and (o0[:, Hd:] == SENT).all()          # columns H*64 .. ld_out and the row behind the last: untouched
    assert (lo1[rows:] == 0x5A).all() and (lo1[:, 2 * Hd:] == 0x5A).all()     # T remainder: the same columns, in bytes
    assert (lo2[rows:] == 0x5A).all() and (lo2[:, Hd:] == 0x5A).all()         # e4m3 remainder: H*64 bytes, then padding up to 2 ld_out bytes
    check_split_pair(dtype, o0[:rows, :Hd], lo1[:rows].view(tt)[:, :Hd], lo2[:rows, :Hd], ref.reshape(rows, Hd))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("B,L,H,flags", [(2, 201, 12, 0), (1, 581, 3, 0), (1, 581, 3, 2), (1, 641, 2, 2), (3, 77, 8, 1)])
def test_attention_fwd_split_output(lib, dtype, pad, B, L, H, flags):
    """The attention forward writing a split operand (the parity mode's vision tower: fp16 attention, e4m3 remainders), at each forward
    kernel's range: L <= 224 (201, and the causal 77), the resident form (581), the staged 16-query-block form (581 with flag bit 1, 641), in
    rows of ld_out = H*64 (passed as 0) and H*64 + 64 elements.  For both lo_modes `out` and lse are bit-identical to the call without
    out_lo; hi + lo against float64; the columns between H*64 and ld_out, the unused part of each e4m3 row and the row behind the last one
    keep their sentinel.
    This test found a defect: in fp16 the two store sites of attention.hip (L <= 224 and the staged kernel) wrote an `out` one code away
    from the call without out_lo on ~4e-5 of the elements -- the plain store's cast was fused with the multiply by 1 / l into one rounding
    of the exact product, the split store rounds the fp32 product first.  The plain store now rounds the fp32 product too
    (Attn::store_t_out)."""
    dt, tt = DT[dtype]
    Hd, ld = H * 64, H * 64 + pad
    g = torch.Generator().manual_seed(L * 3 + H + flags)
    qkv = torch.randn(B, L, 3 * Hd, generator=g).to(tt)
    ref = attn64(qkv, H, bool(flags & 1))
    qc = qkv.cuda()
    runs = [run_attn_split(lib, dt, tt, qc, B, L, H, flags, ld, ld if pad else 0, m) for m in (0, 1, 2)]
    check_split_outputs(dtype, tt, runs, B * L, Hd, ld, ref)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal", [(5, 201, 12, False), (4, 77, 8, True), (3, 581, 4, False)])
def test_attention_single_query_split_output(lib, dtype, B, L, H, causal):
    """The single-query forward (the last block) writing its one row per sequence as a split operand with ld_out > H*64: same rules."""
    dt, tt = DT[dtype]
    Hd, ld = H * 64, H * 64 + 64
    g = torch.Generator().manual_seed(B * 10 + L)
    qkv = torch.randn(B, L, 3 * Hd, generator=g).to(tt)
    pos = torch.randint(1, L, (B,), generator=g) if causal else torch.zeros(B, dtype=torch.long)
    ref = attn64(qkv, H, causal)[torch.arange(B), pos]
    qc = qkv.cuda()
    single = (qkv[torch.arange(B), pos, :Hd].contiguous().cuda(), (torch.arange(B) * L + pos).to(torch.int32).cuda())
    runs = [run_attn_split(lib, dt, tt, qc, B, L, H, int(causal), ld, ld, m, single=single) for m in (0, 1, 2)]
    check_split_outputs(dtype, tt, runs, B, Hd, ld, ref)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("L,H,causal", ATTN_SEL_CASES)
def test_attention_bwd_sel_rows(lib, dtype, L, H, causal):
    """The backward where dout is zero except on ONE row per sequence (the last block with last_single = 0, the class-parallel path): one
    sequence per row position -- first block, last row, and both sides of every 16 / 32 / 64 / 128 boundary below L (under the causal mask:
    a different EOT position per sequence) -- against float64 autograd with that dout.  The form skips query blocks whose dout is zero; the
    general two-kernel form (flag bit 1) on the same dout adds those blocks' exact zeros to the same sums in the same order, so the two are
    equal element for element (a zero may differ in sign: compared by value).  Against the default dispatch (other kernels, another
    association) the form-to-form tolerance of test_attention_fwd_bwd holds.  Bit for bit run to run."""
    dt, tt = DT[dtype]
    pos = torch.tensor(sorted({p for p in (0, 15, 16, 31, 32, 63, 64, 127, 128) if p < L} | {L - 1}))
    B, Hd = len(pos), H * 64
    g = torch.Generator().manual_seed(L + H)
    qkv = torch.randn(B, L, 3 * Hd, generator=g).to(tt)
    dout = torch.zeros(B, L, Hd, dtype=tt)
    dout[torch.arange(B), pos] = torch.randn(B, Hd, generator=g).to(tt)
    q64 = qkv.double().requires_grad_(True)
    (dref,) = torch.autograd.grad(attn64(q64, H, causal), q64, dout.double())
    Lp = lib.mudpt_attention_padded_len(L)
    qc, doc, sel = qkv.cuda(), dout.cuda(), (torch.arange(B) * L + pos).to(torch.int32).cuda()
    out, lse = torch.empty(B, L, Hd, device="cuda", dtype=tt), torch.zeros(B, H, Lp, device="cuda")
    ok(lib, capi.call("mudpt_attention_fwd", dtype=dt, qkv=qc, out=out, lse=lse, B=B, L=L, H=H, causal=int(causal)))
    delta = torch.zeros(B, H, Lp, device="cuda")
    res = []
    for _ in range(2):
        dqkv = torch.full((B, L, 3 * Hd), float("nan"), device="cuda", dtype=tt)
        ok(lib, capi.call("mudpt_attention_bwd_sel", dtype=dt, qkv=qc, out=out, dout=doc, lse=lse, delta=delta, dqkv=dqkv, sel_rows=sel, B=B, L=L, H=H, causal=int(causal)))
        res.append(dqkv.cpu())
    assert torch.equal(res[0].view(torch.int16), res[1].view(torch.int16))
    scale = dref.abs().max().item()
    torch.testing.assert_close(res[0].double(), dref, atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype])
    for flag, same in ATTN_SEL_COMPARE:
        gen = torch.full((B, L, 3 * Hd), float("nan"), device="cuda", dtype=tt)
        ok(lib, capi.call("mudpt_attention_bwd", dtype=dt, qkv=qc, out=out, dout=doc, lse=lse, delta=delta, dqkv=gen, B=B, L=L, H=H, causal=int(causal) | flag))
        if same:
            assert torch.equal(res[0], gen.cpu())
        else:
            torch.testing.assert_close(res[0].float(), gen.cpu().float(), atol=2 * EPS[dtype] * scale, rtol=2 * EPS[dtype])


# ---- the head: fused and unfused launchers, the shapes where the dispatch changes --------------------------------------------------
def head_fits(C, e, train):
    """head.hip's rule, recomputed from its documentation: a workgroup keeps [16][e] normalised image rows (training: plus a [16][e] gradient
    tile) and [16][Cpad] logits in fp32 in LDS, plus 256 bytes of static LDS, within 160 KB; e is a multiple of 16; when training, e <= 1024
    (the text-side kernel's [16][e] tile within its 64 KB)."""
    Cpad = (C + 15) // 16 * 16
    return e % 16 == 0 and (not train or e <= 1024) and (16 * e * (2 if train else 1) + 16 * Cpad) * 4 + 256 <= 163840


def head_inputs(B, C, e):
    g = torch.Generator().manual_seed(B * 1000 + C + e)
    return torch.randn(B, e, generator=g) * 3, torch.randn(C, e, generator=g) * 0.2, torch.randint(0, C, (B,), generator=g)


def peaked_inputs(B=16, C=1000, e=512):
    """Pretrained-like statistics at logit scale 100: every image has cosine ~0.9 with ONE class and ~0 with the rest; half of the labels
    name that class (loss ~0, softmax saturated), half another one (loss ~90)."""
    g = torch.Generator().manual_seed(77)
    txt = torch.randn(C, e, generator=g)
    peak = torch.randint(0, C, (B,), generator=g)
    tn = torch.nn.functional.normalize(txt, dim=-1)
    noise = torch.nn.functional.normalize(torch.randn(B, e, generator=g), dim=-1)
    img = (0.9 * tn[peak] + (1 - 0.81) ** 0.5 * noise) * 7.0
    labels = peak.clone()
    labels[1::2] = (peak[1::2] + 1 + torch.randint(0, C - 1, (B // 2,), generator=g)) % C
    return img, txt * 0.3, labels


def head_eval(img, txt, labels, scale, gscale, dtype):
    """The head from its definition (trainers/mudpt.py:178-182, :250) in `dtype`: logits, per-row CE, mean CE, gradients of gscale * loss."""
    i, t = img.detach().clone().to(dtype).requires_grad_(True), txt.detach().clone().to(dtype).requires_grad_(True)  # fresh leaves: .to() of the same dtype is no copy
    logits = scale * torch.nn.functional.normalize(i, dim=-1) @ torch.nn.functional.normalize(t, dim=-1).t()
    out = {"logits": logits.detach()}
    if labels is not None:
        rows = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
        loss = rows.mean()
        (gscale * loss).backward()
        out.update(row_loss=rows.detach(), loss=loss.detach(), dimg=i.grad, dtxt=t.grad)
    return out


def head_errors(got, ref):
    """Error figures of one head evaluation against the float64 one: logits (absolute), loss (relative to max(1, |loss|)), gradients (relative
    to the gradient's RMS)."""
    err = {"logits": (got["logits"].double() - ref["logits"]).abs().max().item()}
    if "loss" in ref:
        err["loss"] = abs(float(got["loss"]) - float(ref["loss"])) / max(1.0, abs(float(ref["loss"])))
        err["row_loss"] = ((got["row_loss"].double() - ref["row_loss"]).abs() / ref["row_loss"].abs().clamp_min(1.0)).max().item()
        for k in ("dimg", "dtxt"):
            if got.get(k) is not None:
                err[k] = (got[k].double() - ref[k]).abs().max().item() / (ref[k].pow(2).mean().sqrt().item() + 1e-300)
    return err


def run_head(lib, img, txt, labels, scale, gscale, path, B_total=0, state=None, want_dtxt=True):
    """mudpt_head_ex on device copies: returns the outputs on the CPU, the path that ran (0 fused, 1 unfused) and the text state
    (txt_n, txt_inv) for a following call with txt = None."""
    B, e = img.shape
    Cn = state[0].shape[0] if txt is None else txt.shape[0]
    ic, tc, lc = img.cuda(), None if txt is None else txt.cuda(), None if labels is None else labels.cuda()
    txt_n, txt_inv = state if state is not None else (torch.full((Cn, e), SENT, device="cuda"), torch.full((Cn,), SENT, device="cuda"))
    logits = torch.full((B, Cn), SENT, device="cuda")
    loss, row_loss = torch.full((1,), SENT, device="cuda"), torch.full((B,), SENT, device="cuda")
    dimg, dtxt = torch.full((B, e), SENT, device="cuda"), torch.full((Cn, e), SENT, device="cuda")
    taken = C.c_int32(-1)
    train = labels is not None
    rc = lib.mudpt_head_ex(P(ic), P(tc), P(lc), scale, gscale, B, B_total, Cn, e, P(txt_n), P(txt_inv), P(logits), P(loss) if train else None,
                           P(row_loss) if train else None, P(dimg) if train else None, P(dtxt) if train and want_dtxt else None, path,
                           C.byref(taken), None)
    assert rc == 0, lib.mudpt_last_error().decode()
    torch.cuda.synchronize()
    out = {"logits": logits.cpu(), "loss": loss.cpu()[0], "row_loss": row_loss.cpu(), "dimg": dimg.cpu(), "dtxt": dtxt.cpu() if want_dtxt else None,
           "dtxt_raw": dtxt.cpu()}
    return out, taken.value, (txt_n, txt_inv)


# Bounds of the fused head: the suite's (test_head_matches_torch_cross_entropy).
FUSED_BOUND = {"logits": 2e-5, "loss": 2e-6, "row_loss": 2e-6, "dimg": 2e-5, "dtxt": 2e-5}

HEAD_CASES = [(256, 1000, 512, True), (64, 1520, 512, True), (64, 1521, 512, True), (32, 1008, 768, True), (32, 1009, 768, True),
              (8, 2032, 512, False), (8, 2033, 512, False), (5, 7, 72, True), (4, 9, 1040, True)]


_MEASURED = {}


def measured_bound(kind):
    """The bound of a path the suite had none for -- the unfused launchers (l2norm, sgemm, ce_rows with __expf, mean; kind "unfused") and the
    peaked scale-100 row (kind "peaked") -- computed here, not stored: the error of a plain fp32 CPU evaluation of the same formula on the
    same inputs (head_eval with torch.float32) against the float64 one, worst case per figure over HEAD_CASES resp. on peaked_inputs, times
    4.  The figures depend a little on the CPU's fp32 summation order, which is why they are taken on the machine that runs the test; they
    are printed with every use (logits absolute, loss and row losses relative to max(1, |loss|), gradients relative to their RMS)."""
    if kind not in _MEASURED:
        worst = {}
        cases = [(head_inputs(B, Cn, e), 14.2857, 0.5, train) for B, Cn, e, train in HEAD_CASES] if kind == "unfused" else [(peaked_inputs(), 100.0, 1.0, True)]
        for (img, txt, labels), scale, gscale, train in cases:
            labels = labels if train else None
            err = head_errors(head_eval(img, txt, labels, scale, gscale, torch.float32), head_eval(img, txt, labels, scale, gscale, torch.float64))
            for k, v in err.items():
                worst[k] = max(worst.get(k, 0.0), v)
        print(f"fp32 CPU against float64, {kind}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + "; 4x that is allowed")
        _MEASURED[kind] = {k: 4 * v for k, v in worst.items()}
    return _MEASURED[kind]


def within(err, bound, what):
    for k, v in err.items():
        assert v <= bound[k], f"{what}: {k} error {v:.3e} exceeds {bound[k]:.3e}"


@pytest.mark.parametrize("B,C,e,train", HEAD_CASES)
def test_head_both_paths_at_the_dispatch_boundaries(lib, B, C, e, train):
    """The head's float64 comparison through BOTH implementations -- the fused kernels of head.hip and the unfused launchers of
    elementwise.hip (l2norm, sgemm, ce_rows, mean, l2norm backward) that the dispatch falls back to -- at the benchmark's (256, 1000, 512),
    on both sides of each LDS boundary (training: C = 1520 | 1521 at e = 512, 1008 | 1009 at e = 768 = ViT-L/14 with 1000 classes + one tile;
    forward only: 2032 | 2033), at e = 72 (not a multiple of 16) and at e = 1040 (beyond the text-side kernel's 64 KB: the training head
    must fall back, the forward still fuses).  Which path ran is asserted from mudpt_head_ex against the documented rule.
    The fused path keeps the suite's head bounds; the unfused one is held to measured_bound("unfused"): fp32 CPU against float64 measured
    logits 1.7e-6, loss 5.2e-8, row losses 1.4e-7, dimg 5.4e-6 rms, dtxt 9.5e-6 rms (x86-64, any thread count), so the bound is
    6.8e-6 / 2.1e-7 / 5.6e-7 / 2.2e-5 / 3.8e-5 there."""
    img, txt, labels = head_inputs(B, C, e)
    labels = labels if train else None
    scale, gscale = 14.2857, 0.5
    ref = head_eval(img, txt, labels, scale, gscale, torch.float64)
    fits = head_fits(C, e, train)
    outs = {}
    for path in (0, 1):
        out, taken, _ = run_head(lib, img, txt, labels, scale, gscale, path)
        assert taken == (0 if path == 0 and fits else 1), (path, taken, fits)
        err = head_errors(out, ref)
        print(f"head B {B} C {C} e {e} train {train} path {path} -> {'fused' if taken == 0 else 'unfused'}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        within(err, FUSED_BOUND if taken == 0 else measured_bound("unfused"), f"path {path}")
        outs[path] = out
    # the two implementations agree to the fp32 tolerance of the suite
    torch.testing.assert_close(outs[0]["logits"], outs[1]["logits"], atol=2e-5, rtol=1e-5)
    if train:
        assert abs(outs[0]["loss"] - outs[1]["loss"]).item() <= 2e-6 * max(1.0, abs(float(ref["loss"])))
        for k in ("dimg", "dtxt"):
            assert (outs[0][k] - outs[1][k]).abs().max().item() <= 2e-5 * ref[k].pow(2).mean().sqrt().item()
    assert head_fits(1520, 512, True) and not head_fits(1521, 512, True) and head_fits(1008, 768, True) and not head_fits(1009, 768, True)
    assert head_fits(2032, 512, False) and not head_fits(2033, 512, False) and not head_fits(9, 1040, True) and head_fits(9, 1040, False)


@pytest.mark.parametrize("path", [0, 1])
def test_head_peaked_rows_at_logit_scale_100(lib, path):
    """One class at cosine ~0.9 and the rest ~0 at exp(logit_scale) = 100: logits up to 90, a saturated softmax on half of the rows and a
    loss of ~90 on the other half.  Loss, row losses and both gradients against float64, on the fused and on the unfused path, within
    measured_bound("peaked"): fp32 CPU against float64 measured logits 3.7e-5, loss 3.0e-8, row losses 3.0e-7, dimg 8.4e-7 rms, dtxt
    5.0e-6 rms (x86-64, any thread count), so the bound is 1.5e-4 / 1.2e-7 / 1.2e-6 / 3.4e-6 / 2.0e-5 there."""
    img, txt, labels = peaked_inputs()
    ref = head_eval(img, txt, labels, 100.0, 1.0, torch.float64)
    assert ref["logits"].max().item() > 85 and ref["row_loss"].max().item() > 60 and ref["row_loss"].min().item() < 1e-6
    out, taken, _ = run_head(lib, img, txt, labels, 100.0, 1.0, path)
    assert taken == path
    err = head_errors(out, ref)
    print(f"peaked head path {path}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    within(err, measured_bound("peaked"), f"path {path}")


@pytest.mark.parametrize("path", [0, 1])
def test_head_cached_text_no_text_gradient_and_chunks(lib, path):
    """The other forms of the head, each alone: txt = NULL (the normalised text features of the previous call are reused: fused path only,
    the unfused launchers refuse it) gives bit-identical logits; dtxt = NULL (VPT) leaves a sentinel-filled dtxt untouched and changes
    nothing else; two calls over the halves of the batch with B_total = B give the unchunked row losses and image gradients bit for bit
    (every row is independent of the others) and text gradients that sum to the unchunked ones to fp32 rounding, and do not write `loss`."""
    B, Cn, e = 64, 100, 512
    img, txt, labels = head_inputs(B, Cn, e)
    scale, gscale = 14.2857, 0.5
    whole, taken, state = run_head(lib, img, txt, labels, scale, gscale, path)
    assert taken == path
    if path == 0:
        again, _, _ = run_head(lib, img, None, labels, scale, gscale, path, state=state)
        for k in ("logits", "row_loss", "dimg", "dtxt"):
            assert torch.equal(again[k], whole[k]), k
        fwd, _, _ = run_head(lib, img, None, None, scale, gscale, path, state=state)
        assert torch.equal(fwd["logits"], whole["logits"])
    else:
        lg, ic = torch.full((B, Cn), SENT, device="cuda"), img.cuda()
        rc = lib.mudpt_head_ex(P(ic), None, None, scale, gscale, B, 0, Cn, e, P(state[0]), P(state[1]), P(lg), None, None, None, None, 1, None, None)
        assert rc == 1 and b"head" in lib.mudpt_last_error() and (lg == SENT).all()
    vpt, _, _ = run_head(lib, img, txt, labels, scale, gscale, path, want_dtxt=False)
    assert (vpt["dtxt_raw"] == SENT).all()
    for k in ("logits", "row_loss", "dimg"):
        assert torch.equal(vpt[k], whole[k]), k
    assert vpt["loss"] == whole["loss"]
    h = B // 2
    parts = [run_head(lib, img[s], txt, labels[s], scale, gscale, path, B_total=B)[0] for s in (slice(0, h), slice(h, B))]
    assert all(p["loss"] == SENT for p in parts)
    for k in ("logits", "row_loss", "dimg"):
        assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
    ref = head_eval(img, txt, labels, scale, gscale, torch.float64)
    assert ((parts[0]["dtxt"] + parts[1]["dtxt"]) - whole["dtxt"]).abs().max().item() <= 2e-5 * ref["dtxt"].pow(2).mean().sqrt().item()
    assert abs(float(torch.cat([p["row_loss"] for p in parts]).double().mean()) - float(ref["loss"])) <= 2e-6 * max(1.0, float(ref["loss"]))


def test_head_label_out_of_range_on_the_unfused_path(lib):
    """As test_head_label_out_of_range_gives_nan_loss_not_a_fault, through the unfused launchers (ce_rows_kernel)."""
    g = torch.Generator().manual_seed(4)
    img, txt = torch.randn(4, 64, generator=g), torch.randn(7, 64, generator=g)
    labels = torch.tensor([0, 7, 3, -1])  # 7 and -1 are outside [0, C)
    out, taken, _ = run_head(lib, img, txt, labels, 10.0, 1.0, 1)
    assert taken == 1 and torch.isnan(out["loss"]) and torch.isfinite(out["logits"]).all()
    assert torch.isnan(out["row_loss"][[1, 3]]).all() and torch.isfinite(out["row_loss"][[0, 2]]).all()
    assert torch.isfinite(out["dimg"]).all() and torch.isfinite(out["dtxt"]).all()


def pair_eval(img, txt, labels, scale, gscale, B_total=0):
    """CoCoOp's head from its definition in float64: logits[i, c] = scale <normalise(img_i), normalise(txt_{i,c})>, mean CE over the batch."""
    B, C, e = txt.shape
    t = txt.double().requires_grad_(True)
    logits = scale * torch.einsum("be,bce->bc", torch.nn.functional.normalize(img.double(), dim=-1), torch.nn.functional.normalize(t, dim=-1))
    rows = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
    (gscale * rows.sum() / (B_total or B)).backward()
    return {"logits": logits.detach(), "row_loss": rows.detach(), "loss": rows.mean().detach(), "dtxt": t.grad}


def run_pair(lib, img, txt, labels, scale, gscale, B_total=0):
    B, C, e = txt.shape
    ic, tc, lc = img.cuda(), txt.reshape(B * C, e).cuda(), labels.cuda()
    logits, loss, row_loss = torch.full((B, C), SENT, device="cuda"), torch.full((1,), SENT, device="cuda"), torch.full((B,), SENT, device="cuda")
    dtxt = torch.full((B * C + 1, e), SENT, device="cuda")
    ok(lib, lib.mudpt_pair_head(P(ic), P(tc), P(lc), scale, gscale, B, B_total, C, e, P(logits), P(loss), P(row_loss), P(dtxt), None))
    torch.cuda.synchronize()
    assert (dtxt[B * C:] == SENT).all()
    return {"logits": logits.cpu(), "loss": loss.cpu()[0], "row_loss": row_loss.cpu(), "dtxt": dtxt[:B * C].cpu().view(B, C, e)}


@pytest.mark.parametrize("B,C,e", [(64, 11, 512), (3, 100, 512), (2, 5, 128)])
def test_pair_head(lib, B, C, e):
    """CoCoOp's head (launch_l2norm, launch_pair_head_fwd / _bwd, launch_mean) against float64 autograd with the head's bounds; chunked over
    the images with B_total = B: logits, row losses and text gradients bit for bit the unchunked ones, `loss` left to the caller."""
    g = torch.Generator().manual_seed(B * C + e)
    img, txt, labels = torch.randn(B, e, generator=g) * 3, torch.randn(B, C, e, generator=g) * 0.2, torch.randint(0, C, (B,), generator=g)
    scale, gscale = 14.2857, 0.5
    ref = pair_eval(img, txt, labels, scale, gscale)
    got = run_pair(lib, img, txt, labels, scale, gscale)
    err = head_errors(got, ref)
    print(f"pair head B {B} C {C} e {e}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    within(err, FUSED_BOUND, "pair head")
    h = max(1, B // 2)
    parts = [run_pair(lib, img[s], txt[s], labels[s], scale, gscale, B_total=B) for s in (slice(0, h), slice(h, B))]
    assert all(p["loss"] == SENT for p in parts)
    for k in ("logits", "row_loss", "dtxt"):
        assert torch.equal(torch.cat([p[k] for p in parts]), got[k]), k


# ---- refusals: every launcher validates on the host before the launch (kernels.h) -----------------------------------------------------
# Every case below is built so that a launch WITHOUT the check would still stay inside the (oversized) allocations: strides that are wrong
# but in bounds, buffers larger than the shape needs.  Nothing relies on a fault being caught.
def test_layernorm_launchers_refuse_bad_arguments(lib):
    rows, d = 16, 64
    f = lambda *shape: torch.full(shape, SENT, device="cuda")  # noqa: E731
    x, g, st = torch.randn(2 * rows, d, device="cuda"), torch.ones(d, device="cuda"), torch.ones(2 * rows, device="cuda")
    h = torch.full((2 * rows, d), SENT, device="cuda", dtype=torch.float16)
    dx, side, idx = f(2 * rows, d), f(2 * rows, d), torch.arange(rows, dtype=torch.int32, device="cuda")
    bwd_args = dict(dtype=1, dy=h, lddy=d, x=x, ldx=d, mean=st, rstd=st, gamma=g, lddres=d, dx=dx, lddx=d, lddx_lp=d, side_L=1, rows=rows, d=d)
    bwd = lambda **k: capi.call("mudpt_layernorm_bwd_ex", **{**bwd_args, **k})  # noqa: E731
    refused(lib, bwd(dres=x, dres_lp=h), "exclusive")                       # both residual gradients
    refused(lib, bwd(dres=x, lddres=d - 4), "dres stride")                 # a stride shorter than the row
    refused(lib, bwd(dres_lp=h, lddres=d - 4), "dres stride")              # ... of the T stream as well
    refused(lib, bwd(dx_lp=h, lddx_lp=d - 4), "dx_lp stride")
    refused(lib, bwd(ldx=d - 4), "shorter than d")
    refused(lib, bwd(lddy=d - 4), "shorter than d")
    refused(lib, bwd(lddx=d - 4), "shorter than d")
    refused(lib, bwd(side=side, side_row0=2, side_n=3, side_L=4, side_ldb=3 * d), "splice rows")   # rows 2..4 of a 4-row sequence
    refused(lib, bwd(side=side, side_row0=1, side_n=2, side_L=4, side_ldb=d), "splice rows")       # two rows do not fit a side stride of d
    refused(lib, bwd(side=side, side_row0=1, side_n=2, side_L=4, side_ldb=2 * d, row_index=idx), "identity row map")
    refused(lib, bwd(index_mode=3), "index_mode")
    assert (dx == SENT).all() and (side == SENT).all() and (h == SENT).all()
    out, xo = f(2 * rows, d), f(2 * rows, d)
    fwd_args = dict(dtype=1, x=x, ldx=d, ldadd=d, ov_L=1, ldxout=d, gamma=g, beta=g, out=out, ldo=d, out_f32=1, rows=rows, d=d)
    fwd = lambda name="mudpt_layernorm_fwd_fused", **k: capi.call(name, **{**fwd_args, **k})  # noqa: E731
    refused(lib, fwd(add=x, ldadd=d - 4), "addend stride")
    refused(lib, fwd(xout=xo, ldxout=d - 4), "xout stride")
    refused(lib, fwd(ov_rows=x, ov_row0=0, ov_n=1, ov_L=0), "splice rows")  # ov_L = 0: r % ov_L
    refused(lib, fwd(ov_rows=x, ov_row0=3, ov_n=2, ov_L=4), "splice rows")  # rows 3..4 of a 4-row sequence
    # the row map next to a fused operand (out is indexed by r, x / add / xout by row_index[r]) and a split output that is not T
    lo = torch.full((2 * rows, 2 * d), SENT, device="cuda")
    ex = lambda **k: fwd("mudpt_layernorm_fwd_ex", **{"ov_L": 4, "lo_mode": 1, "out_f32": 0, **k})  # noqa: E731
    refused(lib, ex(row_index=idx, add=x), "identity row map")
    refused(lib, ex(row_index=idx, xout=xo), "identity row map")
    refused(lib, ex(row_index=idx, ov_rows=x, ov_row0=0, ov_n=2, ov_L=4), "identity row map")
    refused(lib, ex(out_lo=lo, lo_mode=1, out_f32=1), "out_lo needs a T output")
    refused(lib, ex(out_lo=lo, lo_mode=3), "out_lo needs a T output")
    assert (out == SENT).all() and (xo == SENT).all() and (lo == SENT).all()


def test_attention_forward_refuses_a_bad_split_output(lib):
    B, L, H = 2, 40, 2
    qkv = torch.randn(B, L, 3 * H * 64, device="cuda").half()
    out = torch.full((B * L, H * 64 + 64), SENT, device="cuda", dtype=torch.float16)
    lo = torch.full((B * L, 2 * (H * 64 + 64)), 0x5A, device="cuda", dtype=torch.uint8)
    lse = torch.full((B, H, 64), SENT, device="cuda")
    fwd = lambda **k: capi.call("mudpt_attention_fwd_split", dtype=1, qkv=qkv, out=out, out_lo=lo, lse=lse, B=B, L=L, H=H, **k)  # noqa: E731
    refused(lib, fwd(lo_mode=1, ld_out=H * 64 - 8), "ld_out")   # rows would overlap
    refused(lib, fwd(lo_mode=1, ld_out=H * 64 + 4), "ld_out")   # 8-byte rows: not 16-byte aligned
    refused(lib, fwd(lo_mode=3, ld_out=H * 64), "lo_mode")
    refused(lib, fwd(lo_mode=0, ld_out=H * 64), "lo_mode")
    sel, q_sel = (torch.arange(B, dtype=torch.int32) * L).cuda(), qkv[:, 0, :H * 64].contiguous()
    single = lambda **k: capi.call("mudpt_attention_fwd_single_split", dtype=1, qkv=qkv, q_sel=q_sel, sel_rows=sel, out_sel=out, out_lo=lo, lse_sel=lse, B=B, L=L, H=H, **k)  # noqa: E731
    refused(lib, single(lo_mode=0, ld_out=H * 64), "lo_mode")
    refused(lib, single(lo_mode=1, ld_out=H * 64 - 8), "single query")
    dq = torch.full((B, L, 3 * H * 64), SENT, device="cuda", dtype=torch.float16)
    refused(lib, capi.call("mudpt_attention_bwd_sel", dtype=1, qkv=qkv, out=out, dout=qkv, lse=lse, delta=lse, dqkv=dq, B=B, L=L, H=H), "sel_rows")
    assert (out == SENT).all() and (lo == 0x5A).all() and (lse == SENT).all() and (dq == SENT).all()


def test_head_launchers_refuse_bad_arguments(lib):
    """The checks of mudpt_head_ex / mudpt_pair_head themselves (path, B_total < 0, training without its outputs), then those of the
    launchers behind them, which the exports leave the shape to: launch_head_fwd (e = 0), launch_head_fused_fwd (no classes),
    launch_head_fused_train (no classes; a B_total smaller than the chunk), launch_head_bwd and launch_pair_head_bwd (the same B_total,
    after their forward has run: the gradients, row losses and loss stay untouched), launch_pair_head_fwd (no classes).  Without the
    checks these launches would still be in bounds: empty loops or grids, or a different 1 / B_total."""
    B, Cn, e = 4, 5, 64
    f = lambda *shape: torch.full(shape, SENT, device="cuda")  # noqa: E731
    img, txt = torch.randn(B, e, device="cuda"), torch.randn(B * Cn, e, device="cuda")
    tn, ti, lg = f(B * Cn, e), f(B * Cn), f(B, Cn)
    loss, rl, dimg, dtxt = f(1), f(B), f(B, e), f(B * Cn, e)
    lab = torch.zeros(B, dtype=torch.int64, device="cuda")
    head = lambda path, Bt=0, C_=Cn, e_=e, train=False, lab_=None: lib.mudpt_head_ex(  # noqa: E731
        P(img), P(txt), P(lab) if train or lab_ else None, 1.0, 1.0, B, Bt, C_, e_, P(tn), P(ti), P(lg), P(loss) if train else None, P(rl) if train else None,
        P(dimg) if train else None, P(dtxt) if train else None, path, None, None)
    refused(lib, head(2), "path")
    refused(lib, head(0, Bt=-1), "head_ex")
    refused(lib, head(0, lab_=1), "training needs")
    refused(lib, head(1, e_=0), "head: bad shape")                         # launch_head_fwd
    refused(lib, head(0, C_=0), "head: bad arguments")                     # launch_head_fused_fwd
    refused(lib, head(0, C_=0, train=True), "head: bad shape")             # launch_head_fused_train
    refused(lib, head(0, Bt=B - 1, train=True), "head: B_total")           # launch_head_fused_train
    assert (tn == SENT).all() and (ti == SENT).all() and (lg == SENT).all()
    refused(lib, head(1, Bt=B - 1, train=True), "head bwd: B_total")       # launch_head_bwd, after launch_head_fwd
    assert all((t == SENT).all() for t in (loss, rl, dimg, dtxt))
    lg.fill_(SENT)
    pair = lambda Bt=0, C_=Cn, train=False, lab_=None: lib.mudpt_pair_head(P(img), P(txt), P(lab) if train or lab_ else None, 1.0, 1.0, B, Bt, C_, e, P(lg),  # noqa: E731
                                                                           P(loss) if train else None, P(rl) if train else None, P(dtxt) if train else None, None)
    refused(lib, pair(Bt=-1), "pair_head")
    refused(lib, pair(lab_=1), "training needs")
    refused(lib, pair(C_=0), "head: bad shape")                            # launch_pair_head_fwd
    assert (lg == SENT).all()
    refused(lib, pair(Bt=B - 1, train=True), "pair head bwd: B_total")     # launch_pair_head_bwd, after launch_pair_head_fwd
    assert all((t == SENT).all() for t in (loss, rl, dtxt))


def test_remaining_launchers_refuse_bad_arguments(lib):
    """launch_sgemm, launch_reduce_rows, launch_cocoop_dbias, launch_coop_dctx, launch_attn_bwd (general and sel_rows form),
    launch_attn_bwd_single and launch_attn_fwd_exact through their exports: strides shorter than a row (overlapping rows inside oversized
    buffers), empty shapes (an empty loop or grid), an unknown dtype (no kernel to launch).  Every destination keeps its sentinel."""
    f = lambda *shape: torch.full(shape, SENT, device="cuda")  # noqa: E731
    A, Bm, Cm = torch.randn(64, 64, device="cuda"), torch.randn(64, 64, device="cuda"), f(64, 64)
    sg = lambda tA=0, tB=0, M=16, N=24, K=32, lda=64, ldb=64, ldc=64: lib.mudpt_sgemm(tA, tB, M, N, K, 1.0, P(A), lda, P(Bm), ldb, 0.0, P(Cm), ldc, None, None)  # noqa: E731
    refused(lib, sg(lda=31), "sgemm: a stride")            # A [M, K]: lda < K
    refused(lib, sg(tA=1, lda=15), "sgemm: a stride")      # A [K, M]: lda < M
    refused(lib, sg(ldb=23), "sgemm: a stride")            # B [K, N]: ldb < N
    refused(lib, sg(tB=1, ldb=31), "sgemm: a stride")      # B [N, K]: ldb < K
    refused(lib, sg(ldc=23), "sgemm: a stride")            # C rows would overlap
    refused(lib, sg(K=0), "sgemm: bad arguments")
    assert (Cm == SENT).all()
    Bq, L, d = 2, 4, 16
    src, src_lp, out = torch.randn(Bq * L + 2, d, device="cuda"), torch.randn(Bq * L + 2, d, device="cuda").half(), f(4, d)
    rr = lambda dt=1, d_=d, row0=1, n=2, lp=False: lib.mudpt_reduce_rows(dt, None if lp else P(src), P(src_lp) if lp else None, Bq, L, d_, row0, n, P(out), 0, 0, 1.0, None)  # noqa: E731
    refused(lib, rr(d_=0), "reduce_rows")
    refused(lib, rr(row0=3, n=2), "reduce_rows")           # rows 3..4 of a 4-row sequence
    refused(lib, rr(dt=7, lp=True), "reduce_rows")
    assert (out == SENT).all()
    Cn = 2
    dx, dx_lp, dbias = torch.randn(Bq * Cn * L, d, device="cuda"), torch.randn(Bq * Cn * L, d, device="cuda").half(), f(Bq, d)
    db = lambda dt=1, d_=d, n=2, lp=False: lib.mudpt_cocoop_dbias(dt, None if lp else P(dx), P(dx_lp) if lp else None, P(dbias), Bq, Cn, L, d_, n, 1.0, None)  # noqa: E731
    refused(lib, db(d_=0), "cocoop_dbias")
    refused(lib, db(n=3), "cocoop_dbias")                  # 1 + n rows leave no class token in a 4-row prompt
    refused(lib, db(dt=7, lp=True), "cocoop_dbias")
    assert (dbias == SENT).all()
    n, dc = 2, 96
    rows = (torch.arange(Cn).view(Cn, 1) * L + 1 + torch.arange(n).view(1, n)).reshape(-1).to(torch.int32).cuda()
    gx, gx_lp, dctx = torch.randn(Cn * L, 128, device="cuda"), torch.randn(Cn * L, 128, device="cuda").half(), f(Cn * n, 128)
    dc_ = lambda dt=1, d_=128, lp=False, csc=0: lib.mudpt_coop_dctx(dt, None if lp else P(gx), P(gx_lp) if lp else None, P(rows), P(dctx), Cn, n, d_, csc, 1.0, None)  # noqa: E731
    refused(lib, dc_(d_=dc), "coop_dctx")                  # d % 64
    refused(lib, dc_(d_=0, csc=1), "coop_dctx")
    refused(lib, dc_(dt=7, lp=True), "coop_dctx")
    assert (dctx == SENT).all()
    B, La, H = 2, 40, 2
    Hd = H * 64
    qkv = torch.randn(B, La, 3 * Hd, device="cuda").half()
    o, lse, delta = torch.randn(B, La, Hd, device="cuda").half(), torch.zeros(B, H, 64, device="cuda"), f(B, H, 64)
    dq = torch.full((B, La, 3 * Hd), SENT, device="cuda", dtype=torch.float16)
    sel = (torch.arange(B, dtype=torch.int32) * La).cuda()
    bwd_args = dict(dtype=1, qkv=qkv, out=o, dout=o, lse=lse, delta=delta, dqkv=dq, B=B, L=La, H=H)
    for name, form in (("mudpt_attention_bwd", {}), ("mudpt_attention_bwd_sel", {"sel_rows": sel})):
        call = lambda **k: capi.call(name, **{**bwd_args, **form, **k})  # noqa: E731
        refused(lib, call(B=0), "attention: bad arguments")
        refused(lib, call(L=0), "attention: bad arguments")
        refused(lib, call(dtype=9), "unknown dtype")
    q_sel, dq_sel, lse_sel = qkv[:, 0, :Hd].contiguous(), torch.full((B, Hd), SENT, device="cuda", dtype=torch.float16), torch.zeros(B, H, device="cuda")
    b1 = lambda dt=1, B_=B: lib.mudpt_attention_bwd_single(dt, P(qkv), P(q_sel), P(sel), P(q_sel), P(q_sel), P(lse_sel), P(dq), P(dq_sel), B_, La, H, 0, None)  # noqa: E731
    refused(lib, b1(B_=0), "single query")
    refused(lib, b1(dt=9), "unknown dtype")
    assert (dq == SENT).all() and (dq_sel == SENT).all() and (delta == SENT).all()
    q32 = torch.randn(B, La, 3 * Hd, device="cuda")
    hi = torch.full((B * La + 1, Hd), SENT, device="cuda", dtype=torch.float16)
    lo, lp = hi.clone(), torch.full((B, La, 3 * Hd), SENT, device="cuda", dtype=torch.float16)
    xl = f(B, H, 64)
    fx = lambda lo_mode=1, ld=Hd, B_=B: lib.mudpt_attention_fwd_exact(P(q32), P(lp), P(hi), P(lo), lo_mode, ld, P(xl), B_, La, H, 0, None)  # noqa: E731
    refused(lib, fx(ld=Hd - 8), "ld_out")                  # rows would overlap
    refused(lib, fx(lo_mode=3), "lo_mode")
    refused(lib, fx(B_=0), "attention (exact): bad arguments")
    assert (hi == SENT).all() and (lo == SENT).all() and (lp == SENT).all() and (xl == SENT).all()
