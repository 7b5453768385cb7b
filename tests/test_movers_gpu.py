"""The data movers of elementwise.hip and coop.hip, each launcher on its own through its C-ABI test export: bit for bit against torch
indexing on the CPU (a mover rounds at most once), the two fp32 sums against float64.  Destinations are pre-filled with a sentinel so a
write outside the documented rows shows; the sizes wrap every grid-stride loop behind its block cap at least once."""
import pytest
import torch

from tests.helpers import PATCH_CASES, PATCH_SPLIT_CASES, SENT, P, e4m3_spacing, ok, refused

pytestmark = pytest.mark.gpu

DT = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16)}


@pytest.fixture(scope="module")
def lib():
    from mudpt_amd import capi
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return capi.load()


def bits(t):
    """Bit pattern of a tensor (so that -0.0 / +0.0 and NaN payloads count)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- patchify ------------------------------------------------------------------------------------------------------------------------
def patch_rows(images, p):
    """im2col of the stride-p convolution from its definition: row (b, gy, gx), inner order (c, py, px)."""
    B, _, S, _ = images.shape
    g = S // p
    return images.view(B, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * p * p)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,S,p,ldk", PATCH_CASES)
def test_patchify_plain(lib, dtype, B, S, p, ldk):
    """The vector form (p % 8 == 0, ldk = 3 p p) and the any-p form with zero-padded rows (ViT-L/14: p = 14, 588 -> 640): bit-equal to
    images.to(T) rearranged, padding columns exactly zero, nothing written behind the last row."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(S + p)
    images = torch.randn(B, 3, S, S, generator=g) * 1.3
    rows, K0 = B * (S // p) ** 2, 3 * p * p
    want = torch.zeros(rows, ldk, dtype=tt)
    want[:, :K0] = patch_rows(images, p).to(tt)
    out = torch.full((rows + 2, ldk), SENT, dtype=tt, device="cuda")
    ic = images.cuda()
    ok(lib, lib.mudpt_patchify(dt, P(ic), P(out), None, 0, B, S, p, ldk, None))
    got = out.cpu()
    assert torch.equal(bits(got[:rows]), bits(want))
    assert (got[rows:] == SENT).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("lo_mode", [1, 2])
@pytest.mark.parametrize("B,S,p,ldk", PATCH_SPLIT_CASES)
def test_patchify_split(lib, dtype, lo_mode, B, S, p, ldk):
    """The split form: hi bit-equal to the plain form; lo_mode 1: lo bit-equal to T(v - hi); lo_mode 2: the first ldk bytes of each
    2 ldk-byte row are e4m3 codes of (v - hi) * 2^12 within half an e4m3 spacing (round to nearest; |(v - hi) * 2^12| <= 2^-8 * 4096 * 6
    stays far below the 448 maximum), the second half of the row is never written.  Padding columns are zero in hi and in lo."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(S * 3 + p + lo_mode)
    images = torch.randn(B, 3, S, S, generator=g) * 1.3
    rows, K0 = B * (S // p) ** 2, 3 * p * p
    v = torch.zeros(rows, ldk)
    v[:, :K0] = patch_rows(images, p)
    hi_want = v.to(tt)
    rem = v - hi_want.float()  # exact in fp32: hi is v rounded to fewer bits
    ic = images.cuda()
    hi = torch.full((rows + 1, ldk), SENT, dtype=tt, device="cuda")
    lo = torch.full((rows + 1, ldk * 2), 0x5A, dtype=torch.uint8, device="cuda")
    ok(lib, lib.mudpt_patchify(dt, P(ic), P(hi), P(lo), lo_mode, B, S, p, ldk, None))
    hi_c, lo_c = hi.cpu(), lo.cpu()
    assert torch.equal(bits(hi_c[:rows]), bits(hi_want))
    assert (hi_c[rows:] == SENT).all() and (lo_c[rows:] == 0x5A).all()
    if lo_mode == 1:
        assert torch.equal(bits(lo_c[:rows].view(tt)), bits(rem.to(tt)))
    else:
        assert (lo_c[:rows, ldk:] == 0x5A).all(), "the second half of an e4m3 row is padding and must not be written"
        codes = lo_c[:rows, :ldk]
        assert (codes[:, K0:] == 0).all()
        s = rem.double() * 4096.0
        assert s.abs().max().item() < 448
        dec = codes.contiguous().view(torch.float8_e4m3fn).double()
        assert ((dec - s).abs() <= 0.5 * e4m3_spacing(s)).all()
        assert (dec / 4096.0 + hi_want[:, :].double() - v.double()).abs().max().item() <= (2.0 ** -4) * rem.abs().max().item() + 2.0 ** -22


# ---- row movers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,d,row0,n", [(256, 201, 768, 197, 4), (1000, 20, 512, 1, 4), (3, 7, 64, 0, 7), (2, 5, 1028, 4, 1)])
@pytest.mark.parametrize("with_add", [False, True])
def test_set_rows(lib, B, L, d, row0, n, with_add):
    """x[b, row0 + i, :] = rows[i, :] (+ add[i, :]): one fp32 add, so bit-equal to torch; every other row keeps the sentinel (d = 1028:
    more float4 than the 256 threads of a block, the inner loop wraps)."""
    g = torch.Generator().manual_seed(B + d)
    rows, add = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    x = torch.full((B + 1, L, d), SENT, device="cuda")
    rc, ac = rows.cuda(), add.cuda()
    ok(lib, lib.mudpt_set_rows(P(x), B, L, d, row0, n, P(rc), P(ac) if with_add else None, None))
    want = torch.full((B + 1, L, d), SENT)
    want[:B, row0:row0 + n] = rows + add if with_add else rows
    assert torch.equal(bits(x.cpu()), bits(want))


@pytest.mark.parametrize("nrows,total,row_bytes,src_stride,dst_stride", [(256, 256 * 201, 1536, 1536, 1536), (1000, 20000, 4608, 4608, 4608 + 64),
                                                                        (7, 40, 16, 48, 32), (33, 100, 3072, 3072 + 16, 3072)])
def test_gather_and_scatter_rows(lib, nrows, total, row_bytes, src_stride, dst_stride):
    """dst[r] = src[rows[r]] / dst[rows[r]] = src[r] for whole rows of row_bytes with byte strides wider than the row: bit-equal to torch
    indexing; the padding between rows and the rows not named keep the sentinel (4608 bytes: more 16-byte pieces than a block has threads)."""
    g = torch.Generator().manual_seed(nrows)
    idx = torch.randperm(total, generator=g)[:nrows].to(torch.int32)
    big = torch.randint(-2 ** 31, 2 ** 31 - 1, (total, src_stride // 4), generator=g, dtype=torch.int32)
    rb = row_bytes // 4
    dst = torch.full((nrows, dst_stride // 4), -7, dtype=torch.int32, device="cuda")
    bc, ic = big.cuda(), idx.cuda()
    ok(lib, lib.mudpt_gather_rows(P(bc), src_stride, P(ic), P(dst), dst_stride, nrows, row_bytes, None))
    want = torch.full((nrows, dst_stride // 4), -7, dtype=torch.int32)
    want[:, :rb] = big[idx.long(), :rb]
    assert torch.equal(dst.cpu(), want)
    # scatter: the compact rows go back to their token rows of a wider buffer
    small = torch.randint(-2 ** 31, 2 ** 31 - 1, (nrows, dst_stride // 4), generator=g, dtype=torch.int32)
    out = torch.full((total, src_stride // 4), -7, dtype=torch.int32, device="cuda")
    sc = small.cuda()
    ok(lib, lib.mudpt_scatter_rows(P(sc), dst_stride, P(ic), P(out), src_stride, nrows, row_bytes, None))
    want = torch.full((total, src_stride // 4), -7, dtype=torch.int32)
    want[idx.long(), :rb] = small[:, :rb]
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("nrows,total,d", [(256, 256 * 201, 768), (1000, 20000, 512), (5, 9, 8), (3, 11, 1032)])
def test_add_rows(lib, dtype, nrows, total, d):
    """dst[rows[r], :] += src[r, :] in T: one fp32 add and one rounding per element, so bit-equal to T(float(dst) + float(src)); rows not
    named are untouched (d = 1032: the inner loop of a 128-thread block wraps)."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(nrows + d)
    idx = torch.randperm(total, generator=g)[:nrows].to(torch.int32)
    dst0 = torch.randn(total, d, generator=g).to(tt)
    src = (torch.randn(nrows, d, generator=g) * 0.3).to(tt)
    dst, sc, ic = dst0.cuda(), src.cuda(), idx.cuda()
    ok(lib, lib.mudpt_add_rows(dt, P(sc), P(ic), P(dst), nrows, d, None))
    want = dst0.clone()
    want[idx.long()] = (dst0[idx.long()].float() + src.float()).to(tt)
    assert torch.equal(bits(dst.cpu()), bits(want))


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------
WRAP = 2048 * 256  # the block cap of launch_add / launch_cast times the block size


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 255, WRAP - 1, 2 * WRAP + 77])
def test_cast(lib, dtype, n):
    """fp32 -> T, round to nearest even: bit-equal to torch's conversion over 13 decades (fp16: overflow to inf and the subnormal range
    included), past the 2048-block cap of the grid-stride loop; the element behind the last one keeps the sentinel."""
    dt, tt = DT[dtype]
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * torch.pow(10.0, torch.randint(-7, 6, (n,), generator=g).float())
    x[::97] = 0.0
    x[1::101] = -0.0
    y = torch.full((n + 8,), SENT, dtype=tt, device="cuda")
    xc = x.cuda()
    ok(lib, lib.mudpt_cast(dt, P(xc), P(y), n, None))
    got = y.cpu()
    assert torch.equal(bits(got[:n]), bits(x.to(tt)))
    assert (got[n:] == SENT).all()


@pytest.mark.parametrize("n", [3, WRAP, 3 * WRAP + 5])
def test_add(lib, n):
    """y = a + b in fp32: a single correctly rounded add, i.e. the float64 sum rounded to fp32 (a tolerance of zero terms), past the block cap."""
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g) * 0.01
    y = torch.full((n + 4,), SENT, device="cuda")
    ac, bc = a.cuda(), b.cuda()
    ok(lib, lib.mudpt_add(P(ac), P(bc), P(y), n, None))
    got = y.cpu()
    assert torch.equal(bits(got[:n]), bits((a.double() + b.double()).float()))
    assert (got[n:] == SENT).all()


@pytest.mark.parametrize("M,N,lda", [(256, 512, 512), (256, 128, 640), (1000, 33, 40), (7, 300, 304), (1, 1, 1)])
def test_colsum(lib, M, N, lda):
    """out[n] (+)= sum_m A[m, n] over rows of stride lda > N: against a float64 sum with the fp32 bound of an M-term sum of unit-variance
    values (4e-6 sqrt(M), as test_reduce_rows); with accumulate the previous contents are added; columns N .. of the output row are untouched."""
    g = torch.Generator().manual_seed(M * N)
    A = torch.randn(M, lda, generator=g)
    ref = A[:, :N].double().sum(0)
    out = torch.full((N + 3,), SENT, device="cuda")
    Ac = A.cuda()
    ok(lib, lib.mudpt_colsum(P(Ac), M, N, lda, P(out), 0, None))
    tol = 4e-6 * M ** 0.5
    got = out.cpu()
    assert (got[:N].double() - ref).abs().max().item() <= tol
    assert (got[N:] == SENT).all()
    prev = torch.randn(N + 3, generator=g)
    out2 = prev.clone().cuda()
    ok(lib, lib.mudpt_colsum(P(Ac), M, N, lda, P(out2), 1, None))
    got2 = out2.cpu()
    assert torch.equal(bits(got2[:N]), bits(prev[:N] + got[:N]))  # the same sum, then ONE fp32 add onto the old value
    assert torch.equal(got2[N:], prev[N:])


@pytest.mark.parametrize("n", [5, 256 * 1024 + 3, 1000 * 2048])
def test_relu_and_its_backward(lib, n):
    """y = max(y, 0) in place and dy = y > 0 ? dy : 0 (meta_net, trainers/cocoop.py:103-107), with -0.0, +0.0, denormals and infinities in
    y.  Values pass through unrounded, so positives are bit-equal; the forward's zero may carry either sign (fmaxf(-0, +0) is either), so
    its zeros are compared by value.  The backward writes a literal +0 or dy itself: compared bit for bit."""
    g = torch.Generator().manual_seed(n)
    y0 = torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-41, -1e-41, float("inf")])
    y0[:5] = special[:min(5, n)]
    y = torch.cat([y0, torch.full((4,), SENT)]).cuda()
    ok(lib, lib.mudpt_relu(P(y), n, None))
    got = y.cpu()
    want = torch.where(y0 > 0, y0, torch.zeros(()))
    assert torch.equal(got[:n], want) and torch.equal(bits(got[:n][y0 > 0]), bits(y0[y0 > 0]))
    assert (got[n:] == SENT).all()
    dy0 = torch.randn(n, generator=g)
    dy = torch.cat([dy0, torch.full((4,), SENT)]).cuda()
    ok(lib, lib.mudpt_relu_bwd(P(dy), P(y), n, None))  # y now holds the forward's output: exact zeros where the input was <= 0
    gd = dy.cpu()
    assert torch.equal(bits(gd[:n]), bits(torch.where(want > 0, dy0, torch.zeros(()))))
    assert (gd[n:] == SENT).all()


# ---- prompt construction -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,L,d,n", [(64, 11, 9, 512, 4), (3, 100, 20, 512, 4), (2, 5, 7, 128, 2), (1, 2, 4, 1028, 2)])
def test_cocoop_prompts(lib, B, C, L, d, n):
    """Text-tower input of every (image, class) pair (trainers/cocoop.py:148-165, :52): the class prompt's embedding + position on every row
    except rows 1..n, which are (ctx[l - 1] + bias[i]) + pos[l] -- two fp32 adds in that order, so bit-equal to torch."""
    g = torch.Generator().manual_seed(B * C + L)
    emb_pos, ctx = torch.randn(C, L, d, generator=g), torch.randn(n, d, generator=g)
    bias, pos = torch.randn(B, d, generator=g), torch.randn(L, d, generator=g)
    want = emb_pos.unsqueeze(0).expand(B, C, L, d).clone()
    want[:, :, 1:1 + n] = ((ctx.view(1, n, d) + bias.view(B, 1, d)) + pos[1:1 + n].view(1, n, d)).unsqueeze(1)
    x0 = torch.full((B * C * L + 2, d), SENT, device="cuda")
    ec, cc, bc, pc = emb_pos.cuda(), ctx.cuda(), bias.cuda(), pos.cuda()
    ok(lib, lib.mudpt_cocoop_prompts(P(x0), P(ec), P(cc), P(bc), P(pc), B, C, L, d, n, None))
    got = x0.cpu()
    assert torch.equal(bits(got[:B * C * L]), bits(want.reshape(B * C * L, d)))
    assert (got[B * C * L:] == SENT).all()


@pytest.mark.parametrize("csc", [0, 1])
@pytest.mark.parametrize("C,n,d,L", [(11, 4, 512, 20), (1000, 16, 512, 40), (3, 2, 64, 9), (2, 1, 1028, 5)])
def test_coop_splice(lib, csc, C, n, d, L):
    """CoOp's context rows (trainers/coop.py:99-164): x[rows[c n + j]] = ctx[csc ? c : 0][j] + tpos[pos[c n + j]], the shared and the
    class-specific context, rows scattered over the sequences as the class-token position dictates: bit-equal, other rows untouched."""
    g = torch.Generator().manual_seed(C * n + csc)
    ctx = torch.randn(C if csc else 1, n, d, generator=g)
    tpos = torch.randn(L, d, generator=g)
    start = torch.randint(1, L - n, (C,), generator=g)   # where each class's context rows begin (front / middle / end differ per class)
    pos = (start.view(C, 1) + torch.arange(n).view(1, n)).reshape(-1).to(torch.int32)
    rows = (torch.arange(C).view(C, 1) * L + pos.view(C, n)).reshape(-1).to(torch.int32)
    x = torch.full((C * L, d), SENT, device="cuda")
    cc, tc, rc, pc = ctx.cuda(), tpos.cuda(), rows.cuda(), pos.cuda()
    ok(lib, lib.mudpt_coop_splice(P(x), P(cc), P(tc), P(rc), P(pc), C, n, d, csc, None))
    want = torch.full((C * L, d), SENT)
    want[rows.long()] = (ctx.expand(C, n, d).reshape(C * n, d) + tpos[pos.long()])
    assert torch.equal(bits(x.cpu()), bits(want))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_movers_refuse_bad_arguments_before_launching(lib):
    """kernels.h: every launcher validates on the host before the launch.  One bad call per mover: MUDPT_ERR_ARG, a message naming the
    launcher, and the destination untouched.  Every case is built so that a launch WITHOUT the check would still stay inside the
    (oversized) allocations or launch an empty grid: nothing here relies on a fault being caught."""
    f = lambda *shape: torch.full(shape, SENT, device="cuda")  # noqa: E731
    idx = torch.arange(8, dtype=torch.int32, device="cuda")
    x, rows = f(4, 8, 64), f(8, 64)
    refused(lib, lib.mudpt_set_rows(P(x), 2, 8, 64, 7, 2, P(rows), None, None), "set_rows")          # row0 + n > L
    refused(lib, lib.mudpt_set_rows(P(x), 2, 8, 0, 0, 2, P(rows), None, None), "set_rows")           # d = 0
    src, dst = f(16, 64), f(16, 64)
    refused(lib, lib.mudpt_gather_rows(P(src), 256, P(idx), P(dst), 256, 8, 24, None), "gather_rows")   # row_bytes % 16
    refused(lib, lib.mudpt_gather_rows(P(src), 16, P(idx), P(dst), 256, 8, 32, None), "gather_rows")    # stride < row
    refused(lib, lib.mudpt_scatter_rows(P(src), 256, P(idx), P(dst), 256, 8, 24, None), "scatter_rows")
    refused(lib, lib.mudpt_scatter_rows(P(src), 256, P(idx), P(dst), 16, 8, 32, None), "scatter_rows")
    h = torch.full((16, 64), SENT, device="cuda", dtype=torch.float16)
    refused(lib, lib.mudpt_add_rows(7, P(h), P(idx), P(h), 8, 64, None), "add_rows")                 # unknown dtype
    refused(lib, lib.mudpt_add_rows(1, P(h), P(idx), P(h), 0, 64, None), "add_rows")                 # no rows
    refused(lib, lib.mudpt_colsum(P(src), 16, 64, 63, P(dst), 0, None), "colsum")                    # lda < N
    refused(lib, lib.mudpt_add(P(src), P(src), P(dst), 0, None), "add")
    refused(lib, lib.mudpt_cast(1, P(src), P(h), 0, None), "cast")
    refused(lib, lib.mudpt_cast(5, P(src), P(h), 64, None), "cast")
    refused(lib, lib.mudpt_relu(P(dst), 0, None), "relu")
    refused(lib, lib.mudpt_relu_bwd(P(dst), P(src), 0, None), "relu_bwd")
    big = f(2 * 3 * 8, 64)
    refused(lib, lib.mudpt_cocoop_prompts(P(big), P(big), P(rows), P(rows), P(rows), 2, 3, 4, 64, 3, None), "cocoop_prompts")  # 1 + n >= L
    refused(lib, lib.mudpt_coop_splice(P(big), P(rows), P(rows), P(idx), P(idx), 2, 4, 0, 0, None), "coop_splice")          # d = 0
    refused(lib, lib.mudpt_coop_splice(P(big), P(rows), P(rows), P(idx), P(idx), 0, 4, 64, 0, None), "coop_splice")         # no classes
    img = f(2, 3, 16, 16)
    pt = torch.full((40, 192), SENT, device="cuda", dtype=torch.float16)  # room for the 2 * 9 rows a launch with S % p != 0 would write
    refused(lib, lib.mudpt_patchify(1, P(img), P(pt), None, 0, 2, 16, 8, 128, None), "patchify")     # ldk < 3 p p
    refused(lib, lib.mudpt_patchify(1, P(img), P(pt), None, 0, 2, 16, 5, 192, None), "patchify")     # S % p
    refused(lib, lib.mudpt_patchify(9, P(img), P(pt), None, 0, 2, 16, 8, 192, None), "patchify")     # unknown dtype
    pl = torch.full((40, 192), SENT, device="cuda", dtype=torch.float16)
    refused(lib, lib.mudpt_patchify(1, P(img), P(pt), P(pl), 3, 2, 16, 8, 192, None), "lo_mode")     # split form: lo_mode 1 / 2 only
    for t in (x, dst, big):
        assert (t == SENT).all()
    assert (h == SENT).all() and (pt == SENT).all() and (pl == SENT).all()
