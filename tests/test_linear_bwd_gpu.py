"""mudpt_linear_bwd on the GPU: the backward of one trained Linear y = x W^T + b in ONE launch (elementwise.hip linear_bwd_kernel) against the
three launches it replaces -- mudpt_sgemm (dW = dy^T x), mudpt_colsum (db), mudpt_sgemm (dx = dy W) -- bit for bit, and against float64 at
test_sgemm's bound (tests/test_kernels_gpu.py, tests/test_promptgen_gpu.py: 3e-5 sqrt(K) absolute, 1e-5 relative for unit-variance operands; K
is R for dW and db, `out` for dx).  Every operand sits between guard rows: NaN around the inputs, a sentinel around the outputs."""
import pytest
import torch

from tests.helpers import SENT, P, ok

pytestmark = pytest.mark.gpu
GUARD = 16  # rows of the operand's own width before and after it

# (R, out, in): one tile of everything; ragged against 16 in all three; two row tiles of dx and 12 x 4 tiles of dW; K of the dx tile (784) no
# multiple of the 8 waves' 16-k step, 49 x 12 + 12 tiles; K = 64 over 3 row tiles, `in` = 2304 = 144 column tiles (the in_proj of width 768)
SHAPES = [(1, 16, 16), (16, 24, 40), (17, 192, 64), (14, 784, 192), (33, 64, 2304)]


@pytest.fixture(scope="module")
def lib():
    from mudpt_amd import capi
    return capi.load()


def guarded(rows, cols, fill, value=None):
    """A [rows, cols] window (dense) in the middle of a buffer filled with `fill`; value: what the window holds."""
    buf = torch.full(((rows + 2 * GUARD) * cols,), fill, dtype=torch.float32, device="cuda")
    win = buf[GUARD * cols:(GUARD + rows) * cols].view(rows, cols)
    if value is not None:
        win.copy_(value)
    return buf, win


def guards_untouched(buf, rows, cols):
    return bool((buf[:GUARD * cols] == SENT).all()) and bool((buf[(GUARD + rows) * cols:] == SENT).all())


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("R,out,inn", SHAPES)
def test_linear_bwd_is_the_three_launches_bit_for_bit(lib, R, out, inn):
    g = torch.Generator().manual_seed(R * 1000003 + out * 1009 + inn)
    dy, x, W = torch.randn(R, out, generator=g), torch.randn(R, inn, generator=g), torch.randn(out, inn, generator=g)
    nan = float("nan")
    (_, dyc), (_, xc), (_, Wc) = guarded(R, out, nan, dy), guarded(R, inn, nan, x), guarded(out, inn, nan, W)  # NaN beyond R, out and in

    def fused():
        (bW, dW), (bb, db), (bx, dx) = guarded(out, inn, SENT), guarded(1, out, SENT), guarded(R, inn, SENT)
        ok(lib, lib.mudpt_linear_bwd(R, out, inn, P(dyc), P(xc), P(Wc), P(dW), P(db), P(dx), None))
        assert guards_untouched(bW, out, inn) and guards_untouched(bb, 1, out) and guards_untouched(bx, R, inn)
        return dW.clone(), db.clone().view(out), dx.clone()

    dW, db, dx = fused()
    assert not (dW == SENT).any() and not (db == SENT).any() and not (dx == SENT).any()  # every element written
    # against float64: nothing of the NaN guards arrived, and sgemm's bound holds
    for got, ref, K, tag in ((dW, dy.double().t() @ x.double(), R, "dW"), (db, dy.double().sum(0), R, "db"), (dx, dy.double() @ W.double(), out, "dx")):
        err = (got.cpu().double() - ref).abs()
        print(f"({R}, {out}, {inn}) {tag}: max err {err.max().item():.3e} against atol {3e-5 * K ** 0.5:.3e}")
        torch.testing.assert_close(got.cpu().double(), ref, atol=3e-5 * K ** 0.5, rtol=1e-5)
    # the three launches on the same buffers
    (bW, dW3), (bb, db3), (bx, dx3) = guarded(out, inn, SENT), guarded(1, out, SENT), guarded(R, inn, SENT)
    ok(lib, lib.mudpt_sgemm(1, 0, out, inn, R, 1.0, P(dyc), out, P(xc), inn, 0.0, P(dW3), inn, None, None))
    ok(lib, lib.mudpt_colsum(P(dyc), R, out, out, P(db3), 0, None))
    ok(lib, lib.mudpt_sgemm(0, 0, R, inn, out, 1.0, P(dyc), out, P(Wc), inn, 0.0, P(dx3), inn, None, None))
    assert torch.equal(bits(dW), bits(dW3)) and torch.equal(bits(db), bits(db3.view(out))) and torch.equal(bits(dx), bits(dx3))
    # a second launch: identical bits
    dW2, db2, dx2 = fused()
    assert torch.equal(bits(dW), bits(dW2)) and torch.equal(bits(db), bits(db2)) and torch.equal(bits(dx), bits(dx2))


def test_linear_bwd_refusals_leave_the_outputs_alone(lib):
    from tests.helpers import refused
    R, out, inn = 4, 8, 16
    dy, x, W = (torch.randn(s, device="cuda") for s in ((R, out), (R, inn), (out, inn)))
    dW, db, dx = (torch.full(s, SENT, device="cuda") for s in ((out, inn), (out,), (R, inn)))
    refused(lib, lib.mudpt_linear_bwd(R, out, inn, P(dy), P(x), P(W), P(dW), None, P(dx), None), "null")
    refused(lib, lib.mudpt_linear_bwd(0, out, inn, P(dy), P(x), P(W), P(dW), P(db), P(dx), None), "bad arguments")
    refused(lib, lib.mudpt_linear_bwd(R, out, inn, P(dy), P(x), P(W), P(W), P(db), P(dx), None), "aliases")
    refused(lib, lib.mudpt_linear_bwd(R, out, inn, P(dy), P(x), P(W), P(dW), P(db), P(x), None), "aliases")
    assert (dW == SENT).all() and (db == SENT).all() and (dx == SENT).all()
