"""The linear probe on the GPU: the kernels of mudpt_amd/csrc/probe.hip against float64, the HIP evaluator against the float64 torch evaluator,
and LogisticProbe / linear_probe end to end against sklearn's recorded fits (tests/golden/probe_sklearn.npz).

GEMM bound: the project's sgemm bound -- 3e-5 sqrt(K) absolute, 1e-5 relative, unit-variance operands (tests/test_kernels_gpu.py).  Every
operand sits in a buffer of its own with a leading dimension, NaN in every element a kernel must not read (guard rows, the gap between a row's
end and the next row) and a sentinel in every element it must not write."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import SENT, P, ok, refused

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
T, S = 128, 32  # block edge and K-step of probe_gemm_kernel
GUARD = 3       # guard rows of the operand's own leading dimension before and after it
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_sklearn.npz")


@pytest.fixture(scope="module")
def lib():
    from mudpt_amd import capi
    return capi.load()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def strided(rows, cols, ld, fill, value=None):
    """A [rows, cols] window with leading dimension ld inside a buffer filled with `fill` (guard rows and the gap of every row included)."""
    buf = torch.full(((rows + 2 * GUARD) * ld,), fill, dtype=torch.float32, device="cuda")
    win = buf.view(rows + 2 * GUARD, ld)[GUARD:GUARD + rows, :cols]
    if value is not None:
        win.copy_(value)
    return buf, win


def only_window_written(buf, win, rows, cols, ld):
    """every element outside the window still holds the sentinel, every element inside was written"""
    mask = torch.ones_like(buf, dtype=torch.bool).view(rows + 2 * GUARD, ld)
    mask[GUARD:GUARD + rows, :cols] = False
    return bool((buf.view(rows + 2 * GUARD, ld)[mask] == SENT).all()) and not bool((win == SENT).any())


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_gemm_close(got, ref, K, tag):
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"{tag}: max err {err:.3e} against atol {3e-5 * K ** 0.5:.3e}")
    torch.testing.assert_close(got.double().cpu(), ref, atol=3e-5 * K ** 0.5, rtol=1e-5)


# (M, N, K, pad): pad is added to every leading dimension (0: dense; 4: longer rows that keep 16-byte alignment; odd: the scalar loads)
NT_SHAPES = [(1, 1, 1, 0), (T, T, S, 0), (T + 1, T + 2, S + 1, 0), (T + 1, T + 2, S + 1, 3), (70, 50, 77, 4), (2 * T + 5, 19, 40, 0), (300, 1000, 512, 0),
             (300, 1000, 512, 4)]


@pytest.mark.parametrize("M,N,K,pad", NT_SHAPES)
def test_gemm_nt_against_float64(lib, M, N, K, pad):
    """Z = X W^T + b: A [M, K] and B [N, K] k-contiguous, bias epilogue; one element, exactly one block, one past the block in M, two in N and
    one past the K-step at once, an odd K, strides longer than the rows (aligned and not), 1000 classes x 512 features over 300 rows."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K + pad)
    A, B, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    nan = float("nan")
    (_, Ad), (_, Bd) = strided(M, K, K + pad, nan, A), strided(N, K, K + pad, nan, B)
    biasd = torch.full((N + 2,), nan, device="cuda")
    biasd[1:N + 1] = bias.cuda()

    def run(with_bias):
        buf, C = strided(M, N, N + pad, SENT)
        ok(lib, lib.mudpt_probe_gemm_nt(M, N, K, P(Ad), K + pad, P(Bd), K + pad, P(biasd[1:]) if with_bias else None, P(C), N + pad, None))
        assert only_window_written(buf, C, M, N, N + pad)
        return C.clone()

    C = run(True)
    assert_gemm_close(C, A.double() @ B.double().t() + bias.double(), K, f"nt ({M}, {N}, {K}) pad {pad}")
    assert torch.equal(bits(C), bits(run(True)))  # a second run: identical bits
    assert_gemm_close(run(False), A.double() @ B.double().t(), K, "nt without bias")


# (M, N, Kd, pad, slices wish): the split over the depth Kd -- a depth below one slice, 1031 = 32 steps and 7 (one, four ragged, one slice per
# step, the library's choice), a depth where every slice holds exactly two steps, and dW of 1000 classes x 512 features over 300 rows
TN_SHAPES = [(1, 1, 1, 0, 0), (T, T, S, 0, 1), (T + 1, T + 2, S + 1, 0, 2), (T + 1, T + 2, S + 1, 3, 0), (19, 40, 20, 0, 4), (19, 40, 76, 4, 0),
             (33, 70, 1031, 0, 1), (33, 70, 1031, 1, 4), (33, 70, 1031, 0, 33), (33, 70, 1031, 4, 0), (65, 33, 256, 0, 4), (1000, 512, 300, 0, 0),
             (1000, 512, 300, 4, 3)]


@pytest.mark.parametrize("M,N,Kd,pad,want", TN_SHAPES)
def test_gemm_tn_against_float64(lib, M, N, Kd, pad, want):
    """dW = P^T X + beta W and db = P^T 1 in one pass: A [Kd, M], B [Kd, N] row-contiguous, the depth split into slices that a second kernel adds
    in order.  The scratch is exactly as long as the slices need, with a sentinel behind it."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + Kd + pad + want)
    A, B, W = torch.randn(Kd, M, generator=g), torch.randn(Kd, N, generator=g), torch.randn(M, N, generator=g)
    beta, nan = 0.375, float("nan")
    (_, Ad), (_, Bd), (_, Wd) = strided(Kd, M, M + pad, nan, A), strided(Kd, N, N + pad, nan, B), strided(M, N, N + pad, nan, W)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    slices = lib.mudpt_probe_gemm_tn_slices(M, N, Kd, want, ncu)
    steps = -(-Kd // S)
    assert 1 <= slices <= steps and (want == 0 or slices == -(-steps // -(-steps // min(want, steps))))
    need = slices * (M * N + M)

    def run(with_w, with_db):
        (bufC, C), (bufdb, db) = strided(M, N, N + pad, SENT), strided(1, M, M, SENT)
        scratch = torch.full((need + 64,), SENT, device="cuda")
        ok(lib, lib.mudpt_probe_gemm_tn(M, N, Kd, P(Ad), M + pad, P(Bd), N + pad, beta, P(Wd) if with_w else None, N + pad, P(C), N + pad,
                                        P(db) if with_db else None, P(scratch), need, want, None))
        assert only_window_written(bufC, C, M, N, N + pad) and bool((scratch[need:] == SENT).all())
        assert only_window_written(bufdb, db, 1, M, M) if with_db else bool((bufdb == SENT).all())
        return C.clone(), db.clone().view(M)

    C, db = run(True, True)
    ref = A.double().t() @ B.double()
    assert_gemm_close(C, ref + beta * W.double(), Kd, f"tn ({M}, {N}, {Kd}) pad {pad}, {slices} slices: dW")
    assert_gemm_close(db, A.double().sum(0), Kd, "db")
    C2, db2 = run(True, True)
    assert torch.equal(bits(C), bits(C2)) and torch.equal(bits(db), bits(db2))  # a second run: identical bits
    C3, _ = run(False, False)
    assert_gemm_close(C3, ref, Kd, "tn without W and db")


def test_gemm_refusals_leave_the_outputs_alone(lib):
    A, B, W = (torch.randn(s, device="cuda") for s in ((8, 4), (8, 6), (4, 6)))
    C, db, scratch = torch.full((4, 6), SENT, device="cuda"), torch.full((4,), SENT, device="cuda"), torch.full((64,), SENT, device="cuda")
    refused(lib, lib.mudpt_probe_gemm_tn(4, 6, 8, P(A), 4, P(B), 6, 0.0, None, 0, P(C), 6, P(db), P(scratch), 10, 2, None), "scratch")
    refused(lib, lib.mudpt_probe_gemm_tn(4, 6, 8, P(A), 3, P(B), 6, 0.0, None, 0, P(C), 6, P(db), P(scratch), 64, 0, None), "stride")
    refused(lib, lib.mudpt_probe_gemm_tn(4, 6, 8, P(A), 4, P(B), 6, 1.0, P(W), 6, P(W), 6, P(db), P(scratch), 64, 0, None), "aliases")
    refused(lib, lib.mudpt_probe_gemm_tn(4, 6, 0, P(A), 4, P(B), 6, 0.0, None, 0, P(C), 6, P(db), P(scratch), 64, 0, None), "bad sizes")
    refused(lib, lib.mudpt_probe_gemm_nt(8, 8, 4, P(A), 4, P(A), 4, None, None, 8, None), "null")
    refused(lib, lib.mudpt_probe_gemm_nt(8, 8, 4, P(A), 4, P(A), 3, None, P(C), 8, None), "stride")
    assert (C == SENT).all() and (db == SENT).all() and (scratch == SENT).all()


# ---- the row kernel ----------------------------------------------------------------------------------------------------------------------

N_CLS = [1, 2, 19, 64, 65, 1000, 1025]


def row_cases(rows, n_cls, kind, g):
    z = torch.randn(rows, n_cls, generator=g) * 3
    y = torch.randint(0, n_cls, (rows,), generator=g)
    if kind == "big":  # magnitude 90: exp overflows fp32 at 88.7 unless the maximum is subtracted first
        z = (torch.rand(rows, n_cls, generator=g) * 2 - 1) * 90
        z[0, n_cls // 2] = 90.0
        z[-1, 0] = -90.0
    if kind == "sure":  # the label's probability is 1 - 1e-17 (n_cls - 1): it rounds to 1 in fp32 and in fp64
        z = torch.randn(rows, n_cls, generator=g)
        z[torch.arange(rows), y] = 40.0
    return z, y


@pytest.mark.parametrize("kind", ["plain", "big", "sure"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n_cls", N_CLS)
def test_row_kernel_against_float64(lib, n_cls, rows, kind):
    """Per row: P = (softmax - onehot) / rows and the row loss, against float64 computed from the same fp32 logits.  Bounds, from the formats:
    a probability is exp / sum with a 1 - 2 ulp exponential, a sum whose relative error is a few eps and one division, so rows * P is good to
    16 eps32 absolute (values <= 1); a row loss is log1p of that sum plus one exact difference: 8 eps32 relative."""
    g = torch.Generator().manual_seed(n_cls * 101 + rows * 7 + len(kind))
    z, y = row_cases(rows, n_cls, kind, g)
    ld = n_cls + 3
    nan = float("nan")

    def run():
        buf, Z = strided(rows, n_cls, ld, SENT, z)
        (bl, row_loss), loss = strided(1, rows, rows, SENT), torch.full((3,), nan, dtype=torch.float64, device="cuda")
        ok(lib, lib.mudpt_probe_rows(P(Z), ld, P(y.int().cuda()), rows, n_cls, P(row_loss), P(loss[1:]), None))
        assert only_window_written(buf, Z, rows, n_cls, ld) and only_window_written(bl, row_loss, 1, rows, rows)
        assert bool(loss[0].isnan()) and bool(loss[2].isnan())
        return Z.clone(), row_loss.clone().view(rows), loss[1].clone()

    Pm, row_loss, loss_sum = run()
    z64 = z.double()
    lse = torch.logsumexp(z64, dim=1)
    ref_loss = lse - z64[torch.arange(rows), y]
    ref_P = torch.exp(z64 - lse[:, None])
    ref_P[torch.arange(rows), y] -= 1.0
    if kind == "sure":  # softmax - 1 cancels in float64 too: the label's entry is minus the sum of the others
        others = torch.exp(z64 - lse[:, None])
        others[torch.arange(rows), y] = 0.0
        ref_P[torch.arange(rows), y] = -others.sum(1)
        rest = torch.exp(z64 - 40.0)
        rest[torch.arange(rows), y] = 0.0
        ref_loss = torch.log1p(rest.sum(1))
    errP = (Pm.double().cpu() * rows - ref_P).abs().max().item()
    rel_loss = ((row_loss.double().cpu() - ref_loss).abs() / ref_loss.abs().clamp_min(1e-300)).max().item() if n_cls > 1 else float(row_loss.abs().max())
    err_sum, budget = abs(loss_sum.item() - ref_loss.sum().item()), 4 * EPS32 * ref_loss.abs().sum().item()
    print(f"n_cls {n_cls} rows {rows} {kind}: rows*P err {errP:.2e} (16 eps32 = {16 * EPS32:.2e}), row loss rel err {rel_loss / EPS32:.2f} eps32, "
          f"loss sum err {err_sum:.3e} against 4 eps32 sum|loss| = {budget:.3e}")
    assert errP <= 16 * EPS32
    assert rel_loss <= 8 * EPS32
    assert err_sum <= budget
    assert loss_sum.item() == row_loss.double().sum().item() or abs(loss_sum.item() - row_loss.double().sum().item()) <= 4 * 2.0 ** -53 * ref_loss.abs().sum().item()
    if kind == "sure" and n_cls > 1:
        assert bool((row_loss > 0).all()) and bool((Pm[torch.arange(rows), y.cuda()] < 0).all())  # neither rounds to zero
    P2, row_loss2, loss_sum2 = run()
    assert torch.equal(bits(Pm), bits(P2)) and torch.equal(bits(row_loss), bits(row_loss2)) and loss_sum.item() == loss_sum2.item()


def test_loss_sum_is_a_fixed_order_double_sum(lib):
    """700 rows (more than the summing workgroup's 256 threads, not a multiple of them): the sum of the fp32 row losses in double."""
    g = torch.Generator().manual_seed(3)
    rows, n_cls = 700, 19
    z, y = row_cases(rows, n_cls, "plain", g)
    Z, row_loss, loss = z.cuda(), torch.empty(rows, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    ok(lib, lib.mudpt_probe_rows(P(Z), n_cls, P(y.int().cuda()), rows, n_cls, P(row_loss), P(loss), None))
    ref = (torch.logsumexp(z.double(), 1) - z.double()[torch.arange(rows), y])
    assert abs(loss.item() - row_loss.double().sum().item()) <= rows * 2.0 ** -53 * row_loss.double().sum().item()
    print(f"700 rows: loss sum err {abs(loss.item() - ref.sum().item()):.3e} against {4 * EPS32 * ref.sum().item():.3e}")
    assert abs(loss.item() - ref.sum().item()) <= 4 * EPS32 * ref.abs().sum().item()


# ---- argmax ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cls", N_CLS)
def test_argmax_takes_the_lowest_index_on_ties(lib, n_cls):
    g = torch.Generator().manual_seed(n_cls)
    rows = 9
    z = torch.randn(rows, n_cls, generator=g)
    top = z.max() + 1.0
    last, mid = n_cls - 1, n_cls // 2
    z[0, 0] = top; z[0, last] = top            # a tie of the first and the last position
    z[1, mid] = top; z[1, last] = top          # middle and last
    z[2, :] = 0.25                             # all equal
    z[3, last] = top                           # the last alone
    z[4, mid:] = top                           # a run from the middle on
    z[5, 0] = -top                             # nothing special, a very low first
    want = torch.from_numpy(np.argmax(z.numpy(), axis=1))
    assert want[:5].tolist() == [0, mid, 0, last, mid]
    ld = n_cls + 1
    _, Z = strided(rows, n_cls, ld, float("nan"), z)
    pred = torch.full((rows + 2,), -7, dtype=torch.int32, device="cuda")
    ok(lib, lib.mudpt_probe_argmax(P(Z), ld, rows, n_cls, P(pred[1:]), None, None, None))
    assert pred[1:-1].cpu().tolist() == want.tolist() and pred[0].item() == pred[-1].item() == -7
    labels = want.clone().int()
    labels[::2] = (labels[::2] + 1) % max(n_cls, 2)  # rows 0, 2, 4, 6, 8 are made wrong (n_cls = 1: label 1 never matches)
    count = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    ok(lib, lib.mudpt_probe_argmax(P(Z), ld, rows, n_cls, P(pred[1:]), P(labels.cuda()), P(count[1:]), None))
    assert count.cpu().tolist() == [-7, 4, -7] and pred[1:-1].cpu().tolist() == want.tolist()
    refused(lib, lib.mudpt_probe_argmax(P(Z), ld, rows, n_cls, P(pred[1:]), P(labels.cuda()), None, None), "together")


# ---- the evaluator -----------------------------------------------------------------------------------------------------------------------

def evaluator_case(name, golden):
    if name == "fixture":
        return torch.from_numpy(golden["X"]), torch.from_numpy(golden["y"]), 19
    g = torch.Generator().manual_seed(11)
    return torch.randn(130, 33, generator=g) * 1.8, torch.randint(0, 65, (130,), generator=g), 65


@pytest.mark.parametrize("case", ["fixture", "130x65x33"])
@pytest.mark.parametrize("C", [1.0, 1e-2])
def test_hip_evaluator_against_the_float64_evaluator(golden, case, C):
    """f and g at zero and at a random point with |W| ~ 1.  Bounds: the logits carry the GEMM's 3e-5 sqrt(K) times the operands' scale (the
    features have a standard deviation of about 2), the loss is a mean of values that inherit it; the gradient is the GEMM bound over the N
    rows of P (entries <= 1 / N) times that scale, plus 16 eps32 per entry of P."""
    from mudpt_amd import lbfgs, lpclip
    X, y, n_cls = evaluator_case(case, golden)
    N, K = X.shape
    hip = lpclip.HipLogistic(X.cuda(), y.int().cuda(), n_cls, C)
    ref = lbfgs.TorchLogistic(X, y, n_cls, C)
    g = torch.Generator().manual_seed(5)
    xs = float(X.abs().max())
    for x in (torch.zeros(ref.numel(), dtype=torch.float64), torch.randn(ref.numel(), generator=g, dtype=torch.float64)):
        f_ref, g_ref = ref.value_and_grad(x)
        f, grad = hip.value_and_grad(x.cuda())
        f2, grad2 = hip.value_and_grad(x.cuda())
        assert grad.dtype == torch.float64 and grad.is_cuda and torch.equal(grad, grad2) and float(f) == float(f2)
        atol_f = 3e-5 * K ** 0.5 * 2 + 8 * EPS32 * abs(float(f_ref))
        atol_g = (3e-5 * N ** 0.5 + 16 * EPS32 * N) * xs / N
        print(f"{case} C {C} |x| {float(x.abs().max()):.1f}: f err {abs(float(f) - float(f_ref)):.3e} (atol {atol_f:.3e}), g err "
              f"{(grad.cpu() - g_ref).abs().max().item():.3e} (atol {atol_g:.3e})")
        assert abs(float(f) - float(f_ref)) <= atol_f
        torch.testing.assert_close(grad.cpu(), g_ref, atol=atol_g, rtol=1e-5)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(7))
def test_logistic_probe_against_sklearn_on_the_fixture(golden, i):
    """Per C: sklearn's iteration count; coefficients within clamp(8 d32, 16 eps32, 1e-4) max|coef| (d32: what scipy's own L-BFGS-B does on an
    fp32 numpy evaluation, recorded with the fixture; the factor 8 for a tiled, split summation order is a supposition, the measured value is
    printed); sklearn's prediction on every held-out row whose top-two margin is above 2e-4 max|coef| (|x|_1 + 1), at most 2 % left out; a
    second fit with identical bits."""
    from mudpt_amd import lpclip
    C = float(golden["C"][i])
    X, y, Xt = golden["X"], golden["y"], golden["X_test"]
    clf = lpclip.LogisticProbe(C=C).fit(X, y)
    coef, intercept = golden[f"coef_{i}"], golden[f"intercept_{i}"]
    scale = np.abs(coef).max()
    dev = max(np.abs(clf.coef_ - coef).max(), np.abs(clf.intercept_ - intercept).max()) / scale
    bound = min(max(8 * float(golden[f"d32_{i}"]), 16 * EPS32), 1e-4)
    print(f"C = {C:g}: n_iter {int(clf.n_iter_[0])} (sklearn {int(golden[f'n_iter_{i}'])}), deviation {dev:.3e} of max|coef| against {bound:.3e} "
          f"(d32 {float(golden[f'd32_{i}']):.3e}), {clf.status_}")
    assert int(clf.n_iter_[0]) == int(golden[f"n_iter_{i}"])
    assert dev <= bound
    Z = Xt.astype(np.float64) @ coef.T + intercept
    top = np.sort(Z, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 2 * 1e-4 * scale * (np.abs(Xt.astype(np.float64)).sum(1) + 1)
    left_out = 1 - keep.mean()
    print(f"          {left_out:.2%} of the held-out rows left out by the margin rule")
    assert left_out <= 0.02
    pred = clf.predict(torch.from_numpy(Xt).cuda())
    assert np.array_equal(pred[keep], golden[f"pred_{i}"][keep])
    assert clf.score(Xt, golden["y_test"]) == float(np.mean(pred == golden["y_test"]))
    # the logits follow the coefficients: a deviation of 1e-4 max|coef| per coefficient moves a logit by at most that times (|x|_1 + 1)
    assert (np.abs(clf.decision_function(Xt[:7]) - Z[:7]) <= 1e-4 * scale * (np.abs(Xt[:7].astype(np.float64)).sum(1, keepdims=True) + 1) + 1e-5).all()
    again = lpclip.LogisticProbe(C=C).fit(torch.from_numpy(X).cuda(), torch.from_numpy(y))
    assert np.array_equal(again.coef_.view(np.int64), clf.coef_.view(np.int64)) and np.array_equal(again.intercept_.view(np.int64), clf.intercept_.view(np.int64))
    assert again.n_iter_ == clf.n_iter_


def test_linear_probe_runs_the_protocol_on_the_gpu(tmp_path, monkeypatch):
    """A 5-class synthetic set through linear_probe with the real classifier: every shot count, the seven-value search and a two-round bisection
    for one seed (55 fits), both report files written in the script's formats."""
    import re
    from mudpt_amd import lpclip
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(1)
    mu = rng.standard_normal((5, 24))
    for split, n in (("train", 20), ("val", 6), ("test", 30)):
        y = np.repeat(np.array([2, 3, 5, 7, 11]), n)
        f = (mu[np.searchsorted([2, 3, 5, 7, 11], y)] + 1.2 * rng.standard_normal((len(y), 24))).astype(np.float32)
        lpclip.save_features("clip_feat", "toy", split, f, y)
    lines = []
    got = lpclip.linear_probe("toy", "toy", num_step=2, num_run=1, feature_dir="clip_feat", log=lines.append)
    details = open("report/toy/clip_feat_s2r1_details.txt").readlines()
    summary = open("report/toy/clip_feat_s2r1.txt").readlines()
    assert len(details) == 5 * 2 and len(summary) == 5
    for line, shot in zip(summary, (16, 8, 4, 2, 1)):
        assert re.fullmatch(rf"toy, {shot} Shot, Test acc stat: \d+\.\d\d \(0\.00\)\n", line), line
    for line in details:
        assert re.fullmatch(r"toy, seed 1, \d+ shot, weight [0-9.e+-]+, test_acc \d+\.\d\d\n", line), line
    assert sorted(got) == [1, 2, 4, 8, 16] and all(v.shape == (1, 2) for v in got.values())
    assert got[16][0, -1] > 60.0 > 100.0 / 5  # 16 shots of a separable toy set: far above chance
    assert float(summary[0].split("stat: ")[1].split(" ")[0]) == round(float(got[16][0, -1]), 2)
