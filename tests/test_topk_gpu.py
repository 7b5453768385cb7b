"""Top-k on the GPU: the kernels of mudpt_amd/csrc/topk.hip through the C ABI against their restatement on the CPU -- torch.sort(descending=True,
stable=True) in float32 for every index and rank (tests/test_topk_cpu.py holds that sort to the order's definition), the float64 softmax of the
same fp32 logits for the probabilities -- then mudpt_amd.metrics, LibraryModel.predict and DeviceClassification's opt-in on CUDA tensors.

Every logit matrix is a strided window in a NaN-filled buffer (guard rows and the gap of every row: a NaN the kernel reads would be ranked
first and would make every probability NaN), every output sits between sentinels (helpers.SENT, as an integer where the buffer holds integers).

The bound on a probability p against the float64 softmax q of the same logits, m the row maximum, every term counted at a full ulp 2^-23:
    |p - q| <= 2^-23 (|z_j - m| + ln C + chain(C) + 12) q + 1e-37
the rounding of z - m in the term (|z_j - m|) and in the sum (sum_i q_i |z_i - m| <= ln C), two expf, the additions of the stated chain, the
division; 1e-37 covers the subnormal range.  chain(C) is the kernel's longest run of terms in one lane, 4 ceil((C & ~3) / 256) + (C % 4 != 0)
(include/mudpt.h at mudpt_topk: a lane owns groups of four columns), in the place where a column-per-lane walk would have ceil(C / 64); the 6
adds of the xor tree are among the 12.  Measured on an MI355X (N(0, 8^2), 64 rows, one scaled by 10): the kernel sits at 0.310 / 0.181 / 0.194
of the bound for C = 11 / 1000 / 1003, torch's own fp32 CPU softmax at 0.295 / 0.184 / 0.190; over every row kind and shape below at 0.334 at most."""
import math

import pytest
import torch

from tests.helpers import P, SENT, ok
from tests.test_evaluator_gpu import window

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
SENT_I = int(SENT)  # no index, rank or count takes this value
EDGE = 8            # sentinel cells before and after every output
# ... 1027 | 1028: the last width whose rows the top-k kernel keeps in registers and the first it walks again round by round; 1285: that form
# with a second step of its loop and a ragged tail
N_CLS = (1, 2, 63, 64, 65, 255, 257, 1000, 1003, 1027, 1028, 1285)
ROWS = (1, 3, 4, 5, 9)  # a workgroup holds four rows
# (leading dimension, base offset in floats): ldz = C and ldz = C + 5 (the 16-byte form where that is a multiple of 4), the pointer one float off
# (always the scalar form), and a 16-byte-aligned window with ldz % 4 == 0 (always the 16-byte form; with a ragged tail at C = 1003)
LD_MODES = ("dense", "plus5", "offset", "ceil4")


def layout(C, mode):
    ceil4 = -(-C // 4) * 4
    return {"dense": (C, 0), "plus5": (C + 5, 0), "offset": (ceil4 + 4, 1), "ceil4": (ceil4 + 4, 0)}[mode]


def ks_of(C):
    return sorted({k for k in (1, 2, 5, min(C, 64)) if k <= C})


def chain(C):
    return 4 * -(-(C & ~3) // 256) + (1 if C % 4 else 0)


@pytest.fixture(scope="module")
def lib():
    from mudpt_amd import capi
    return capi.load()


def guarded(numel, dtype, fill):
    buf = torch.full((numel + 2 * EDGE,), fill, dtype=dtype, device="cuda")
    return buf, buf[EDGE:EDGE + numel]


def intact(buf, fill):
    return bool((buf[:EDGE] == fill).all()) and bool((buf[-EDGE:] == fill).all())


def run_topk(lib, win, k, value=True, prob=True):
    """one mudpt_topk launch on a window [rows, C]; (index int64, value, prob) on the host, None where not asked for"""
    rows, C = win.shape
    ibuf, index = guarded(rows * k, torch.int32, SENT_I)
    vbuf, val = guarded(rows * k, torch.float32, SENT)
    pbuf, pr = guarded(rows * k, torch.float32, SENT)
    ok(lib, lib.mudpt_topk(P(win), win.stride(0), rows, C, k, P(index), P(val) if value else None, P(pr) if prob else None, None))
    assert intact(ibuf, SENT_I) and intact(vbuf, SENT) and intact(pbuf, SENT)
    assert (value or bool((val == SENT).all())) and (prob or bool((pr == SENT).all()))
    return index.cpu().long().view(rows, k), val.cpu().view(rows, k) if value else None, pr.cpu().view(rows, k) if prob else None


def run_rank(lib, win, y, kmax, state=None, want_rank=True):
    """one mudpt_rank_accumulate launch on a fresh (or the given) zeroed state; ((state buffer, state), ranks on the host)"""
    rows, C = win.shape
    if state is None:
        sbuf, s = guarded(2 + kmax, torch.int32, SENT_I)
        s.zero_()
    else:
        sbuf, s = state
    rbuf, rank = guarded(rows, torch.int32, SENT_I)
    labels = torch.cat([torch.full((2,), 2 ** 50, dtype=torch.int64), y.to(torch.int64), torch.full((2,), 2 ** 50, dtype=torch.int64)]).cuda()[2:2 + rows]
    ok(lib, lib.mudpt_rank_accumulate(P(win), win.stride(0), P(labels), rows, C, kmax, P(s), P(rank) if want_rank else None, None))
    assert intact(sbuf, SENT_I) and intact(rbuf, SENT_I) and (want_rank or bool((rank == SENT_I).all()))
    return (sbuf, s), rank.cpu().long()


def stable_order(z):
    return torch.sort(z, dim=1, descending=True, stable=True)[1]


def inverse(order):
    place = torch.empty_like(order)
    place.scatter_(1, order, torch.arange(order.shape[1]).expand_as(order))
    return place


def expected_rank_state(z, y, kmax):
    """(state [2 + kmax], ranks [rows]) from the stable sort"""
    C = z.shape[1]
    valid = (y >= 0) & (y < C)
    rank = torch.where(valid, inverse(stable_order(z)).gather(1, y.clamp(0, C - 1).unsqueeze(1)).squeeze(1), torch.full_like(y, -1))
    hist = torch.bincount(rank[valid & (rank < kmax)], minlength=kmax)
    return torch.cat([torch.tensor([int(valid.sum()), int((~valid).sum())]), hist]), rank


def prob_fraction(p, z, index):
    """the largest |p - q| / bound over the outputs of rows whose softmax is finite (the module's docstring), and the NaN pattern held exactly"""
    C = z.shape[1]
    soft32 = torch.softmax(z, dim=1)
    nan_row = soft32.isnan().any(1)
    assert torch.equal(nan_row, z.isnan().any(1) | (z == INF).any(1) | (z == -INF).all(1))  # what torch does, stated
    assert torch.equal(p.isnan(), nan_row.unsqueeze(1).expand_as(p)), "NaN probabilities exactly on the rows where torch.softmax gives them"
    if bool(nan_row.all()):
        return 0.0
    zf, idx, pf = z[~nan_row].double(), index[~nan_row], p[~nan_row].double()
    q = torch.softmax(zf, dim=1).gather(1, idx)
    dz = (zf.gather(1, idx) - zf.max(1, keepdim=True).values).abs().clamp(max=1e4)  # -inf columns: q = 0, the bound is the 1e-37
    bound = 2.0 ** -23 * (dz + math.log(C) + chain(C) + 12) * q + 1e-37
    return ((pf - q).abs() / bound).max().item()


def row_kinds(C, g):
    """The rows the order and the softmax are about, positions collapsing at small C."""
    mid, last = C // 2, C - 1
    normal = lambda: torch.randn(C, generator=g) * 8.0  # noqa: E731
    rows = [normal(), normal(),
            torch.tensor([-1.5, 0.25, 3.0])[torch.randint(0, 3, (C,), generator=g)],  # ties everywhere
            torch.full((C,), 2.0),                                                     # all equal
            torch.tensor([0.0, -0.0, -1.0])[torch.randint(0, 3, (C,), generator=g)],   # +-0 mixes
            torch.tensor([0.0, -0.0])[torch.arange(C) % 2], torch.tensor([-0.0, 0.0])[torch.arange(C) % 2],
            torch.full((C,), -INF), torch.full((C,), NAN)]
    for cells in ({0: INF}, {last: INF, mid: INF}, {0: -INF, last: -INF}, {mid: -INF, last: INF}, {0: NAN}, {last: NAN}, {mid: NAN},
                  {0: NAN, mid: NAN, last: NAN, C // 3: INF}, {last: NAN, 0: 100.0}):
        z = normal()
        for j, v in cells.items():
            z[j] = v
        rows.append(z)
    z = torch.full((C,), -INF)  # -inf but for one column: a probability of exactly 1 and exact zeros
    z[mid] = -3.0
    rows.append(z)
    return torch.stack(rows)


@pytest.mark.parametrize("mode", LD_MODES)
@pytest.mark.parametrize("n_cls", N_CLS)
def test_topk_follows_the_stable_sort(lib, n_cls, mode):
    """Every row kind, then 1, 3, 4, 5 and 9 rows of ties, under every k: index exactly the stable sort's, value the gathered logits, prob NaN
    where torch's is and inside the bound elsewhere; index[:, 0] is mudpt_eval_accumulate's prediction on the same buffer."""
    C = n_cls
    g = torch.Generator().manual_seed(C * 1013 + LD_MODES.index(mode))
    ld, off = layout(C, mode)
    vector = off == 0 and ld % 4 == 0
    assert vector == (mode == "ceil4" or (mode == "dense" and C % 4 == 0) or (mode == "plus5" and C % 4 == 3))
    batches = [row_kinds(C, g)] + [torch.randint(-3, 4, (rows, C), generator=g).float() for rows in ROWS]
    worst = 0.0
    for z in batches:
        rows = z.shape[0]
        _, win = window(z, ld, off)
        order = stable_order(z)
        for k in ks_of(C):
            index, value, prob = run_topk(lib, win, k)
            assert torch.equal(index, order[:, :k]), (rows, k, (index != order[:, :k]).nonzero()[:4].tolist())
            want = z.gather(1, index)
            assert torch.equal(value.isnan(), want.isnan()) and torch.equal(value.nan_to_num(7.0).view(torch.int32), want.nan_to_num(7.0).view(torch.int32))
            worst = max(worst, prob_fraction(prob, z, index))
        only_index, _, _ = run_topk(lib, win, ks_of(C)[-1], value=False, prob=False)  # value and prob may be null
        assert torch.equal(only_index, order[:, :ks_of(C)[-1]])
        state = torch.zeros(lib.mudpt_eval_state_numel(C, 0), dtype=torch.int32, device="cuda")
        pred = torch.empty(rows, dtype=torch.int32, device="cuda")
        ok(lib, lib.mudpt_eval_accumulate(P(win), ld, P(torch.zeros(rows, dtype=torch.int64, device="cuda")), rows, C, P(state), 0, P(pred), None))
        assert torch.equal(pred.cpu().long(), order[:, 0])
    print(f"C {C} {mode}: worst |p - q| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("n_cls", (11, 1000, 1003))
def test_probabilities_within_the_bound(lib, n_cls):
    """64 rows of N(0, 8^2), one of them scaled by 10, all min(C, 64) places: the figure beside torch's own fp32 softmax on the CPU."""
    g = torch.Generator().manual_seed(n_cls)
    z = torch.randn(64, n_cls, generator=g) * 8.0
    z[17] *= 10.0
    k = min(n_cls, 64)
    order = stable_order(z)[:, :k]
    torchs = prob_fraction(torch.softmax(z, dim=1).gather(1, order), z, order)
    for mode in ("dense", "offset", "ceil4"):
        _, win = window(z, *layout(n_cls, mode))
        index, _, prob = run_topk(lib, win, k, value=False)
        assert torch.equal(index, order)
        f = prob_fraction(prob, z, index)
        print(f"C {n_cls} {mode}: kernel at {f:.3f} of the bound, torch's fp32 softmax at {torchs:.3f}")
        assert f <= 1.0
        assert bool((prob[:, 1:] <= prob[:, :-1]).all())  # non-increasing along the order on finite rows


@pytest.mark.parametrize("n_cls", (11, 257, 1003, 1285))
def test_a_row_gives_the_same_bits_wherever_it_lies(lib, n_cls):
    """Alone, as row 7 of a batch of 9, and under every layout (both load forms): the same index and the same prob bits."""
    g = torch.Generator().manual_seed(n_cls + 5)
    batch = torch.randn(9, n_cls, generator=g) * 8.0
    batch[7, ::3] = batch[7, 0]  # ties in the row that is followed
    k = min(n_cls, 64)
    got = []
    for mode in LD_MODES:
        for z, at in ((batch[7:8], 0), (batch, 7)):
            _, win = window(z, *layout(n_cls, mode))
            index, value, prob = run_topk(lib, win, k)
            got.append((index[at], value[at].view(torch.int32), prob[at].view(torch.int32)))
            again = run_topk(lib, win, k)  # and in a second run
            assert torch.equal(again[0], index) and torch.equal(again[2].view(torch.int32), prob.view(torch.int32))
    assert len(got) == 8 and all(torch.equal(a, b) for t in got[1:] for a, b in zip(t, got[0]))


@pytest.mark.parametrize("mode", LD_MODES)
@pytest.mark.parametrize("n_cls", N_CLS)
def test_ranks_are_the_inverse_of_the_stable_sort(lib, n_cls, mode):
    """rank = the inverse permutation at the label, hist and total exact for a small and a large kmax, labels -1 and C counted as invalid and
    in nothing else; hist[0] and total are mudpt_eval_accumulate's correct and total on the same batch."""
    C = n_cls
    g = torch.Generator().manual_seed(C * 1019 + LD_MODES.index(mode))
    ld, off = layout(C, mode)
    kinds = row_kinds(C, g)
    for z in [kinds] + [torch.randint(-3, 4, (rows, C), generator=g).float() for rows in ROWS]:
        rows = z.shape[0]
        y = torch.randint(0, C, (rows,), generator=g)
        if rows >= 4:
            y[1], y[rows - 1] = -1, C
        _, win = window(z, ld, off)
        for kmax in sorted({1, min(C, 5), 64}):
            want_state, want_rank = expected_rank_state(z, y, kmax)
            (_, s), rank = run_rank(lib, win, y, kmax)
            assert torch.equal(rank, want_rank), (rows, kmax, rank.tolist(), want_rank.tolist())
            assert torch.equal(s.cpu().long(), want_state), (rows, kmax, s.tolist(), want_state.tolist())
        ev = torch.zeros(lib.mudpt_eval_state_numel(C, 0), dtype=torch.int32, device="cuda")
        ok(lib, lib.mudpt_eval_accumulate(P(win), ld, P(y.cuda()), rows, C, P(ev), 0, None, None))
        assert ev[:3].tolist() == [int(s[0]), int(s[2]), int(s[1])]  # total, correct = hist[0], invalid
    assert int(want_state[0]) == rows - 2 and int(want_state[1]) == 2


def test_rank_accumulations_add(lib):
    """5 + 4 + 1 rows in three launches on one state give the state of one launch of 10; without `rank` nothing else is written."""
    C, kmax = 7, 4
    g = torch.Generator().manual_seed(3)
    z, y = torch.randint(-2, 3, (10, C), generator=g).float(), torch.randint(-1, C + 1, (10,), generator=g)
    want_state, want_rank = expected_rank_state(z, y, kmax)
    _, win = window(z, *layout(C, "dense"))
    (_, one), rank = run_rank(lib, win, y, kmax)
    assert torch.equal(one.cpu().long(), want_state) and torch.equal(rank, want_rank) and 0 < int(want_state[1]) < 10
    state = None
    for lo, hi in ((0, 5), (5, 9), (9, 10)):
        _, part = window(z[lo:hi], *layout(C, "offset"))
        state, _ = run_rank(lib, part, y[lo:hi], kmax, state=state, want_rank=False)
    assert torch.equal(state[1], one)


def test_metrics_on_cuda_tensors_equal_the_cpu_path():
    from mudpt_amd import metrics
    g = torch.Generator().manual_seed(9)
    z = torch.cat([torch.randn(7, 37, generator=g) * 4.0, torch.randint(-2, 3, (6, 37), generator=g).float()])
    z[3, 5] = NAN
    wide = torch.full((13, 40), NAN, device="cuda")  # a view with a longer row stride, NaN in the gap
    wide[:, :37] = z.cuda()
    for host, dev in ((z, z.cuda()), (z, wide[:, :37]), (z.half(), z.half().cuda()), (z.t()[:30], z.cuda().t()[:30])):  # the last: a column stride
        k, kmax = 5, min(host.shape[1], 30)
        yk = torch.randint(0, host.shape[1], (host.shape[0],), generator=g)
        yk[4] = -1
        index, prob, value = metrics.topk(dev, k, probabilities=True, values=True)
        want_index, want_prob, want_value = metrics.topk(host, k, probabilities=True, values=True)
        assert index.is_cuda and index.dtype == torch.int64 and prob.dtype == value.dtype == torch.float32
        assert torch.equal(index.cpu(), want_index) and torch.equal(value.cpu().nan_to_num(7.0), want_value.nan_to_num(7.0))
        assert prob_fraction(prob.cpu(), host.float(), want_index) <= 1.0
        assert torch.equal(metrics.topk(dev, 1).cpu(), want_index[:, :1])
        ranks = metrics.label_ranks(dev, yk.cuda())
        assert ranks.is_cuda and ranks.dtype == torch.int64 and torch.equal(ranks.cpu(), metrics.label_ranks(host, yk))
        got, want = metrics.compute_accuracy(dev, yk.cuda(), topk=(1, 3, kmax)), metrics.compute_accuracy(host, yk, topk=(1, 3, kmax))
        assert all(a.is_cuda and a.shape == (1,) and a.dtype == torch.float32 and a.item() == b.item() for a, b in zip(got, want)) and len(got) == 3
        top1 = metrics.compute_accuracy((dev, None), yk.cuda())[0]  # the step summary's "acc" restated
        assert top1.item() == want[0].item()
    clean = torch.randn(16, 11, generator=g)
    yc = torch.randint(0, 11, (16,), generator=g)
    acc = (clean.cuda().argmax(dim=1) == yc.cuda()).sum().float() * 100.0 / 16
    assert metrics.compute_accuracy(clean.cuda(), yc.cuda())[0].item() == acc.item()


def test_predict_on_a_frozen_and_a_coop_handle():
    from mudpt_amd.model import ModelShape
    from mudpt_amd.zsclip import FrozenCLIP
    from tests import coop_reference as CR
    from tests.test_coop_gpu import build as build_coop
    case = CR.CoopCase("coop_tiny_end")
    B = len(case.labels)
    handles = {"frozen": FrozenCLIP(ModelShape.from_config(case.cfg, 0, 1), case.frozen, case.tokens, max_batch=B, dtype="fp16"),
               "coop": build_coop(case, "fp16").eval()}
    for name, m in handles.items():
        k = min(5, m.n_cls)
        logits = m(case.images).cpu()
        prob, index = m.predict(case.images, k)
        assert tuple(prob.shape) == tuple(index.shape) == (B, k) and prob.dtype == torch.float32 and index.dtype == torch.int64 and prob.is_cuda, name
        assert torch.equal(index.cpu(), stable_order(logits)[:, :k]), name
        assert bool((prob[:, 1:] <= prob[:, :-1]).all()) and prob_fraction(prob.cpu(), logits, index.cpu()) <= 1.0, name
        if m.n_cls >= 5:
            assert torch.equal(m.predict(case.images)[1], index), name  # k defaults to 5
        m.close()


def test_hip_evaluator_with_topk_equals_the_torch_evaluator(tmp_path, capsys):
    from mudpt_amd import dassl_lite
    from mudpt_amd.evaluator import DeviceClassification
    g = torch.Generator().manual_seed(21)
    z = torch.randint(-3, 4, (12, 11), generator=g).float() + torch.randn(12, 11, generator=g).round()  # few distinct values: ties
    y = torch.randint(0, 11, (12,), generator=g)
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = str(tmp_path)
    hip, ref = (DeviceClassification(cfg, evaluator=kind, topk=(1, 5)) for kind in ("hip", "torch"))
    for lo, hi in ((0, 5), (5, 10), (10, 12)):  # the last batch is short
        hip.process(z[lo:hi].cuda(), y[lo:hi].cuda())
        ref.process(z[lo:hi], y[lo:hi])
    assert hip._rank_state.dtype == torch.int32 and hip._rank_state.is_cuda and torch.equal(hip._rank_state.cpu().long(), ref._rank_state)
    capsys.readouterr()
    rh = hip.evaluate()
    text_h = capsys.readouterr().out
    rt = ref.evaluate()
    text_t = capsys.readouterr().out
    assert list(rh) == list(rt) == ["accuracy", "error_rate", "macro_f1", "top1_accuracy", "top5_accuracy"]
    assert all(rh[k] == rt[k] for k in ("accuracy", "top1_accuracy", "top5_accuracy")) and abs(rh["macro_f1"] - rt["macro_f1"]) <= 1e-12 * abs(rt["macro_f1"])
    assert rh["top1_accuracy"] == rh["accuracy"] < rh["top5_accuracy"] and text_h == text_t and "* top5_accuracy: " in text_h
    hip.reset()
    assert int(hip._rank_state.abs().sum()) == 0
