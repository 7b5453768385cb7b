"""No-GPU checks of top-k on the device (mudpt_amd/csrc/topk.hip, mudpt_amd/metrics.py): the two exports and their host refusals, metrics on CPU
tensors against a plain Python loop over the order's definition (the third statement of the order, independent of the stable sort and of the
kernel), Dassl's compute_accuracy contract, and DeviceClassification's opt-in top-k accuracy under the "torch" kind."""
import ctypes as C
import math
import os

import pytest
import torch

from mudpt_amd import build, capi, dassl_lite

NAN, INF = float("nan"), float("inf")
# the rows the order is about: NaN twice among ties, signed zeros and +inf; the row on which torch.topk answers [7, 6, 1]; all equal; all NaN
ROWS = [[1.0, NAN, 3.0, 3.0, -0.0, 0.0, NAN, INF], [0.0, -0.0, 0.0, -0.0, -INF, -INF, 1.0, 1.0], [2.5] * 8, [NAN] * 8]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


def precedes(z, a, b):
    """The order's definition (include/mudpt.h at mudpt_topk), word for word."""
    if math.isnan(z[a]):
        return not math.isnan(z[b]) or a < b
    return not math.isnan(z[b]) and (z[a] > z[b] or (z[a] == z[b] and a < b))


def loop_ranks(row):
    """rank of every column = the number of columns that precede it; a total order gives every rank once"""
    n = len(row)
    ranks = [sum(precedes(row, a, b) for a in range(n) if a != b) for b in range(n)]
    assert sorted(ranks) == list(range(n))
    return ranks


def loop_order(row):
    ranks = loop_ranks(row)
    return sorted(range(len(row)), key=ranks.__getitem__)


def make_cfg(tmp_path):
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = str(tmp_path)
    return cfg


def test_exports_and_abi_version(lib):
    for name in ("mudpt_topk", "mudpt_rank_accumulate"):
        assert name in capi.declared_functions() and hasattr(lib, name)
    assert [n for n, _ in capi.DECLARATIONS["mudpt_topk"][1]] == ["logits", "ldz", "rows", "n_cls", "k", "index", "value", "prob", "stream"]
    assert [n for n, _ in capi.DECLARATIONS["mudpt_rank_accumulate"][1]] == ["logits", "ldz", "labels", "rows", "n_cls", "kmax", "state", "rank", "stream"]
    assert lib.mudpt_abi_version() == capi.ABI_VERSION == 7


def test_refusals_on_the_host(lib):
    """Every check answers MUDPT_ERR_ARG with a message that names the argument, before any GPU call: the buffers are host memory that no
    kernel could use, and nothing is read from them."""
    z, y, out = torch.zeros(4 * 100), torch.zeros(4, dtype=torch.int64), torch.zeros(4 * 64, dtype=torch.int32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def refused(rc, *words):
        msg = lib.mudpt_last_error().decode()
        assert rc == 1 and all(w in msg for w in words), (rc, msg, words)

    def topk(logits=z, ldz=100, rows=4, n_cls=100, k=5, index=out):
        return lib.mudpt_topk(p(logits), ldz, rows, n_cls, k, p(index), None, None, None)

    def rank(logits=z, ldz=100, labels=y, rows=4, n_cls=100, kmax=5, state=out):
        return lib.mudpt_rank_accumulate(p(logits), ldz, p(labels), rows, n_cls, kmax, p(state), None, None)

    refused(topk(logits=None), "topk", "null logits")
    refused(topk(index=None), "topk", "null index")
    refused(rank(logits=None), "rank_accumulate", "null logits")
    refused(rank(labels=None), "rank_accumulate", "null labels")
    refused(rank(state=None), "rank_accumulate", "null state")
    for call, what in ((topk, "topk"), (rank, "rank_accumulate")):
        refused(call(rows=0), what, "rows 0")
        refused(call(rows=-3), what, "rows -3")
        refused(call(n_cls=0, ldz=0), what, "n_cls 0")
        refused(call(ldz=99), what, "ldz 99")
    refused(topk(k=0), "k 0")
    refused(topk(k=-1), "k -1")
    refused(topk(k=65), "k 65")
    refused(topk(k=6, n_cls=5), "k 6", "n_cls 5")
    refused(topk(k=64, n_cls=63, ldz=64), "k 64", "n_cls 63")
    refused(rank(kmax=0), "kmax 0")
    refused(rank(kmax=65), "kmax 65")
    assert int(out.abs().sum()) == 0
    assert capi.call("mudpt_topk") == 1 and capi.call("mudpt_rank_accumulate") == 1  # omitted pointers are null


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64, torch.float16))
def test_metrics_on_cpu_tensors_follow_the_loop(dtype):
    from mudpt_amd import metrics
    z = torch.tensor(ROWS, dtype=dtype)
    want = [loop_order(r) for r in ROWS]
    # the three statements of the order agree: the loop, the CPU's stable sort (the GPU tests' reference), the definition worked by hand
    assert torch.sort(z.float(), dim=1, descending=True, stable=True)[1].tolist() == want
    assert want[0] == [1, 6, 7, 2, 3, 0, 4, 5] and want[1][:3] == [6, 7, 0]  # (torch.topk answers [7, 6, 1] on the second row)
    soft = torch.softmax(z.float(), dim=1)
    for k in (1, 3, 8):
        index = metrics.topk(z, k)
        assert index.dtype == torch.int64 and index.shape == (4, k) and index.tolist() == [w[:k] for w in want]
        index2, prob, value = metrics.topk(z, k, probabilities=True, values=True)
        assert torch.equal(index2, index) and prob.dtype == value.dtype == torch.float32 and prob.shape == value.shape == (4, k)
        assert torch.equal(value.isnan(), z.float().gather(1, index).isnan()) and torch.equal(value.nan_to_num(7.0), z.float().gather(1, index).nan_to_num(7.0))
        assert torch.equal(prob.isnan(), soft.gather(1, index).isnan()) and torch.equal(prob.nan_to_num(7.0), soft.gather(1, index).nan_to_num(7.0))
        _, only_value = metrics.topk(z, k, values=True)
        assert torch.equal(only_value.nan_to_num(7.0), value.nan_to_num(7.0))
    assert prob[0].isnan().all() and prob[3].isnan().all() and not prob[1].isnan().any() and torch.equal(prob[2], torch.full((8,), 0.125))
    ranks = [loop_ranks(r) for r in ROWS]
    for y in range(8):
        assert metrics.label_ranks(z, torch.full((4,), y)).tolist() == [r[y] for r in ranks]
    got = metrics.label_ranks(z, torch.tensor([-1, 8, 2 ** 40, 5]))
    assert got.dtype == torch.int64 and got.tolist() == [-1, -1, -1, ranks[3][5]]
    one = torch.tensor([[3.0], [NAN], [-INF]], dtype=dtype)  # C = 1
    index, prob = metrics.topk(one, 1, probabilities=True)
    assert index.tolist() == [[0]] * 3 and prob[0].item() == 1.0 and prob[1:].isnan().all()
    assert metrics.label_ranks(one, torch.tensor([0, 0, 1])).tolist() == [0, 0, -1]
    for bad, word in ((0, "k = 0"), (65, "k = 65"), (9, "k = 9 is more than the 8 classes")):
        with pytest.raises(ValueError, match=word):
            metrics.topk(z, bad)
    with pytest.raises(ValueError, match=r"not \[B, C\]"):
        metrics.topk(z[0], 1)


def test_compute_accuracy_keeps_dassls_contract():
    from mudpt_amd import metrics
    g = torch.Generator().manual_seed(0)
    z = torch.randn(16, 11, generator=g)
    y = torch.randint(0, 11, (16,), generator=g)
    z[torch.arange(0, 16, 3), y[::3]] += 6.0
    res = metrics.compute_accuracy(z, y, topk=(1, 5, 11))
    assert isinstance(res, list) and len(res) == 3 and all(r.shape == (1,) and r.dtype == torch.float32 and r.device == z.device for r in res)
    ranks = [loop_ranks(r)[int(t)] for r, t in zip(z.tolist(), y.tolist())]
    assert [r.item() for r in res] == [100.0 * sum(n < k for n in ranks) / 16 for k in (1, 5, 11)]
    assert 0.0 < res[0].item() < res[1].item() < res[2].item() == 100.0
    (top1,) = metrics.compute_accuracy(z, y)  # the default: topk = (1,), what trainer.py's "acc" restates
    assert top1.item() == (100 * (z.max(1)[1] == y).float().mean()).item() == res[0].item()
    for wrapped in ((z, "features"), [z, None]):  # a tuple or list whose first item is the logits
        assert metrics.compute_accuracy(wrapped, y, topk=(5,))[0].item() == res[1].item()
    odd = metrics.compute_accuracy(z[:7], y[:7], topk=(1,))[0].item()  # a batch size that 100 is no multiple of
    assert odd == pytest.approx(100.0 * sum(n < 1 for n in ranks[:7]) / 7, rel=1e-6)
    assert metrics.compute_accuracy(z, torch.full((16,), -1), topk=(11,))[0].item() == 0.0  # a label outside the classes is among nothing
    ties = torch.tensor(ROWS)  # the order decides ties: the label at rank 2 of row 1 is column 0
    assert [r.item() for r in metrics.compute_accuracy(ties, torch.tensor([2, 0, 7, 3]), topk=(3, 4, 8))] == [25.0, 75.0, 100.0]
    for bad, word in (((65,), "k = 65"), ((1, 12), "k = 12"), ((0, 1), "k = 0"), ((), "empty")):
        with pytest.raises(ValueError, match=word):
            metrics.compute_accuracy(z, y, topk=bad)


def run(ev, z, y, capsys, batches=((0, 5), (5, 12))):
    capsys.readouterr()
    for lo, hi in batches:
        ev.process(z[lo:hi], y[lo:hi])
    results = ev.evaluate()
    return results, capsys.readouterr().out


def test_evaluator_opt_in(tmp_path, capsys, monkeypatch):
    from mudpt_amd.evaluator import DeviceClassification
    g = torch.Generator().manual_seed(1)
    z = torch.randint(-2, 3, (12, 6), generator=g).float()  # ties in most rows
    y = torch.randint(0, 6, (12,), generator=g)
    names = {i: f"n{i}" for i in range(6)}
    plain, text = run(DeviceClassification(make_cfg(tmp_path), lab2cname=names, evaluator="torch"), z, y, capsys)
    empty, text_empty = run(DeviceClassification(make_cfg(tmp_path), lab2cname=names, evaluator="torch", topk=()), z, y, capsys)
    assert text_empty == text and list(empty.items()) == list(plain.items()) and list(plain) == ["accuracy", "error_rate", "macro_f1"]
    assert text.splitlines()[0] == "=> result" and text.splitlines()[-1].startswith("* macro_f1: ") and "top" not in text
    ev = DeviceClassification(make_cfg(tmp_path), lab2cname=names, evaluator="torch", topk=(1, 3))
    with_k, text_k = run(ev, z, y, capsys)
    assert list(with_k) == ["accuracy", "error_rate", "macro_f1", "top1_accuracy", "top3_accuracy"]
    assert all(with_k[k] == plain[k] for k in plain) and with_k["top1_accuracy"] == with_k["accuracy"]
    ranks = [loop_ranks(r)[int(t)] for r, t in zip(z.tolist(), y.tolist())]
    assert with_k["top3_accuracy"] == 100.0 * sum(n < 3 for n in ranks) / 12 and with_k["top1_accuracy"] < with_k["top3_accuracy"] < 100.0
    assert text_k.splitlines() == text.splitlines() + [f"* top1_accuracy: {with_k['top1_accuracy']:.1f}%", f"* top3_accuracy: {with_k['top3_accuracy']:.1f}%"]
    assert not any(line.startswith("* accuracy:") for line in text_k.splitlines()[-2:])  # the pattern parse scripts look for matches one line
    ev.reset()  # the rank state is zeroed with the other
    again, _ = run(ev, z, y, capsys, batches=((0, 12),))
    assert list(again.items()) == list(with_k.items())
    none, text_none = run(DeviceClassification(make_cfg(tmp_path), lab2cname=names, evaluator="torch", topk=(2,)), z, y, capsys, batches=())
    assert none["top2_accuracy"] == 0.0 and "* top2_accuracy: 0.0%" in text_none  # no batch at all: zeros, never NaN
    # a k above the class count is refused at construction; without class names, by the first batch
    with pytest.raises(ValueError, match="k = 7 is more than the 6 classes"):
        DeviceClassification(make_cfg(tmp_path), lab2cname=names, evaluator="torch", topk=(1, 7))
    with pytest.raises(ValueError, match="1 .. 64"):
        DeviceClassification(make_cfg(tmp_path), evaluator="torch", topk=(0,))
    late = DeviceClassification(make_cfg(tmp_path), evaluator="torch", topk=(7,))
    with pytest.raises(ValueError, match="k = 7 is more than the 6 classes"):
        late.process(z, y)
    # a rank state that disagrees with the evaluator's is a bug, and evaluate says so
    ev._rank_state[2] += 1
    with pytest.raises(RuntimeError, match="rank 0"):
        ev.evaluate()
    # the lite framework's switch
    monkeypatch.delenv("MUDPT_TEST_TOPK", raising=False)
    assert dassl_lite.build_evaluator(make_cfg(tmp_path), lab2cname=names)._topk == ()
    for wish, want in (("5", (5,)), ("3,5", (3, 5)), (" 1, 2 ", (1, 2))):
        monkeypatch.setenv("MUDPT_TEST_TOPK", wish)
        assert dassl_lite.build_evaluator(make_cfg(tmp_path), lab2cname=names)._topk == want
    monkeypatch.setenv("MUDPT_TEST_TOPK", "five")
    with pytest.raises(ValueError, match="MUDPT_TEST_TOPK"):
        dassl_lite.build_evaluator(make_cfg(tmp_path), lab2cname=names)
    monkeypatch.setenv("MUDPT_TEST_TOPK", "9")
    with pytest.raises(ValueError, match="k = 9 is more than the 6 classes"):
        dassl_lite.build_evaluator(make_cfg(tmp_path), lab2cname=names)
