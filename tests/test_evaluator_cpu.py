"""The test pass's evaluator without a GPU: mudpt_amd.evaluator.DeviceClassification under evaluator="torch" (the bincount restatement the GPU
tests use as their reference) against sklearn's recorded numbers (tests/golden/evaluator_sklearn.npz, written by gen_golden_evaluator.py the way
Dassl's Classification evaluator calls sklearn), Dassl's printout and protocol, and DeviceEvalLoader's host arithmetic."""
import os

import numpy as np
import pytest
import torch

from mudpt_amd import augment, dassl_lite, synth
from mudpt_amd.evaluator import DeviceClassification

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator_sklearn.npz")
CASES = ("c37", "c2", "c1", "c1000")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def make_cfg(tmp_path, per_class=False, cmat=False):
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.TEST.PER_CLASS_RESULT, cfg.TEST.COMPUTE_CMAT = per_class, cmat
    return cfg


def logits_for(pred, n_cls):
    """fp32 logits whose row maximum sits at pred"""
    z = torch.zeros(len(pred), n_cls)
    z[torch.arange(len(pred)), torch.as_tensor(pred, dtype=torch.int64)] = 1.0
    return z


def case_tensors(golden, name):
    C = int(golden[f"{name}_n_cls"])
    y, p = torch.from_numpy(golden[f"{name}_y_true"].astype(np.int64)), torch.from_numpy(golden[f"{name}_y_pred"].astype(np.int64))
    return C, y, p


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_fixture_holds_the_cases_the_evaluator_must_survive(golden):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    C, y, p = case_tensors(golden, "c37")
    assert (C, y.numel()) == (37, 500) and int(y.max()) < 30 and 5 not in p.tolist() and 31 in p.tolist() and 31 not in y.tolist()
    assert golden["c37_cmat"].shape == (golden["c37_labels"].size,) * 2 and golden["c37_cmat"].dtype == np.float64
    C, y, p = case_tensors(golden, "c1000")
    assert (C, y.numel()) == (1000, 3000) and y.unique().numel() <= 300 and "c1000_cmat" not in golden
    assert int(golden["c1_n_cls"]) == 1 and golden["c1_macro_f1"] == 100.0 and int(golden["c2_n_cls"]) == 2


@pytest.mark.parametrize("name", CASES)
def test_torch_evaluator_against_sklearn(golden, name, tmp_path):
    C, y, p = case_tensors(golden, name)
    with_cmat = f"{name}_cmat" in golden
    ev = DeviceClassification(make_cfg(tmp_path, per_class=True, cmat=with_cmat), lab2cname={i: f"n{i}" for i in range(C)}, evaluator="torch")
    ev.reset()
    ev.process(logits_for(p, C), y)
    res = ev.evaluate()
    assert list(res) == ["accuracy", "error_rate", "macro_f1", "perclass_accuracy"]
    print(f"{name}: macro_f1 {res['macro_f1']!r} against {float(golden[f'{name}_macro_f1'])!r}, perclass {res['perclass_accuracy']!r}")
    assert rel(res["macro_f1"], float(golden[f"{name}_macro_f1"])) <= 1e-12
    assert rel(res["perclass_accuracy"], float(golden[f"{name}_perclass_accuracy"])) <= 1e-12
    assert res["accuracy"] == 100.0 * int((p == y).sum()) / y.numel() and res["error_rate"] == 100.0 - res["accuracy"]
    assert ev.last["n_supported"] == y.unique().numel() and ev.last["total"] == y.numel() and ev.last["invalid"] == 0
    if with_cmat:
        cmat = torch.load(os.path.join(str(tmp_path), "cmat.pt"), weights_only=False)
        assert isinstance(cmat, np.ndarray) and cmat.dtype == np.float64 and cmat.shape == golden[f"{name}_cmat"].shape
        assert np.array_equal(cmat, golden[f"{name}_cmat"])
        sums = cmat.sum(1)
        assert set(np.round(sums, 12).tolist()) == {0.0, 1.0}  # label 31 is predicted and never true: its row stays zero
    else:
        assert not os.path.exists(os.path.join(str(tmp_path), "cmat.pt"))


def test_printout_is_dassls(tmp_path, capsys):
    """1 234 rows over three classes, the first 100 wrong: every line of Dassl's evaluator, `{:,}` included."""
    n, C = 1234, 3
    y = torch.arange(n) % C
    p = y.clone()
    p[:100] = (y[:100] + 1) % C
    ev = DeviceClassification(make_cfg(tmp_path, per_class=True), lab2cname={0: "cat", 1: "dog", 2: "tree frog"}, evaluator="torch")
    ev.process(logits_for(p, C), y)
    capsys.readouterr()
    res = ev.evaluate()
    support = [int((y == c).sum()) for c in range(C)]
    hit = [int(((y == c) & (p == c)).sum()) for c in range(C)]
    predicted = [int((p == c).sum()) for c in range(C)]
    f1 = 100.0 * sum(2.0 * hit[c] / (support[c] + predicted[c]) for c in range(C)) / C
    accs = [100.0 * hit[c] / support[c] for c in range(C)]
    assert support == [412, 411, 411] and sum(hit) == 1134
    want = ["=> result", "* total: 1,234", "* correct: 1,134", "* accuracy: 91.9%", "* error: 8.1%", f"* macro_f1: {f1:.1f}%", "=> per-class result"]
    want += [f"* class: {c} ({name})\ttotal: {support[c]:,}\tcorrect: {hit[c]:,}\tacc: {accs[c]:.1f}%" for c, name in enumerate(("cat", "dog", "tree frog"))]
    want += [f"* average: {sum(accs) / C:.1f}%"]
    assert capsys.readouterr().out.splitlines() == want
    assert rel(res["macro_f1"], f1) <= 1e-12 and rel(res["perclass_accuracy"], sum(accs) / C) <= 1e-12
    # a class without a sample has no line: Dassl lists the labels that occurred
    ev = DeviceClassification(make_cfg(tmp_path, per_class=True), lab2cname={0: "a", 1: "b", 2: "c"}, evaluator="torch")
    ev.process(logits_for([0, 2, 2, 0, 1], 3), torch.tensor([0, 2, 0, 0, 2]))
    ev.evaluate()
    lines = capsys.readouterr().out.splitlines()
    assert [l.split("\t")[0] for l in lines if l.startswith("* class")] == ["* class: 0 (a)", "* class: 2 (c)"]
    assert "* class: 0 (a)\ttotal: 3\tcorrect: 2\tacc: 66.7%" in lines and lines[-1] == f"* average: {(200.0 / 3 + 50.0) / 2:.1f}%"
    # one class, a million and more rows: the per-class line carries the separators too
    ev = DeviceClassification(make_cfg(tmp_path, per_class=True), lab2cname={0: "only"}, evaluator="torch")
    ev.process(torch.zeros(1200000, 1), torch.zeros(1200000, dtype=torch.int64))
    assert ev.evaluate()["accuracy"] == 100.0
    assert "* class: 0 (only)\ttotal: 1,200,000\tcorrect: 1,200,000\tacc: 100.0%" in capsys.readouterr().out.splitlines()


def test_protocol_two_calls_equal_one_and_reset(golden, tmp_path):
    C, y, p = case_tensors(golden, "c37")
    z = logits_for(p, C)
    cfg = make_cfg(tmp_path, cmat=True)
    one, two = DeviceClassification(cfg, evaluator="torch"), DeviceClassification(cfg, evaluator="torch")
    one.process(z, y)
    two.process(z[:123], y[:123])
    two.process(z[123:], y[123:])
    assert torch.equal(one._state, two._state) and one._state.numel() == 4 + 3 * C + C * C
    assert one.evaluate() == two.evaluate()
    head, support, predicted, hit = one.counts()
    assert head.tolist() == [500, int((p == y).sum()), 0, 0]
    assert torch.equal(support, torch.bincount(y, minlength=C)) and torch.equal(predicted, torch.bincount(p, minlength=C))
    assert torch.equal(hit, torch.bincount(y[p == y], minlength=C))
    assert torch.equal(one._state[4 + 3 * C:].view(C, C), torch.bincount(y * C + p, minlength=C * C).view(C, C))  # row = label, column = prediction
    two.reset()
    assert int(two._state.abs().sum()) == 0
    two.process(z, y)
    assert torch.equal(one._state, two._state)
    with pytest.raises(ValueError, match="36 classes"):  # another width in the same pass
        two.process(z[:, :36], y)


def test_empty_pass_gives_zeros(tmp_path, capsys):
    for processed in (False, True):
        ev = DeviceClassification(make_cfg(tmp_path, per_class=True, cmat=True), lab2cname={0: "a", 1: "b"}, evaluator="torch")
        if processed:
            ev.process(logits_for([0, 1], 2), torch.tensor([1, 1]))
            ev.reset()
        res = ev.evaluate()
        assert dict(res) == {"accuracy": 0.0, "error_rate": 0.0, "macro_f1": 0.0, "perclass_accuracy": 0.0}
        assert "* total: 0" in capsys.readouterr().out
        assert torch.load(os.path.join(str(tmp_path), "cmat.pt"), weights_only=False).shape == (0, 0)


def test_more_rows_than_int32_holds_are_refused(tmp_path):
    ev = DeviceClassification(make_cfg(tmp_path), evaluator="torch")
    z, y = logits_for([0, 1, 1, 0], 2), torch.tensor([0, 1, 0, 0])
    ev.process(z, y)
    before = ev._state.clone()
    ev._rows = 2 ** 31 - 1 - 3  # as after that many rows: three more fit, four do not
    with pytest.raises(ValueError, match="2147483647"):
        ev.process(z, y)
    assert torch.equal(ev._state, before) and ev._rows == 2 ** 31 - 4
    ev.process(z[:3], y[:3])
    assert ev._rows == 2 ** 31 - 1


def test_labels_outside_the_classes_raise_with_their_count(tmp_path):
    ev = DeviceClassification(make_cfg(tmp_path), evaluator="torch")
    ev.process(logits_for([0, 1, 2, 2, 1], 3), torch.tensor([0, -1, 2, 3, 2 ** 40]))
    head, support, predicted, hit = ev.counts()
    assert head.tolist() == [2, 2, 3, 0] and support.tolist() == [1, 0, 1] and predicted.tolist() == [1, 0, 1] and hit.tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="3 labels"):
        ev.evaluate()


def test_construction_and_the_lite_framework(tmp_path):
    cfg = dassl_lite.default_cfg()
    assert dict(cfg.TEST) == {"EVALUATOR": "Classification", "PER_CLASS_RESULT": False, "COMPUTE_CMAT": False}
    assert isinstance(dassl_lite.build_evaluator(cfg, lab2cname={0: "a"}), DeviceClassification)
    cfg.TEST.EVALUATOR = "Microf1Classification"
    with pytest.raises(KeyError, match="Microf1Classification"):
        dassl_lite.build_evaluator(cfg)
    with pytest.raises(ValueError, match="unknown evaluator"):
        DeviceClassification(cfg, evaluator="numpy")
    with pytest.raises(AssertionError):  # Dassl: the per-class table needs the names
        DeviceClassification(make_cfg(tmp_path, per_class=True))
    ev = DeviceClassification(make_cfg(tmp_path), evaluator="hip")
    with pytest.raises(RuntimeError, match="no fallback"):  # the HIP evaluator never falls back to torch
        ev.process(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    big = DeviceClassification(make_cfg(tmp_path, cmat=True), evaluator="torch")
    with pytest.raises(AssertionError, match="2\\^31"):
        big.state_numel(46341)  # 46341^2 = 2^31 + 4 ...
    assert big.state_numel(46340) == 4 + 3 * 46340 + 46340 ** 2


def test_eval_loader_arithmetic():
    images, labels = synth.synthetic_uint8_images(23, 5, seed=1, lo=8, hi=20)
    store = augment.DeviceImageStore.from_arrays(images, labels, device="cpu")
    loader = augment.DeviceEvalLoader(store, 5, 8)
    assert torch.equal(loader.params, augment.center_crop_params(store, range(23), 8)) and loader.params.dtype == torch.int32
    assert torch.equal(loader.params_dev, loader.params) and loader.params[:, 0].tolist() == list(range(23))
    ranges = loader.batch_ranges()
    assert len(loader) == len(ranges) == 5 and ranges[0] == (0, 5) and ranges[-1] == (20, 23)  # a ragged last batch, nothing dropped
    assert [i for lo, hi in ranges for i in range(lo, hi)] == list(range(23))
    assert len(augment.DeviceEvalLoader(store, 23, 8)) == 1 and len(augment.DeviceEvalLoader(store, 100, 8)) == 1
    with pytest.raises(RuntimeError, match="GPU"):  # there is no CPU form of the kernel
        next(iter(loader))
    empty = augment.DeviceImageStore.from_arrays([], [], device="cpu")
    with pytest.raises(ValueError, match="0 images"):
        augment.DeviceEvalLoader(empty, 4, 8)
    with pytest.raises(ValueError, match="batch of 0"):
        augment.DeviceEvalLoader(store, 0, 8)
