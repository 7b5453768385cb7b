"""The test pass's evaluator on the GPU: the kernels of mudpt_amd/csrc/evaluate.hip against torch on the CPU (torch.max(z, 1)[1] for the
predictions, bincount for the counts) and sklearn's recorded numbers (tests/golden/evaluator_sklearn.npz), DeviceClassification under "hip"
against its torch restatement, DeviceEvalLoader against store.augment, and the dassl_lite plugin's test().

Every logit matrix is a strided window in a NaN-filled buffer (guard rows and the gap of every row: a NaN the kernel reads would win its row), the
state and every output sit between sentinels.  Integer results are compared exactly; the doubles within 1e-12 relative (sums of at most 1000
terms in another order: 1000 x 2^-53 = 1.1e-13)."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import P, ok, refused

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator_sklearn.npz")
GUARD = 3        # guard rows of the window's own leading dimension before and after it
EDGE = 8         # sentinel cells before and after the state and the predictions
SENT_I = -77777  # no count and no prediction takes this value
SENT_D = -1234.5
NAN, INF = float("nan"), float("inf")
N_CLS = (1, 2, 63, 64, 65, 129, 1000)
LD_MODES = ("dense", "plus1", "plus4", "ceil4", "offset")  # plus1: the scalar path; plus4 / ceil4: the vector path (ceil4: for every width, with a ragged tail)


@pytest.fixture(scope="module")
def lib():
    from mudpt_amd import capi
    return capi.load()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def layout(n_cls, mode):
    """(leading dimension, base offset in floats) of a mode"""
    ceil4 = -(-n_cls // 4) * 4
    return {"dense": (n_cls, 0), "plus1": (n_cls + 1, 0), "plus4": (n_cls + 4, 0), "ceil4": (ceil4 + 4, 0), "offset": (ceil4 + 4, 1)}[mode]


def takes_vector_path(n_cls, mode):
    ld, off = layout(n_cls, mode)
    return off == 0 and ld % 4 == 0  # torch's allocations are 16-byte aligned, and so is GUARD * ld floats further on when ld % 4 == 0


def window(z, ld, off):
    """z [rows, C] on the device as a window of leading dimension ld, `off` floats into a NaN-filled buffer"""
    rows, C = z.shape
    buf = torch.full((off + (rows + 2 * GUARD) * ld,), NAN, dtype=torch.float32, device="cuda")
    win = buf[off:].view(rows + 2 * GUARD, ld)[GUARD:GUARD + rows, :C]
    win.copy_(z)
    return buf, win


def guarded(numel, dtype=torch.int32, fill=SENT_I):
    buf = torch.full((numel + 2 * EDGE,), fill, dtype=dtype, device="cuda")
    return buf, buf[EDGE:EDGE + numel]


def edges_intact(buf, fill=SENT_I):
    return bool((buf[:EDGE] == fill).all()) and bool((buf[-EDGE:] == fill).all())


def accumulate(lib, z, y, n_cls, mode="dense", with_cmat=0, state=None, want_pred=True):
    """one launch on a fresh (or the given) state; returns (state buffer, state, predictions on the host)"""
    ld, off = layout(n_cls, mode)
    _, win = window(z, ld, off)
    rows = z.shape[0]
    if state is None:
        sbuf, s = guarded(lib.mudpt_eval_state_numel(n_cls, with_cmat))
        ok(lib, lib.mudpt_eval_reset(P(s), n_cls, with_cmat, None))
    else:
        sbuf, s = state
    pbuf, pred = guarded(rows)
    labels = torch.cat([torch.full((2,), 2 ** 50, dtype=torch.int64), y.to(torch.int64), torch.full((2,), 2 ** 50, dtype=torch.int64)]).cuda()[2:2 + rows]
    ok(lib, lib.mudpt_eval_accumulate(P(win), ld, P(labels), rows, n_cls, P(s), with_cmat, P(pred) if want_pred else None, None))
    assert edges_intact(sbuf) and edges_intact(pbuf) and (want_pred or bool((pred == SENT_I).all()))
    return (sbuf, s), pred.cpu().long()


def expected_state(z, y, n_cls, with_cmat):
    """the layout of include/mudpt.h from torch on the CPU"""
    p = torch.max(z, 1)[1]
    valid = (y >= 0) & (y < n_cls)
    yv, pv = y[valid], p[valid]
    parts = [torch.tensor([int(valid.sum()), int((pv == yv).sum()), int((~valid).sum()), 0]), torch.bincount(yv, minlength=n_cls),
             torch.bincount(pv, minlength=n_cls), torch.bincount(yv[pv == yv], minlength=n_cls)]
    if with_cmat:
        parts.append(torch.bincount(yv * n_cls + pv, minlength=n_cls * n_cls))
    return torch.cat(parts), torch.where(valid, p, torch.full_like(p, -1))


def special_rows(C, g):
    """The rows the prediction rule is about; every one on a background below its marked values.  Positions collapse at C = 1 and 2."""
    at = lambda i: min(max(i, 0), C - 1)  # noqa: E731
    rows = []

    def row(fill=None, **cells):
        z = torch.rand(C, generator=g) - 2.0 if fill is None else torch.full((C,), fill)
        for k, v in cells.items():
            z[at(int(k[1:]))] = v
        rows.append(z)
        return z
    mid, last, third = C // 2, C - 1, C // 3
    row(**{"i0": 5.0, f"i{last}": 5.0})                      # a tie of the first and the last
    row(**{f"i{mid}": 5.0, f"i{last}": 5.0})                 # ... of the middle and the last
    row(fill=2.0)                                            # all equal
    z = row()
    z[third:third + 5] = 7.0                                 # a run of equal maxima
    row(**{f"i{mid}": INF, f"i{last}": INF})                 # +inf twice
    row(fill=-INF)                                           # a row of -inf: index 0
    row(fill=-1.0, **{f"i{mid}": -0.0, f"i{last}": 0.0})     # -0 before +0: they are equal, the earlier wins
    row(fill=-1.0, **{f"i{mid}": 0.0, f"i{last}": -0.0})     # +0 before -0
    row(**{f"i{mid}": NAN})                                  # NaN alone
    row(**{f"i{third}": NAN, f"i{last}": 100.0})             # NaN before a larger finite value
    row(**{f"i{third}": 100.0, f"i{last}": NAN})             # NaN after one
    row(fill=NAN)                                            # all NaN: index 0
    row(**{f"i{mid}": INF, f"i{mid + 1}": NAN})              # NaN beside +inf, either way round
    row(**{f"i{mid}": NAN, f"i{mid + 1}": INF})
    row(**{f"i{last}": NAN, "i1": NAN})                      # two NaN: the first
    return torch.stack(rows)


def test_the_torch_rule_itself():
    """What the kernel is held to, stated once on the CPU: lowest index of the maximum, first NaN, +0 == -0, -inf -> 0."""
    z = torch.tensor([[1.0, 3.0, 3.0, 2.0], [-INF] * 4, [-1.0, -0.0, 0.0, -1.0], [-1.0, 0.0, -0.0, -1.0], [5.0, NAN, 7.0, NAN], [NAN, INF, 0.0, 0.0],
                      [INF, NAN, 0.0, 0.0], [NAN] * 4])
    assert torch.max(z, 1)[1].tolist() == [1, 0, 1, 1, 1, 0, 1, 0]


@pytest.mark.parametrize("mode", LD_MODES)
@pytest.mark.parametrize("n_cls", N_CLS)
def test_predictions_follow_torch_max_on_the_cpu(lib, n_cls, mode):
    """rows 1, 4, 5 and 9 (a workgroup holds four rows) of values drawn from a few integers, so that most rows hold ties, then the special rows;
    every width under every layout, the vector and the scalar path both."""
    g = torch.Generator().manual_seed(n_cls * 1009 + LD_MODES.index(mode))
    assert takes_vector_path(n_cls, "ceil4") and not takes_vector_path(n_cls, "offset")
    for rows in (1, 4, 5, 9):
        z = torch.randint(-3, 4, (rows, n_cls), generator=g).float()
        y = torch.randint(0, n_cls, (rows,), generator=g)
        want_state, want_pred = expected_state(z, y, n_cls, 0)
        (_, s), pred = accumulate(lib, z, y, n_cls, mode)
        assert pred.tolist() == want_pred.tolist(), (rows, pred.tolist(), want_pred.tolist())
        assert torch.equal(s.cpu().long(), want_state)
    z = special_rows(n_cls, g)
    y = torch.randint(0, n_cls, (z.shape[0],), generator=g)
    want_state, want_pred = expected_state(z, y, n_cls, 1)
    (_, s), pred = accumulate(lib, z, y, n_cls, mode, with_cmat=1)
    assert pred.tolist() == want_pred.tolist(), (pred.tolist(), want_pred.tolist())
    assert torch.equal(s.cpu().long(), want_state)


@pytest.mark.parametrize("with_cmat", (0, 1))
@pytest.mark.parametrize("n_cls,rows,mode", [(11, 64, "dense"), (65, 300, "plus4"), (1000, 257, "dense"), (37, 500, "ceil4"), (2, 9, "plus1")])
def test_every_field_of_the_state_against_bincount(lib, n_cls, rows, mode, with_cmat):
    g = torch.Generator().manual_seed(n_cls + rows + with_cmat)
    z = torch.randn(rows, n_cls, generator=g)
    y = torch.randint(0, n_cls, (rows,), generator=g)
    z[torch.arange(0, rows, 2), y[::2]] += 4.0  # about half the rows right
    want_state, want_pred = expected_state(z, y, n_cls, with_cmat)
    assert lib.mudpt_eval_state_numel(n_cls, with_cmat) == want_state.numel() == 4 + 3 * n_cls + with_cmat * n_cls * n_cls
    (_, s), pred = accumulate(lib, z, y, n_cls, mode, with_cmat)
    assert torch.equal(s.cpu().long(), want_state) and pred.tolist() == want_pred.tolist()
    assert 0 < want_state[1] < want_state[0] == rows
    (_, s2), _ = accumulate(lib, z, y, n_cls, mode, with_cmat, want_pred=False)  # a second run, without predictions: the same bits
    assert torch.equal(s, s2)


def test_launches_add_up(lib):
    """5 + 4 + 1 rows in three launches on one state give, bit for bit, the state of one launch of 10; reset zeroes it again."""
    n_cls = 7
    g = torch.Generator().manual_seed(3)
    z, y = torch.randint(-2, 3, (10, n_cls), generator=g).float(), torch.randint(0, n_cls, (10,), generator=g)
    for with_cmat in (0, 1):
        (_, one), pred = accumulate(lib, z, y, n_cls, "dense", with_cmat)
        state, parts = None, []
        for lo, hi in ((0, 5), (5, 9), (9, 10)):
            state, p = accumulate(lib, z[lo:hi], y[lo:hi], n_cls, "plus1", with_cmat, state=state)
            parts += p.tolist()
        assert torch.equal(state[1], one) and parts == pred.tolist() and int(one[0]) == 10
        ok(lib, lib.mudpt_eval_reset(P(state[1]), n_cls, with_cmat, None))
        assert int(state[1].abs().sum()) == 0 and edges_intact(state[0])


def test_labels_outside_the_classes_are_only_counted_as_invalid(lib):
    n_cls = 5
    g = torch.Generator().manual_seed(4)
    z = torch.randn(9, n_cls, generator=g)
    y = torch.tensor([0, -1, 4, n_cls, 2, 2 ** 40, 1, -2 ** 40, 3])
    want_state, want_pred = expected_state(z, y, n_cls, 1)
    assert want_state[:4].tolist()[0::2] == [5, 4] and want_pred.tolist().count(-1) == 4
    (sbuf, s), pred = accumulate(lib, z, y, n_cls, "dense", with_cmat=1)
    assert torch.equal(s.cpu().long(), want_state) and pred.tolist() == want_pred.tolist() and edges_intact(sbuf)
    only_bad = torch.tensor([-1, n_cls, 2 ** 40])
    (sbuf, s), pred = accumulate(lib, z[:3], only_bad, n_cls, "plus1", with_cmat=1)
    assert s.cpu().tolist() == [0, 0, 3, 0] + [0] * (3 * n_cls + n_cls * n_cls) and pred.tolist() == [-1, -1, -1]


def finalize(lib, s, n_cls):
    rbuf, r = guarded(6, torch.float64, SENT_D)
    ok(lib, lib.mudpt_eval_finalize(P(s), n_cls, P(r), None))
    assert edges_intact(rbuf, SENT_D)
    return r.clone()


@pytest.mark.parametrize("name", ("c37", "c2", "c1", "c1000"))
def test_finalize_against_sklearn(lib, golden, name):
    C = int(golden[f"{name}_n_cls"])
    y, p = torch.from_numpy(golden[f"{name}_y_true"].astype(np.int64)), torch.from_numpy(golden[f"{name}_y_pred"].astype(np.int64))
    z = torch.zeros(y.numel(), C)
    z[torch.arange(y.numel()), p] = 1.0
    (_, s), pred = accumulate(lib, z, y, C, "dense", with_cmat=int(name == "c37"))
    assert pred.tolist() == p.tolist()
    r = finalize(lib, s, C)
    got = r.cpu().tolist()
    f1, acc = float(golden[f"{name}_macro_f1"]), float(golden[f"{name}_perclass_accuracy"])
    print(f"{name}: macro_f1 {got[4]!r} against {f1!r}, perclass {got[5]!r} against {acc!r}")
    assert got[:4] == [float(y.numel()), float((p == y).sum()), 0.0, float(y.unique().numel())]
    assert abs(got[4] - f1) <= 1e-12 * abs(f1) and abs(got[5] - acc) <= 1e-12 * abs(acc)
    assert torch.equal(r.view(torch.int64), finalize(lib, s, C).view(torch.int64))  # two runs: the same bits
    if name == "c37":  # the matrix the evaluator saves, from the device's counts
        from mudpt_amd.evaluator import normalized_cmat
        cmat = normalized_cmat(s[4 + 3 * C:].cpu().long().view(C, C))
        assert cmat.shape == golden["c37_cmat"].shape and np.array_equal(cmat, golden["c37_cmat"])


def test_finalize_of_an_empty_state_gives_zeros(lib):
    for n_cls in (1, 300):
        sbuf, s = guarded(lib.mudpt_eval_state_numel(n_cls, 0))
        ok(lib, lib.mudpt_eval_reset(P(s), n_cls, 0, None))
        assert finalize(lib, s, n_cls).cpu().tolist() == [0.0] * 6 and edges_intact(sbuf)


def test_refusals_leave_the_outputs_alone(lib):
    n_cls, rows = 6, 4
    z, y = torch.randn(rows, n_cls, device="cuda"), torch.zeros(rows, dtype=torch.int64, device="cuda")
    sbuf, s = guarded(lib.mudpt_eval_state_numel(n_cls, 1))
    pbuf, pred = guarded(rows)
    rbuf, r = guarded(6, torch.float64, SENT_D)
    acc = lib.mudpt_eval_accumulate
    refused(lib, acc(None, n_cls, P(y), rows, n_cls, P(s), 1, P(pred), None), "null")
    refused(lib, acc(P(z), n_cls, None, rows, n_cls, P(s), 1, P(pred), None), "null")
    refused(lib, acc(P(z), n_cls, P(y), rows, n_cls, None, 1, P(pred), None), "null")
    refused(lib, acc(P(z), n_cls, P(y), 0, n_cls, P(s), 1, P(pred), None), "rows 0")
    refused(lib, acc(P(z), n_cls, P(y), rows, 0, P(s), 1, P(pred), None), "n_cls 0")
    refused(lib, acc(P(z), n_cls - 1, P(y), rows, n_cls, P(s), 1, P(pred), None), "ldz 5")
    refused(lib, acc(P(z), 46341, P(y), rows, 46341, P(s), 1, P(pred), None), "2^31")
    refused(lib, lib.mudpt_eval_reset(None, n_cls, 1, None), "null")
    refused(lib, lib.mudpt_eval_reset(P(s), 0, 1, None), "n_cls 0")
    refused(lib, lib.mudpt_eval_reset(P(s), 46341, 1, None), "2^31")
    refused(lib, lib.mudpt_eval_finalize(None, n_cls, P(r), None), "null")
    refused(lib, lib.mudpt_eval_finalize(P(s), n_cls, None, None), "null")
    refused(lib, lib.mudpt_eval_finalize(P(s), 0, P(r), None), "n_cls 0")
    assert bool((sbuf == SENT_I).all()) and bool((pbuf == SENT_I).all()) and bool((rbuf == SENT_D).all())
    assert [lib.mudpt_eval_state_numel(*a) for a in ((0, 0), (-1, 1), (46341, 1), (46340, 1), (46341, 0))] == [0, 0, 0, 4 + 3 * 46340 + 46340 ** 2, 4 + 3 * 46341]


# ---- the evaluator and the loader -------------------------------------------------------------------------------------------------------

def make_cfg(tmp_path, per_class=False, cmat=False):
    from mudpt_amd import dassl_lite
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.TEST.PER_CLASS_RESULT, cfg.TEST.COMPUTE_CMAT = per_class, cmat
    return cfg


def same_results(a, b):
    return list(a) == list(b) and all(abs(a[k] - b[k]) <= 1e-12 * abs(b[k]) for k in a)


@pytest.mark.parametrize("case", ("random", "all_wrong"))
def test_hip_evaluator_equals_the_torch_evaluator(tmp_path, case):
    from mudpt_amd.evaluator import DeviceClassification
    g = torch.Generator().manual_seed(11)
    if case == "random":
        z = torch.randn(300, 65, generator=g)
        y = torch.randint(0, 65, (300,), generator=g)
        z[torch.arange(0, 300, 3), y[::3]] += 5.0
    else:  # every sample wrong: the label's logit is the row's smallest
        z = torch.randn(64, 11, generator=g)
        y = torch.randint(0, 11, (64,), generator=g)
        z[torch.arange(64), y] = -10.0
    names = {i: f"n{i}" for i in range(z.shape[1])}
    dirs = {k: tmp_path / k for k in ("hip", "torch")}
    for d in dirs.values():
        d.mkdir()
    hip = DeviceClassification(make_cfg(dirs["hip"], True, True), lab2cname=names, evaluator="hip")
    ref = DeviceClassification(make_cfg(dirs["torch"], True, True), lab2cname=names, evaluator="torch")
    zd, yd = z.cuda(), y.cuda()
    wide = torch.full((z.shape[0], z.shape[1] + 3), NAN, device="cuda")  # the first batch: a view with a longer row stride, NaN in the gap
    wide[:, :z.shape[1]] = zd
    for lo, hi, src in ((0, 7, wide[:, :z.shape[1]]), (7, z.shape[0], zd)):
        hip.process(src[lo:hi], yd[lo:hi])
        ref.process(z[lo:hi], y[lo:hi])
    assert hip._state.dtype == torch.int32 and hip._state.is_cuda and torch.equal(hip._state.cpu().long(), ref._state)
    for a, b in zip(hip.counts(), ref.counts()):
        assert torch.equal(a, b)
    rh, rt = hip.evaluate(), ref.evaluate()
    print(case, dict(rh), dict(rt))
    assert same_results(rh, rt) and {k: hip.last[k] for k in ("total", "correct", "invalid", "n_supported")} == {k: ref.last[k] for k in ("total", "correct", "invalid", "n_supported")}
    if case == "all_wrong":
        assert rh["accuracy"] == 0.0 and rh["macro_f1"] == 0.0 and rh["perclass_accuracy"] == 0.0 and rh["error_rate"] == 100.0
    ch, ct = (torch.load(str(d / "cmat.pt"), weights_only=False) for d in (dirs["hip"], dirs["torch"]))
    assert np.array_equal(ch, ct) and ch.shape[0] == ch.shape[1] >= y.unique().numel()
    hip.reset()
    assert int(hip._state.abs().sum()) == 0 and hip.evaluate()["accuracy"] == 0.0
    with pytest.raises(ValueError, match="1 labels"):  # a label outside the classes raises in evaluate, with its count
        hip.process(zd[:2], torch.tensor([0, z.shape[1]], device="cuda"))
        hip.evaluate()
    half = DeviceClassification(make_cfg(tmp_path), evaluator="hip")  # logits that are not fp32 are widened on the device
    half.process(zd.half(), yd)
    ref16 = DeviceClassification(make_cfg(tmp_path), evaluator="torch")
    ref16.process(z.half(), y)
    assert torch.equal(half._state.cpu().long(), ref16._state)


def test_eval_loader_batches_are_the_kernels_output_for_its_rows():
    """7 synthetic images of mixed sizes at size 32 and batch 3: every batch is, bit for bit, store.augment(center_crop_params(...)) of its
    indices with the store's labels; the rows were uploaded once."""
    from mudpt_amd import augment, synth
    images, labels = synth.synthetic_uint8_images(7, 5, seed=2, lo=20, hi=70)
    assert len({tuple(im.shape) for im in images}) > 3
    store = augment.DeviceImageStore.from_arrays(images, labels, device="cuda")
    loader = augment.DeviceEvalLoader(store, 3, 32)
    assert loader.params_dev.is_cuda and len(loader) == 3
    seen = 0
    for (lo, hi), batch in zip(loader.batch_ranges(), loader):
        want = store.augment(augment.center_crop_params(store, range(lo, hi), 32), 32)
        assert batch["_mudpt_sharded"] and batch["img"].is_cuda and tuple(batch["img"].shape) == (hi - lo, 3, 32, 32)
        assert torch.equal(batch["img"].view(torch.int32), want.view(torch.int32))
        assert torch.equal(batch["label"], store.labels[lo:hi]) and batch["label"].dtype == torch.int64
        seen += hi - lo
    assert seen == 7 and torch.equal(torch.cat([b["label"] for b in loader]).cpu(), torch.as_tensor(labels, dtype=torch.int64))


def test_plugin_test_pass(tmp_path, monkeypatch, capsys):
    """dassl_lite's MuDPT trainer, the tiny configuration of test_trainer_gpu.py: test() drives the evaluator, returns the accuracy of a manual
    model_inference loop and prints Dassl's lines; with device_test_store set the pass runs over the DeviceEvalLoader."""
    from mudpt_amd import augment, dassl_lite, trainer  # noqa: F401
    from mudpt_amd.evaluator import DeviceClassification
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_DEVICE_TEST", "MUDPT_DEVICE_DATA"):
        monkeypatch.delenv(var, raising=False)
    cfg = make_cfg(tmp_path, per_class=True, cmat=True)
    cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 8, 10
    cfg.DATALOADER.TEST.BATCH_SIZE = 4
    cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH = 4, 12
    cfg.INPUT.TRANSFORMS, cfg.INPUT.INTERPOLATION = ("random_resized_crop", "random_flip", "normalize"), "bicubic"
    t = dassl_lite.build_trainer(cfg)
    assert isinstance(t.evaluator, DeviceClassification) and isinstance(t.test_loader, list)

    def by_hand(loader):
        ref = DeviceClassification(make_cfg(tmp_path, per_class=True), lab2cname=t.lab2cname, evaluator="torch")
        t.set_model_mode("eval")
        correct = total = 0
        with torch.no_grad():
            for batch in loader:
                x, y = t.parse_batch_test(batch)
                logits = t.model_inference(x)
                correct += int((logits.argmax(dim=1) == y).sum())
                total += int(y.numel())
                ref.process(logits.cpu(), y.cpu())
        return 100.0 * correct / total, total, ref

    def run_test():
        capsys.readouterr()
        acc = t.test()
        return acc, capsys.readouterr().out.splitlines()

    want_acc, total, ref = by_hand(t.test_loader)
    acc, lines = run_test()
    want = ref.evaluate()
    capsys.readouterr()
    assert total == 8 and acc == want_acc == want["accuracy"]  # two whole batches of 4 (the lite data manager drops the ragged tail)
    assert lines[:4] == ["=> result", f"* total: {total}", f"* correct: {ref.last['correct']}", f"* accuracy: {acc:.1f}%"]
    assert lines[4] == f"* error: {100.0 - acc:.1f}%" and lines[5] == f"* macro_f1: {want['macro_f1']:.1f}%"
    assert t.evaluator._kind == "hip" and all(torch.equal(a, b) for a, b in zip(t.evaluator.counts(), ref.counts()))
    assert abs(t.evaluator.last["macro_f1"] - want["macro_f1"]) <= 1e-12 * abs(want["macro_f1"])
    # the per-class table and the matrix
    assert "=> per-class result" in lines and lines[-2].startswith("* average: ") and lines[-1].startswith("Confusion matrix is saved to ")
    support = ref.counts()[1].tolist()
    assert [l.split("\t")[0] for l in lines if l.startswith("* class: ")] == [f"* class: {c} ({t.lab2cname[c]})" for c in range(11) if support[c] > 0]
    cmat = torch.load(str(tmp_path / "cmat.pt"), weights_only=False)
    used = sum(1 for s, p in zip(support, ref.counts()[2].tolist()) if s > 0 or p > 0)
    assert cmat.shape == (used, used) and cmat.dtype == np.float64 and set(np.round(cmat.sum(1), 12).tolist()) <= {0.0, 1.0} and cmat.sum() > 0
    # the device-resident test pass: all 10 images of the synthetic uint8 test set, in three batches
    t.device_test_store = t.dm.uint8_test_store("cuda:0")
    acc, lines = run_test()
    assert isinstance(t.test_loader, augment.DeviceEvalLoader) and len(t.test_loader) == 3 and lines[0].startswith("Device-resident test data: 10 images")
    want_acc, total, ref = by_hand(t.test_loader)
    assert total == 10 and acc == want_acc and all(torch.equal(a, b) for a, b in zip(t.evaluator.counts(), ref.counts()))
    assert f"* total: {total}" in lines and f"* correct: {int(ref.counts()[0][1])}" in lines
    # another interpolation: refused with a note, the loader in place stays
    t.test_loader = t.dm.test_loader
    t.cfg.INPUT.INTERPOLATION = "bilinear"
    assert trainer.device_test_loader(t, t.test_loader, 0) is None and "refused" in capsys.readouterr().out
    t.cfg.INPUT.INTERPOLATION = "bicubic"
    with monkeypatch.context() as m:  # ... and a store over a quarter of the free device memory
        m.setattr(torch.cuda, "mem_get_info", lambda *a: (400000, 10 ** 9))
        del t.device_test_store
        assert trainer.device_test_loader(t, t.test_loader, 0) is None and not hasattr(t, "device_test_store")
    t.model.close()
