"""The linear probe without a GPU: the L-BFGS driver (mudpt_amd/lbfgs.py) with its float64 torch evaluator against sklearn's recorded fits
(tests/golden/probe_sklearn.npz), the line search on two textbook functions, the protocol of mudpt_amd.lpclip.linear_probe against the
script's arithmetic written out again here, and the argument checks of LogisticProbe."""
import os

import numpy as np
import pytest
import torch

from mudpt_amd import lbfgs, lpclip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_sklearn.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_driver_reproduces_sklearn_on_the_fixture(golden):
    """float64 against float64: the same iteration count for all seven C, coefficients and intercepts within 1e-6 max|coef|."""
    X, y = torch.from_numpy(golden["X"]), torch.from_numpy(golden["y"])
    n_cls, K = 19, X.shape[1]
    for i, C in enumerate(golden["C"]):
        ev = lbfgs.TorchLogistic(X, y, n_cls, float(C))
        res = lbfgs.minimize(ev, torch.zeros(ev.numel(), dtype=torch.float64))
        coef, intercept = res.x[:n_cls * K].view(n_cls, K).numpy(), res.x[n_cls * K:].numpy()
        scale = np.abs(golden[f"coef_{i}"]).max()
        dev = max(np.abs(coef - golden[f"coef_{i}"]).max(), np.abs(intercept - golden[f"intercept_{i}"]).max()) / scale
        print(f"C = {float(C):g}: n_iter {res.n_iter} (sklearn {int(golden[f'n_iter_{i}'])}), {res.n_eval} evaluations, deviation {dev:.2e} of max|coef|, {res.message}")
        assert res.n_iter == int(golden[f"n_iter_{i}"]) and res.converged
        assert dev <= 1e-6


def test_logistic_probe_float64_matches_sklearn_predictions(golden):
    clf = lpclip.LogisticProbe(C=1.0, evaluator="torch64", device="cpu").fit(golden["X"], golden["y"])
    assert clf.n_iter_.tolist() == [int(golden["n_iter_3"])] and clf.coef_.shape == (19, 40) and clf.intercept_.shape == (19,)
    assert np.array_equal(clf.predict(golden["X_test"]), golden["pred_3"])
    assert clf.score(golden["X_test"], golden["pred_3"]) == 1.0
    Z = clf.decision_function(golden["X_test"][:5])
    np.testing.assert_allclose(Z, golden["X_test"][:5].astype(np.float64) @ golden["coef_3"].T + golden["intercept_3"], atol=1e-4)


def test_fixture_regenerates_where_sklearn_is_importable(golden):
    pytest.importorskip("sklearn")
    pytest.importorskip("scipy")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_probe", os.path.join(os.path.dirname(GOLDEN), "gen_golden_probe.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.generate()  # its own assertions run too: the 0.98 - 1.02 band around tol and the 2 % margin rule
    assert set(new) == set(golden)
    for k in ("X", "y", "X_test", "y_test", "C"):
        assert np.array_equal(new[k], golden[k]), k
    for i in range(7):
        scale = np.abs(golden[f"coef_{i}"]).max()
        assert int(new[f"n_iter_{i}"]) == int(golden[f"n_iter_{i}"])
        assert np.abs(new[f"coef_{i}"] - golden[f"coef_{i}"]).max() <= 1e-9 * scale and np.abs(new[f"intercept_{i}"] - golden[f"intercept_{i}"]).max() <= 1e-9 * scale
        assert np.array_equal(new[f"pred_{i}"], golden[f"pred_{i}"])
        # d32 is the end of an fp32 run: another BLAS may add in another order, so it is held to its size class -- within 4x, or both past the
        # point where the tolerance built from it (8 d32, capped at 1e-4) no longer moves
        a, b = float(new[f"d32_{i}"]), float(golden[f"d32_{i}"])
        assert 0.25 <= a / b <= 4 or min(a, b) >= 1e-4 / 8, (i, a, b)


class Rosenbrock:
    def __init__(self, n=6):
        self.n, self.calls = n, 0

    def value_and_grad(self, x):
        self.calls += 1
        a, b = x[:-1], x[1:]
        f = (100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2).sum()
        g = torch.zeros_like(x)
        g[:-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
        g[1:] += 200.0 * (b - a * a)
        return f, g


class Quadratic:
    """0.5 x^T diag(h) x - c.x with curvatures over four decades"""

    def __init__(self, n=30):
        self.h = torch.logspace(-2, 2, n, dtype=torch.float64)
        self.c = torch.linspace(-1, 1, n, dtype=torch.float64)

    def value_and_grad(self, x):
        return float(0.5 * (self.h * x * x).sum() - (self.c * x).sum()), self.h * x - self.c


@pytest.mark.parametrize("problem", ["rosenbrock", "quadratic"])
def test_line_search_accepts_only_strong_wolfe_steps(problem):
    ev = Rosenbrock() if problem == "rosenbrock" else Quadratic()
    x0 = torch.full((6,), -1.2, dtype=torch.float64) if problem == "rosenbrock" else torch.zeros(30, dtype=torch.float64)
    res = lbfgs.minimize(ev, x0, tol=1e-8, max_iter=2000, record=True)
    assert res.converged and res.n_iter == len(res.searches) > 5
    assert res.max_grad <= 1e-8 or res.status == lbfgs.CONVERGED_DECREASE
    want = torch.ones(6, dtype=torch.float64) if problem == "rosenbrock" else ev.c / ev.h
    assert (res.x - want).abs().max() <= 1e-5 * max(1.0, float(want.abs().max()))
    for f0, gd0, stp, f, gd, verdict, trials in res.searches:
        assert verdict == "converged" and 1 <= trials <= lbfgs.MAX_TRIALS
        assert gd0 < 0 and stp > 0
        assert f <= f0 + lbfgs.FTOL * stp * gd0, "sufficient decrease"
        assert abs(gd) <= lbfgs.GTOL * abs(gd0), "curvature"
    assert res.n_eval == 1 + sum(s[-1] for s in res.searches)


def test_line_search_trial_cap_and_failure_path():
    """The 50-trial cap, and what follows a failed search: with memory, the memory is dropped and steepest descent gets its own trials from the
    same iterate; without, the run ends with FAILED_LINE_SEARCH at the last accepted iterate."""
    class Cone:
        """f = |x| with a constant vector reported as its gradient: from x = 0 the slope promises a descent that no step delivers.  The
        safeguarded step shrinks by a constant factor per trial and, the iterate being 0, every trial point and value stays representable, so
        nothing but the cap ends the search (in a real problem rounding ends it first: the bracket collapses onto the iterate)."""
        calls = 0

        def value_and_grad(self, x):
            self.calls += 1
            return torch.linalg.vector_norm(x), torch.ones_like(x)

    assert lbfgs.MAX_TRIALS == 50
    ev = Cone()
    res = lbfgs.minimize(ev, torch.zeros(4, dtype=torch.float64), record=True)
    assert res.status == lbfgs.FAILED_LINE_SEARCH and not res.converged and "line search" in res.message
    assert (res.n_iter, res.searches, res.f) == (0, [], 0.0) and ev.calls == res.n_eval == 1 + 50 and not res.x.any()  # 50 trials, not one more

    class Plane(Rosenbrock):
        """Rosenbrock for `good` evaluations; from then on the plane through the last good point c that falls a tenth as fast as sufficient
        decrease asks, f = f(c) + 1e-4 g(c).(x - c), with g(c) reported as the gradient everywhere: every trial is refused."""
        def __init__(self, good):
            super().__init__()
            self.good = good

        def value_and_grad(self, x):
            f, g = super().value_and_grad(x)
            if self.calls == self.good:
                self.centre, self.f_centre, self.g_centre = x.clone(), f, g.clone()
            if self.calls > self.good:
                return self.f_centre + 1e-4 * torch.dot(self.g_centre, x - self.centre), self.g_centre.clone()
            return f, g

    ev = Plane(good=9)
    res = lbfgs.minimize(ev, torch.full((6,), -1.2, dtype=torch.float64), tol=1e-8, max_trials=8, record=True)
    assert res.status == lbfgs.FAILED_LINE_SEARCH
    accepted = sum(s[-1] for s in res.searches)
    assert 1 + accepted == 9 and res.n_iter == len(res.searches) >= 2 and res.searches[-1][-1] == 1  # evaluation 9 was an accepted iterate: c
    assert ev.calls == res.n_eval == 9 + 2 * 8  # the search with memory, then the restart from steepest descent: 8 trials each
    assert float(ev.f_centre) == res.f == res.searches[-1][3] and torch.equal(res.x, ev.centre)  # x, f are the last ACCEPTED iterate
    # a start point that already meets the tolerance: no iteration, one evaluation
    res = lbfgs.minimize(Rosenbrock(), torch.ones(6, dtype=torch.float64))
    assert res.status == lbfgs.CONVERGED_GRADIENT and (res.n_iter, res.n_eval) == (0, 1)


def test_max_iter_stops_with_a_status(golden):
    ev = lbfgs.TorchLogistic(torch.from_numpy(golden["X"]), torch.from_numpy(golden["y"]), 19, 1.0)
    res = lbfgs.minimize(ev, torch.zeros(ev.numel(), dtype=torch.float64), max_iter=5)
    assert (res.status, res.n_iter, res.converged) == (lbfgs.STOPPED_ITERATIONS, 5, False)


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------

class StubClassifier:
    """Nearest class mean with a C-dependent tilt, so that the accuracies differ between C values; column 0 of every feature row is the row's
    index in its table, which lets the test read off which rows a fit received."""
    log = []

    def __init__(self, C):
        self.C = C

    def fit(self, X, y):
        X = np.asarray(torch.as_tensor(X).cpu(), dtype=np.float64)
        StubClassifier.log.append((self.C, X[:, 0].astype(int).tolist(), np.asarray(y).tolist()))
        self.classes = np.unique(y)
        self.means = np.stack([X[y == c, 1:].mean(0) for c in self.classes])
        return self

    def predict(self, X):
        X = np.asarray(torch.as_tensor(X).cpu(), dtype=np.float64)[:, 1:]
        tilt = np.sin(np.log10(self.C) * (1 + np.arange(len(self.classes))))
        return self.classes[np.argmax(X @ self.means.T + 0.8 * tilt, axis=1)]


def write_sets(root, name, n_cls, per_class, K, rng, splits):
    labels_all = np.array([3, 7, 8, 20, 41][:n_cls])  # non-contiguous class ids
    mu = rng.standard_normal((n_cls, K))
    for split, n in zip(splits, per_class):
        y = np.repeat(labels_all, n)
        y = y[rng.permutation(len(y))]
        f = (mu[np.searchsorted(labels_all, y)] + 1.5 * rng.standard_normal((len(y), K))).astype(np.float32)
        f = np.concatenate([np.arange(len(y), dtype=np.float32)[:, None], f], axis=1)
        lpclip.save_features(root, name, split, f, y)


def expected_protocol(sets, name, feature_dir, num_step, num_run, shots):
    """The script's arithmetic, written out again: returns (fits in order as (C, training rows), detail lines, summary lines)."""
    (Xtr, ytr), (Xva, yva), (Xte, yte) = sets
    fits, details, summary = [], [], []

    def run(c, rows, vrows):
        clf = StubClassifier(c).fit(Xtr[rows], ytr[rows])
        fits.append((c, list(rows)))
        return clf, sum(clf.predict(Xva[vrows]) == yva[vrows]) / len(vrows)

    for shot in shots:
        last = []
        for seed in range(1, num_run + 1):
            np.random.seed(seed)
            classes = np.unique(ytr)
            rows = [i for c in classes for i in np.random.choice(np.where(ytr == c)[0], size=shot, replace=False)]
            vshot = {1: 1, 2: 2, 4: 4, 8: 4, 16: 4}[shot]
            vrows = [i for c in classes for i in np.random.choice(np.where(yva == c)[0], size=vshot, replace=False)]
            grid = [1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6]
            accs = [run(c, rows, vrows)[1] for c in grid]
            peak = grid[int(np.argmax(accs))]
            lo, hi = 1e-1 * peak, 1e1 * peak
            for step in range(num_step):
                (clf_lo, acc_lo), (clf_hi, acc_hi) = run(lo, rows, vrows), run(hi, rows, vrows)
                mid = 0.5 * (np.log10(hi) + np.log10(lo))
                if acc_lo < acc_hi:
                    c_final, clf, nxt = hi, clf_hi, (mid, np.log10(hi))
                else:
                    c_final, clf, nxt = lo, clf_lo, (np.log10(lo), mid)
                acc = 100 * sum(clf.predict(Xte) == yte) / len(yte)
                details.append("{}, seed {}, {} shot, weight {}, test_acc {:.2f}\n".format(name, seed, shot, c_final, acc))
                lo, hi = np.power(10, nxt[0]), np.power(10, nxt[1])
            last.append(acc)
        summary.append("{}, {} Shot, Test acc stat: {:.2f} ({:.2f})\n".format(name, shot, np.mean(last), np.std(last)))
    return fits, details, summary


def test_linear_probe_protocol_matches_the_scripts_arithmetic(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(7)
    write_sets("clip_feat", "toy", 5, (20, 9, 11), 6, rng, ("train", "val", "test"))
    sets = [tuple(np.load(f"clip_feat/toy/{s}.npz")[k] for k in ("feature_list", "label_list")) for s in ("train", "val", "test")]
    num_step, num_run, shots = 3, 2, [16, 8, 4, 2, 1]
    StubClassifier.log = []
    lines = []
    got = lpclip.linear_probe("toy", "toy", num_step=num_step, num_run=num_run, feature_dir="clip_feat", classifier=StubClassifier, log=lines.append)
    mine = list(StubClassifier.log)
    fits, details, summary = expected_protocol(sets, "toy", "clip_feat", num_step, num_run, shots)
    assert len(mine) == len(fits) == len(shots) * num_run * (7 + 2 * num_step)
    for (c, rows, labels), (c_want, rows_want) in zip(mine, fits):
        assert c == c_want and type(c) is type(c_want), (c, c_want)  # the bisection hands 10 ** c back as numpy's float64, bit for bit
        assert rows == [int(r) for r in rows_want]                    # the sampled indices, in order
        assert labels == sets[0][1][rows_want].tolist()
    assert len({tuple(r) for _, r, _ in mine}) == len(shots) * num_run  # every (shot, seed) drew its own subset
    assert len({c for c, _, _ in mine}) > 7 + 2  # the bisection moved
    assert open(f"report/toy/clip_feat_s{num_step}r{num_run}_details.txt").readlines() == details
    assert open(f"report/toy/clip_feat_s{num_step}r{num_run}.txt").readlines() == summary
    assert sorted(got) == sorted(shots) and got[16].shape == (num_run, num_step)
    assert any(line.startswith("toy, 16 Shot, Round 0: ") for line in lines) and any(line.startswith("search c_weight accuracy: [") for line in lines)


def test_command_line_takes_the_scripts_arguments(capsys):
    with pytest.raises(SystemExit) as e:
        lpclip.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--trainval_dataset", "--test_dataset", "--num_step", "--num_run", "--feature_dir"):
        assert flag in out


# ---- the classifier's surface ------------------------------------------------------------------------------------------------------------

def test_classes_map_non_contiguous_labels(golden):
    X, y = golden["X"], golden["y"]
    ids = np.array([5, 9, 100, 101, -3, 17, 1000, 42, 43, 44, 60, 61, 62, 7, 8, 2, 1, 0, 77])  # 19 ids, unsorted
    a = lpclip.LogisticProbe(C=1.0, evaluator="torch64", device="cpu").fit(X, y)
    b = lpclip.LogisticProbe(C=1.0, evaluator="torch64", device="cpu").fit(torch.from_numpy(X), torch.from_numpy(ids[y]))
    assert np.array_equal(a.classes_, np.arange(19)) and np.array_equal(b.classes_, np.sort(ids))
    order = np.argsort(ids)  # row r of b's coefficients is class ids[order[r]]
    # the same fit with its classes in another order: sums run in another order, nothing else differs
    np.testing.assert_allclose(b.coef_, a.coef_[order], rtol=0, atol=1e-9)
    np.testing.assert_allclose(b.intercept_, a.intercept_[order], rtol=0, atol=1e-9)
    assert b.n_iter_ == a.n_iter_
    assert np.array_equal(b.predict(golden["X_test"]), ids[a.predict(golden["X_test"])])
    assert b.score(golden["X_test"], ids[golden["y_test"]]) == a.score(golden["X_test"], golden["y_test"])


def test_argument_errors_come_before_any_gpu_call():
    """With the default (HIP) evaluator on a machine without a GPU any device call would raise something else than ValueError."""
    X, y = np.zeros((6, 4), dtype=np.float32), np.array([0, 1, 2, 0, 1, 2])
    for C in (0.0, -1.0, float("nan"), 1e-60):  # 1e-60 is zero as fp32, the type C travels in
        with pytest.raises(ValueError, match="C must be positive"):
            lpclip.LogisticProbe(C=C)
    with pytest.raises(ValueError, match="max_iter"):
        lpclip.LogisticProbe(C=1.0, max_iter=0)
    clf = lpclip.LogisticProbe(C=1.0)
    with pytest.raises(ValueError, match="outside"):
        clf.fit_indexed(X, np.array([0, 1, 3, 0, 1, 2]), 3)
    with pytest.raises(ValueError, match="outside"):
        clf.fit_indexed(X, np.array([0, 1, -1, 0, 1, 2]), 3)
    with pytest.raises(ValueError, match="do not match"):
        clf.fit(X, y[:5])
    with pytest.raises(ValueError, match="do not match"):
        clf.fit(X.reshape(-1), y)
    with pytest.raises(ValueError, match="empty"):
        clf.fit(X[:0], y[:0])
    with pytest.raises(ValueError, match="empty"):
        clf.fit(X[:, :0], y)
    with pytest.raises(ValueError, match="integers"):
        clf.fit(X, y.astype(np.float32))
    with pytest.raises(ValueError, match="two classes"):
        clf.fit(X, np.zeros(6, dtype=np.int64))
    with pytest.raises(ValueError, match="not fitted"):
        clf.predict(X)
    fitted = lpclip.LogisticProbe(C=1.0, evaluator="torch64", device="cpu").fit(X + np.arange(6, dtype=np.float32)[:, None], y)
    with pytest.raises(ValueError, match="width"):
        fitted.predict(np.zeros((2, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="empty"):
        fitted.predict(X[:0])


def test_split_reduction_slice_rule():
    """Host arithmetic of the gradient GEMM's split (mudpt_probe_gemm_tn_slices): slices of whole 32-deep steps, at least two steps each when the
    library chooses, about two workgroups per compute unit."""
    from mudpt_amd import build, capi
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    s = lambda M, N, Kd, want, ncu: capi.call("mudpt_probe_gemm_tn_slices", M=M, N=N, Kd=Kd, slices=want, ncu=ncu)  # noqa: E731
    assert s(1000, 512, 16000, 0, 256) == 16 and s(100, 512, 1600, 0, 256) == 25  # 32 tiles x 16; 4 tiles: 50 steps / 2
    assert s(19, 40, 76, 0, 256) == 1 and s(19, 40, 20, 0, 256) == 1 and s(19, 40, 20, 8, 256) == 1  # a depth below one slice
    assert s(8, 8, 1031, 4, 256) == 4 and s(8, 8, 1031, 33, 256) == 33 and s(8, 8, 1031, 1000, 256) == 33  # 33 steps: 9 + 9 + 9 + 6
    assert s(8, 8, 1031, 5, 256) == 5 and s(8, 8, 1031, 6, 256) == 6 and s(8, 8, 1031, 7, 256) == 7 and s(8, 8, 1031, 10, 256) == 9  # ceil(33 / 4) = 9 slices of 4
    assert s(0, 8, 8, 0, 256) == -1 and s(8, 8, 0, 0, 256) == -1
