"""Writes tests/golden/probe_sklearn.npz: what sklearn's LogisticRegression(solver="lbfgs", max_iter=1000, penalty="l2") -- the classifier of
lpclip/linear_probe.py:64 -- gives on a small few-shot problem, for the seven C of the script's search list.  Needs sklearn and scipy.

    python tests/golden/gen_golden_probe.py            # writes the file
    (tests/test_probe_cpu.py regenerates the numbers where sklearn is importable and compares)

Fixture: 19 classes x 4 shots, K = 40, X = 1.6 (mu_y + eps) as fp32 with mu ~ 0.5 N(0, 1), eps ~ N(0, 1), numpy.default_rng(0); 760 held-out rows
(40 per class) drawn the same way.  Per C (rounded to fp32, as it travels to the kernels): coef_, intercept_, n_iter_ and d32 -- the relative
deviation from sklearn of scipy's own L-BFGS-B fed a numpy fp32 evaluation of the objective: the size of fp32 evaluation error after the
optimiser, measured without any code of this project.
"""
import os

import numpy as np

SEED = 0
N_CLS, SHOTS, K, HELD_OUT_PER_CLASS = 19, 4, 40, 40
C_LIST = [1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6]
TOL = 1e-4
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe_sklearn.npz")


def make_data():
    rng = np.random.default_rng(SEED)
    mu = 0.5 * rng.standard_normal((N_CLS, K))
    y = np.repeat(np.arange(N_CLS), SHOTS)
    X = (1.6 * (mu[y] + rng.standard_normal((len(y), K)))).astype(np.float32)
    y_test = np.repeat(np.arange(N_CLS), HELD_OUT_PER_CLASS)
    X_test = (1.6 * (mu[y_test] + rng.standard_normal((len(y_test), K)))).astype(np.float32)
    return X, y.astype(np.int64), X_test, y_test.astype(np.int64)


def objective64(X, y, W, b, C):
    """F and its gradient in float64 (the formulas of mudpt_amd/lpclip.py's docstring)."""
    N = len(y)
    Z = X.astype(np.float64) @ W.T + b
    m = Z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(Z - m).sum(1))
    f = (lse - Z[np.arange(N), y]).mean() + (W * W).sum() / (2 * C * N)
    P = np.exp(Z - lse[:, None])
    P[np.arange(N), y] -= 1
    P /= N
    return f, P.T @ X.astype(np.float64) + W / (C * N), P.sum(0)


def fit_scipy_fp32(X, y, n_cls, C):
    """scipy's L-BFGS-B with sklearn's options on an fp32 numpy evaluation of F."""
    from scipy.optimize import minimize
    N, K_ = X.shape
    reg = np.float32(1.0 / (float(C) * N))
    onehot = np.zeros((N, n_cls), dtype=np.float32)
    onehot[np.arange(N), y] = 1

    def fun(x):
        x = x.astype(np.float32)
        W, b = x[:n_cls * K_].reshape(n_cls, K_), x[n_cls * K_:]
        Z = X @ W.T + b
        m = Z.max(1, keepdims=True)
        E = np.exp(Z - m)
        s = E.sum(1, keepdims=True)
        f = np.float32((m[:, 0] + np.log(s[:, 0]) - Z[np.arange(N), y]).sum(dtype=np.float32) / np.float32(N)) + np.float32(0.5) * reg * (W * W).sum(dtype=np.float32)
        P = (E / s - onehot) / np.float32(N)
        g = np.concatenate([(P.T @ X + reg * W).ravel(), P.sum(0)])
        return float(f), g.astype(np.float64)

    res = minimize(fun, np.zeros(n_cls * (K_ + 1)), jac=True, method="L-BFGS-B",
                   options={"maxiter": 1000, "maxls": 50, "gtol": TOL, "ftol": 64 * np.finfo(float).eps})
    return res.x[:n_cls * K_].reshape(n_cls, K_), res.x[n_cls * K_:]


def low_margin(coef, intercept, X):
    """rows whose top-two margin is below 2 tol max|coef| (|x|_1 + 1): a coefficient error of tol max|coef| could change their prediction"""
    Z = X.astype(np.float64) @ coef.T + intercept
    top = np.sort(Z, axis=1)
    return (top[:, -1] - top[:, -2]) < 2 * TOL * np.abs(coef).max() * (np.abs(X.astype(np.float64)).sum(1) + 1)


def generate():
    from sklearn.linear_model import LogisticRegression
    X, y, X_test, y_test = make_data()
    out = {"X": X, "y": y, "X_test": X_test, "y_test": y_test, "C": np.array(C_LIST, dtype=np.float32)}
    for i, c in enumerate(out["C"]):
        C = float(c)
        clf = LogisticRegression(solver="lbfgs", max_iter=1000, penalty="l2", C=C, tol=TOL).fit(X, y)
        _, gW, gb = objective64(X, y, clf.coef_, clf.intercept_, C)
        ratio = max(np.abs(gW).max(), np.abs(gb).max()) / TOL
        assert not 0.98 <= ratio <= 1.02, f"C = {C}: sklearn stopped at max|g| = {ratio:.3f} tol; change SEED, not the rule"
        low = low_margin(clf.coef_, clf.intercept_, X_test)
        assert low.mean() <= 0.02, f"C = {C}: {low.mean():.3%} of the held-out rows have a top-two margin inside the coefficient tolerance"
        W32, b32 = fit_scipy_fp32(X, y, N_CLS, C)
        scale = max(np.abs(clf.coef_).max(), np.abs(clf.intercept_).max())
        d32 = max(np.abs(W32 - clf.coef_).max(), np.abs(b32 - clf.intercept_).max()) / scale
        print(f"C = {C:g}: n_iter {clf.n_iter_[0]}, final max|g| = {ratio:.3f} tol, low-margin rows {low.mean():.2%}, d32 {d32:.3e}")
        out[f"coef_{i}"], out[f"intercept_{i}"] = clf.coef_, clf.intercept_
        out[f"n_iter_{i}"], out[f"d32_{i}"] = np.int64(clf.n_iter_[0]), np.float64(d32)
        out[f"pred_{i}"] = clf.predict(X_test).astype(np.int64)
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **generate())
    print(PATH, os.path.getsize(PATH), "bytes")
