"""Regenerates tests/golden/evaluator_sklearn.npz: sklearn's numbers for the test pass's evaluator, called the way Dassl's Classification
evaluator calls them (dassl/evaluation/evaluator.py):

    macro_f1 = 100.0 * f1_score(y_true, y_pred, average="macro", labels=np.unique(y_true))
    cmat     = confusion_matrix(y_true, y_pred, normalize="true")
    perclass = np.mean([100.0 * correct / total for every label that occurs, sorted])

Recorded with scikit-learn 1.7.2.  Run from the repository root: python tests/golden/gen_golden_evaluator.py
Every case holds <name>_n_cls, _y_true, _y_pred, _macro_f1, _perclass_accuracy and _labels (the sorted union of y_true and y_pred, the
rows and columns of sklearn's matrix); c37 also _cmat.
"""
import os

import numpy as np
from sklearn.metrics import confusion_matrix, f1_score

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "evaluator_sklearn.npz")


def noisy(rng, y, n_cls, p_right):
    wrong = rng.integers(0, n_cls, y.shape[0])
    return np.where(rng.random(y.shape[0]) < p_right, y, wrong)


def cases():
    rng = np.random.default_rng(20240607)
    # 37 classes, 500 samples: classes 30 .. 36 never occur as labels; class 5 is never predicted; class 31 is predicted but never true
    y = rng.integers(0, 30, 500)
    p = noisy(rng, y, 30, 0.6)
    p[p == 5] = 6
    p[rng.choice(500, 9, replace=False)] = 31
    assert set(np.unique(y)) == set(range(30)) and 5 not in p and 31 in p and 31 not in y
    yield "c37", 37, y, p, True
    y = rng.integers(0, 2, 200)
    yield "c2", 2, y, noisy(rng, y, 2, 0.5), False
    y = np.zeros(50, dtype=np.int64)
    yield "c1", 1, y, y.copy(), False
    # 1000 classes, 3000 samples over 300 of them: most classes are unsupported; the predictions range over all 1000
    y = rng.choice(1000, 300, replace=False)[rng.integers(0, 300, 3000)]
    yield "c1000", 1000, y, noisy(rng, y, 1000, 0.7), False


def main():
    out = {}
    for name, n_cls, y_true, y_pred, with_cmat in cases():
        yt, yp = y_true.tolist(), y_pred.tolist()  # Dassl keeps Python lists
        out[f"{name}_n_cls"] = np.int64(n_cls)
        out[f"{name}_y_true"], out[f"{name}_y_pred"] = y_true.astype(np.int16), y_pred.astype(np.int16)
        out[f"{name}_macro_f1"] = np.float64(100.0 * f1_score(yt, yp, average="macro", labels=np.unique(yt)))
        accs = [100.0 * sum(p == t for p, t in zip(yp, yt) if t == label) / yt.count(label) for label in sorted(set(yt))]
        out[f"{name}_perclass_accuracy"] = np.float64(np.mean(accs))
        out[f"{name}_labels"] = np.union1d(y_true, y_pred).astype(np.int16)
        if with_cmat:
            out[f"{name}_cmat"] = confusion_matrix(yt, yp, normalize="true")
            assert out[f"{name}_cmat"].shape == (out[f"{name}_labels"].size,) * 2
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
