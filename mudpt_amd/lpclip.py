"""The reference's linear-probe baseline (lpclip/), both halves.

Feature extraction (lpclip/feat_extractor.py:113-137): the raw ``clip_model.visual(image)`` features of every image of a split, saved in the
file ``lpclip/linear_probe.py`` reads -- ``extract_features`` / ``save_features``.

The probe (lpclip/linear_probe.py): ``LogisticProbe`` is its ``LogisticRegression(solver="lbfgs", max_iter=1000, penalty="l2", C=c)`` on the
GPU -- the multinomial objective

    F(W, b) = (1/N) sum_i [logsumexp(z_i) - z_i[y_i]] + |W|^2 / (2 C N),   z_i = W x_i + b,   start W = 0, b = 0,

evaluated by the kernels of csrc/probe.hip (two exact-fp32 GEMMs on the matrix cores and a row kernel) and minimised by mudpt_amd/lbfgs.py, the
L-BFGS that solver runs.  ``linear_probe`` is the script's protocol -- few-shot sampling per seed, a seven-value search for C, a bisection in
log10(C), two report files -- and ``python -m mudpt_amd.lpclip`` takes the script's five arguments.  Features are uploaded once and stay on the
device across the 345 fits of a run.

Two classes: this class fits the same softmax objective with two rows of W; sklearn switches to the one-row sigmoid form there, whose penalty
counts |w1 - w0|^2 instead of |w0|^2 + |w1|^2.  The reference's datasets all have more classes.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import lbfgs


@torch.no_grad()
def extract_features(model, loader, on_device=False):
    """feat_extractor.py:118-129: ``model.encode_image`` (a ``zsclip.FrozenCLIP``) over the batches of ``loader`` (dicts with "img" and
    "label").  Returns (features float32 [N, embed_dim], labels int64 [N]) in loader order: on the host, or with on_device=True where the model
    left them (what ``LogisticProbe`` and ``linear_probe`` take without another copy)."""
    features, labels = [], []
    for batch in loader:
        f = model.encode_image(batch["img"]).to(torch.float32)
        y = torch.as_tensor(batch["label"]).to(torch.int64).reshape(-1)
        features.append(f if on_device else f.cpu())
        labels.append(y.to(f.device) if on_device else y.cpu())
    if not features:
        return torch.zeros(0, model.shape.embed_dim, dtype=torch.float32), torch.zeros(0, dtype=torch.int64)
    return torch.cat(features), torch.cat(labels)


def save_features(output_dir, dataset_name, split, features, labels) -> str:
    """feat_extractor.py:130-137: ``{output_dir}/{dataset_name}/{split}.npz`` with the keys ``feature_list`` (float32) and ``label_list``
    (int64).  The file is complete or absent: written under a temporary name in the same directory, then renamed."""
    save_dir = os.path.join(output_dir, dataset_name)
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, f"{split}.npz")
    tmp = os.path.join(save_dir, f".{split}.npz.{os.getpid()}.tmp")
    try:
        with open(tmp, "wb") as f:
            np.savez(f, feature_list=np.asarray(torch.as_tensor(features).cpu(), dtype=np.float32),
                     label_list=np.asarray(torch.as_tensor(labels).cpu(), dtype=np.int64))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


# ---- the objective on the GPU ------------------------------------------------------------------------------------------------------------

def _stream():
    return torch.cuda.current_stream().cuda_stream


def probe_gemm_nt(A, B, bias, out):
    """out [M, N] = A [M, K] . B [N, K]^T (+ bias): fp32 device tensors with unit inner stride (csrc/probe.hip)."""
    from . import capi
    (M, K), N = A.shape, B.shape[0]
    capi.check(capi.call("mudpt_probe_gemm_nt", M=M, N=N, K=K, A=A, lda=A.stride(0), B=B, ldb=B.stride(0), bias=bias, C=out, ldc=out.stride(0),
                         stream=_stream()), "probe_gemm_nt")
    return out


def probe_tn_slices(M, N, Kd, slices=0, device=None):
    from . import capi
    return capi.call("mudpt_probe_gemm_tn_slices", M=M, N=N, Kd=Kd, slices=slices, ncu=torch.cuda.get_device_properties(device).multi_processor_count)


def probe_gemm_tn(A, B, out, beta=0.0, W=None, db=None, scratch=None, slices=0):
    """out [M, N] = A [Kd, M]^T . B [Kd, N] (+ beta W), db [M] = column sums of A, the depth split over `slices` workgroups per tile."""
    from . import capi
    (Kd, M), N = A.shape, B.shape[1]
    slices = probe_tn_slices(M, N, Kd, slices, A.device)
    if scratch is None:
        scratch = torch.empty(slices * (M * N + M), dtype=torch.float32, device=A.device)
    capi.check(capi.call("mudpt_probe_gemm_tn", M=M, N=N, Kd=Kd, A=A, lda=A.stride(0), B=B, ldb=B.stride(0), beta=beta, W=W,
                         ldw=W.stride(0) if W is not None else 0, C=out, ldc=out.stride(0), db=db, scratch=scratch, scratch_numel=scratch.numel(),
                         slices=slices, stream=_stream()), "probe_gemm_tn")
    return out


def probe_rows(Z, labels, row_loss, loss_sum):
    """Z [rows, n_cls] logits -> P = (softmax - onehot) / rows in place; row_loss [rows] fp32; loss_sum [1] float64 = their sum."""
    from . import capi
    capi.check(capi.call("mudpt_probe_rows", Z=Z, ldz=Z.stride(0), labels=labels, rows=Z.shape[0], n_cls=Z.shape[1], row_loss=row_loss, loss_sum=loss_sum,
                         stream=_stream()), "probe_rows")


def probe_argmax(Z, pred, labels=None, count=None):
    from . import capi
    capi.check(capi.call("mudpt_probe_argmax", Z=Z, ldz=Z.stride(0), rows=Z.shape[0], n_cls=Z.shape[1], pred=pred, labels=labels, count=count,
                         stream=_stream()), "probe_argmax")
    return pred


class HipLogistic:
    """The objective on the HIP kernels: ``value_and_grad(x64)`` casts x = [W.ravel(), b] to fp32, runs Z = X W^T + b, the row kernel, and
    dW = P^T X + W / (C N) with db = P^T 1 from the same pass -- five launches -- and casts the gradient back.  X fp32 [N, K] and labels int32 [N]
    are device tensors and stay where they are; nothing here synchronises.  C travels as fp32; 1 / (C N) is formed in double from that value."""
    LAUNCHES = 5  # logit GEMM, row kernel, loss sum, gradient GEMM, its ordered reduction

    def __init__(self, X, labels, n_cls, C):
        assert X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1 and labels.dtype == torch.int32
        self.X, self.labels, self.n_cls = X, labels, n_cls
        self.N, self.K = X.shape
        self.reg = 1.0 / (float(np.float32(C)) * self.N)
        dev, nW = X.device, n_cls * self.K
        self.nW = nW
        self.x32 = torch.empty(nW + n_cls, dtype=torch.float32, device=dev)
        self.g32 = torch.empty(nW + n_cls, dtype=torch.float32, device=dev)
        self.Z = torch.empty(self.N, n_cls, dtype=torch.float32, device=dev)
        self.row_loss = torch.empty(self.N, dtype=torch.float32, device=dev)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        self.slices = probe_tn_slices(n_cls, self.K, self.N, 0, dev)
        self.scratch = torch.empty(self.slices * (nW + n_cls), dtype=torch.float32, device=dev)

    def numel(self):
        return self.nW + self.n_cls

    def value_and_grad(self, x):
        nW, W64 = self.nW, x[:self.nW]
        self.x32.copy_(x)
        W, b = self.x32[:nW].view(self.n_cls, self.K), self.x32[nW:]
        probe_gemm_nt(self.X, W, b, self.Z)
        probe_rows(self.Z, self.labels, self.row_loss, self.loss_sum)
        probe_gemm_tn(self.Z, self.X, self.g32[:nW].view(self.n_cls, self.K), beta=float(np.float32(self.reg)), W=W, db=self.g32[nW:], scratch=self.scratch,
                      slices=self.slices)
        f = self.loss_sum[0] / self.N + (0.5 * self.reg) * torch.dot(W64, W64)
        return f, self.g32.to(torch.float64)


# ---- the classifier ----------------------------------------------------------------------------------------------------------------------

def _features(X, device):
    """fp32 [N, K] with unit inner stride on `device`; a tensor that already is one is taken as it is."""
    X = torch.as_tensor(X)
    if X.dim() != 2:
        raise ValueError(f"features must be [N, K], got {tuple(X.shape)}")
    return X.to(device=device, dtype=torch.float32).contiguous()


class LogisticProbe:
    """``LogisticRegression(solver="lbfgs", penalty="l2", C=C, max_iter=max_iter, tol=tol)`` of lpclip/linear_probe.py:64 on the GPU.  Features
    are numpy arrays or tensors (device tensors are used where they are); labels any integers, mapped through ``np.unique`` to ``classes_``.
    After ``fit``: ``coef_`` [n_cls, K] and ``intercept_`` [n_cls] (float64 numpy), ``n_iter_`` (an array of one, as sklearn's), ``status_``
    (mudpt_amd.lbfgs.STATUS).  ``evaluator`` = "hip" (default; needs the GPU) or "torch64" (the float64 reference evaluator, any device)."""

    def __init__(self, C=1.0, max_iter=1000, tol=1e-4, device=None, evaluator="hip"):
        if not (np.isfinite(C) and C > 0 and float(np.float32(C)) > 0):
            raise ValueError(f"C must be positive (and positive as fp32), got {C}")
        if max_iter < 1 or not tol > 0:
            raise ValueError(f"max_iter {max_iter} and tol {tol} must be positive")
        if evaluator not in ("hip", "torch64"):
            raise ValueError(f"unknown evaluator {evaluator!r}")
        self.C, self.max_iter, self.tol, self.evaluator = C, max_iter, tol, evaluator
        self.device = torch.device(device if device is not None else ("cuda" if evaluator == "hip" else "cpu"))

    def fit(self, X, y):
        y_host = np.asarray(torch.as_tensor(y).cpu())
        if y_host.ndim != 1 or not np.issubdtype(y_host.dtype, np.integer):
            raise ValueError(f"labels must be a vector of integers, got {y_host.dtype} {y_host.shape}")
        classes, index = np.unique(y_host, return_inverse=True)
        return self.fit_indexed(X, index, len(classes), classes=classes)

    def fit_indexed(self, X, index, n_cls, classes=None):
        """``fit`` on labels that already are class indices in [0, n_cls).  Everything is validated here, on the host, once per fit and before
        any GPU call: the kernels trust the labels they are given."""
        index = np.asarray(torch.as_tensor(index).cpu())
        shape = tuple(X.shape) if hasattr(X, "shape") else np.asarray(X).shape
        if len(shape) != 2 or index.ndim != 1 or shape[0] != index.shape[0]:
            raise ValueError(f"features {shape} and labels {index.shape} do not match")
        if shape[0] == 0 or shape[1] == 0:
            raise ValueError("an empty training set")
        if not np.issubdtype(index.dtype, np.integer):
            raise ValueError(f"labels must be integers, got {index.dtype}")
        if n_cls < 2:
            raise ValueError("the probe needs at least two classes")
        if index.min() < 0 or index.max() >= n_cls:
            raise ValueError(f"a label outside [0, {n_cls}): {int(index.min())} .. {int(index.max())}")
        self.classes_ = np.arange(n_cls) if classes is None else np.asarray(classes)
        X, index = _features(X, self.device), torch.as_tensor(index.astype(np.int32)).to(self.device)
        K = X.shape[1]
        ev = HipLogistic(X, index, n_cls, self.C) if self.evaluator == "hip" else lbfgs.TorchLogistic(X, index, n_cls, self.C)
        res = lbfgs.minimize(ev, torch.zeros(n_cls * (K + 1), dtype=torch.float64, device=X.device), tol=self.tol, max_iter=self.max_iter)
        self.result_ = res
        self.status_ = res.message
        self.n_iter_ = np.array([res.n_iter], dtype=np.int32)
        self._W = res.x[:n_cls * K].view(n_cls, K).to(torch.float32).contiguous()
        self._b = res.x[n_cls * K:].to(torch.float32).contiguous()
        x = res.x.cpu().numpy()
        self.coef_, self.intercept_ = x[:n_cls * K].reshape(n_cls, K).copy(), x[n_cls * K:].copy()
        return self

    def _check(self, X):
        if not hasattr(self, "coef_"):
            raise ValueError("this LogisticProbe is not fitted yet")
        X = _features(X, self.device)
        if X.shape[1] != self.coef_.shape[1]:
            raise ValueError(f"features of width {X.shape[1]}, the probe was fitted on {self.coef_.shape[1]}")
        if X.shape[0] == 0:
            raise ValueError("an empty set")
        return X

    def _decision(self, X):
        if self.evaluator == "hip":
            return probe_gemm_nt(X, self._W, self._b, torch.empty(X.shape[0], self._W.shape[0], dtype=torch.float32, device=X.device))
        return torch.addmm(self._b.double(), X.double(), self._W.double().t())

    def decision_function(self, X):
        return self._decision(self._check(X)).cpu().numpy()

    def _predict_index(self, X):
        """class indices (int32 device tensor) of checked device features"""
        Z = self._decision(X)
        if self.evaluator == "hip":
            return probe_argmax(Z, torch.empty(Z.shape[0], dtype=torch.int32, device=Z.device))
        return Z.argmax(dim=1).to(torch.int32)

    def predict(self, X):
        index = self._predict_index(self._check(X)).cpu().numpy()
        return self.classes_[index]

    def score(self, X, y):
        y = np.asarray(torch.as_tensor(y).cpu())
        pred = self.predict(X)
        if pred.shape != y.shape:
            raise ValueError(f"features {pred.shape[0]} rows, labels {y.shape}")
        return float(np.mean(pred == y))


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------

VAL_SHOT_LIST = {1: 1, 2: 2, 4: 4, 8: 4, 16: 4}  # linear_probe.py:33
SEARCH_LIST = [1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6]  # linear_probe.py:61
SHOTS = [16, 8, 4, 2, 1]  # linear_probe.py:35


def sample_few_shot(all_label_list, labels, num_shot):
    """linear_probe.py:43-47 / :52-56: per class of all_label_list (``np.unique`` of the TRAINING labels, for the validation subset too),
    ``np.random.choice`` of num_shot of its indices in `labels` without replacement, from numpy's GLOBAL generator (the caller seeds it)."""
    selected = []
    for label in all_label_list:
        selected.extend(np.random.choice(np.where(labels == label)[0], size=num_shot, replace=False))
    return selected


def _load(path):
    f = np.load(path)
    return f["feature_list"], f["label_list"]


def linear_probe(trainval_dataset, test_dataset, num_step=8, num_run=3, feature_dir="clip_feat", device=None, classifier=None, log=print):
    """lpclip/linear_probe.py line for line.  Reads ``{feature_dir}/{trainval_dataset}/train.npz`` / ``val.npz`` and
    ``{feature_dir}/{test_dataset}/test.npz``; for each shot count and seed 1..num_run: ``np.random.seed(seed)``, the training subset, then the
    validation subset (``VAL_SHOT_LIST``), one fit per value of ``SEARCH_LIST``, then num_step bisection rounds of two fits around the best C
    (first maximum), each round appending a line to ``report/{test_dataset}/{feature_dir}_s{num_step}r{num_run}_details.txt``; per shot
    count one line of mean (std) of the last round's test accuracies to ``..._s{num_step}r{num_run}.txt``.  (The script's own call of its
    ``binary_search`` leaves out two parameters the body never reads; this is what the body does.)

    The three feature tables are uploaded once; subsets are gathered on the device.  ``classifier(C)`` -> an object with ``fit(X, y)`` and
    ``predict(X)`` taking device tensors for X and numpy labels (default: ``LogisticProbe`` on `device`).  Returns {num_shot: [num_run, num_step]
    test accuracies}."""
    if classifier is None:
        dev = torch.device(device if device is not None else "cuda")
        classifier = lambda c: LogisticProbe(C=c, max_iter=1000, device=dev)  # noqa: E731
    else:
        dev = torch.device(device if device is not None else "cpu")
    log(f"loading train and val files of Dataset: {trainval_dataset}")
    train_feature, train_label = _load(os.path.join(feature_dir, trainval_dataset, "train.npz"))
    val_feature, val_label = _load(os.path.join(feature_dir, trainval_dataset, "val.npz"))
    log(f"Loading test file of Dataset: {test_dataset}")
    test_feature, test_label = _load(os.path.join(feature_dir, test_dataset, "test.npz"))
    for name, f, y in (("train", train_feature, train_label), ("val", val_feature, val_label), ("test", test_feature, test_label)):
        if f.ndim != 2 or y.ndim != 1 or len(f) != len(y) or len(y) == 0:
            raise ValueError(f"{name}: features {f.shape} and labels {y.shape} do not make a set")
    train_dev, val_dev, test_dev = (_features(f, dev) for f in (train_feature, val_feature, test_feature))
    os.makedirs(f"report/{test_dataset}", exist_ok=True)
    stem = "./report/{}/{}_s{}r{}".format(test_dataset, feature_dir, num_step, num_run)  # linear_probe.py:108,124
    results = {}

    def fit_and_score(c, X, y, Xv, yv):
        clf = classifier(c).fit(X, y)
        pred = np.asarray(clf.predict(Xv))
        return clf, np.sum(pred == yv) / len(yv)

    for num_shot in SHOTS:
        test_acc_step_list = np.zeros([num_run, num_step])
        for seed in range(1, num_run + 1):
            np.random.seed(seed)
            log(f"-- Seed: {seed} --------------------------------------------------------------")
            all_label_list = np.unique(train_label)
            selected = sample_few_shot(all_label_list, train_label, num_shot)
            X, y = train_dev[torch.as_tensor(np.asarray(selected, dtype=np.int64), device=dev)], train_label[selected]
            val_selected = sample_few_shot(all_label_list, val_label, VAL_SHOT_LIST[num_shot])
            Xv, yv = val_dev[torch.as_tensor(np.asarray(val_selected, dtype=np.int64), device=dev)], val_label[val_selected]

            acc_list = [fit_and_score(c, X, y, Xv, yv)[1] for c in SEARCH_LIST]
            log(f"search c_weight accuracy: {acc_list}")
            c_peak = SEARCH_LIST[np.argmax(acc_list)]
            c_left, c_right = 1e-1 * c_peak, 1e1 * c_peak
            for step in range(num_step):
                log(f"{test_dataset}, {num_shot} Shot, Round {step}: {c_left}/{c_right}")
                clf_left, acc_left = fit_and_score(c_left, X, y, Xv, yv)
                log("Val accuracy (Left): {:.2f}".format(100 * acc_left))
                clf_right, acc_right = fit_and_score(c_right, X, y, Xv, yv)
                log("Val accuracy (Right): {:.2f}".format(100 * acc_right))
                if acc_left < acc_right:
                    c_final, clf_final = c_right, clf_right
                    c_left, c_right = 0.5 * (np.log10(c_right) + np.log10(c_left)), np.log10(c_right)
                else:
                    c_final, clf_final = c_left, clf_left
                    c_left, c_right = np.log10(c_left), 0.5 * (np.log10(c_right) + np.log10(c_left))
                pred = np.asarray(clf_final.predict(test_dev))
                test_acc = 100 * np.sum(pred == test_label) / len(pred)
                log("Test Accuracy: {:.2f}".format(test_acc))
                test_acc_step_list[seed - 1, step] = test_acc
                with open(stem + "_details.txt", "a+") as writer:
                    writer.write("{}, seed {}, {} shot, weight {}, test_acc {:.2f}\n".format(test_dataset, seed, num_shot, c_final, test_acc))
                c_left, c_right = np.power(10, c_left), np.power(10, c_right)
        test_acc_list = test_acc_step_list[:, -1]
        save_line = "{}, {} Shot, Test acc stat: {:.2f} ({:.2f})\n".format(test_dataset, num_shot, np.mean(test_acc_list), np.std(test_acc_list))
        log(save_line)
        with open(stem + ".txt", "a+") as writer:
            writer.write(save_line)
        results[num_shot] = test_acc_step_list
    return results


def main(argv=None):
    parser = argparse.ArgumentParser(description="linear-probe CLIP: few-shot logistic regression on saved features (lpclip/linear_probe.py)")
    parser.add_argument("--trainval_dataset", type=str, default="", help="path to dataset")
    parser.add_argument("--test_dataset", type=str, default="", help="path to dataset")
    parser.add_argument("--num_step", type=int, default=8, help="number of steps")
    parser.add_argument("--num_run", type=int, default=3, help="number of runs")
    parser.add_argument("--feature_dir", type=str, default="clip_feat", help="feature dir path")
    args = parser.parse_args(argv)
    linear_probe(args.trainval_dataset, args.test_dataset, num_step=args.num_step, num_run=args.num_run, feature_dir=args.feature_dir)


if __name__ == "__main__":
    main()
