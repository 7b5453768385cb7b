"""The test pass's evaluator on the device: Dassl's ``Classification`` (dassl/evaluation/evaluator.py -- accuracy, error rate, macro-F1,
TEST.PER_CLASS_RESULT's table, TEST.COMPUTE_CMAT's cmat.pt) without its per-batch device-to-host traffic.

Dassl's evaluator copies every prediction and label to Python lists (and calls .item() once per sample for the per-class table), then
hands them to sklearn.  Here ``process`` is ONE launch of mudpt_eval_accumulate (csrc/evaluate.hip) on the current stream that adds
integer counts to a state buffer in device memory, and ``evaluate`` is one mudpt_eval_finalize plus one transfer of six doubles (and of the
3 C per-class counts / the C x C matrix when asked for).  Every number is the one sklearn's f1_score(average="macro",
labels=np.unique(y_true)) and confusion_matrix(normalize="true") give, called the way Dassl calls them
(tests/golden/evaluator_sklearn.npz); the prediction is torch.max(logits, 1)[1]'s CPU rule, Dassl's ``mo.max(1)[1]``.

``evaluator`` = None (by the tensors: CUDA -> "hip", CPU -> "torch"), "hip" (needs the GPU; no fallback) or "torch" (the same counts
restated with torch.bincount on the host: the reference the tests hold the kernels to).  Merging ranks is not built: the state is integers,
so an all-reduce of it before finalize would be exact.

``topk`` = (3, 5) (opt-in; dassl_lite.build_evaluator fills it from MUDPT_TEST_TOPK=3,5) adds top-k accuracy, the second number of CLIP's
ImageNet tables: ``process`` makes one more launch, mudpt_rank_accumulate (csrc/topk.hip), into a second small state [total, invalid,
hist[max k]] of the labels' ranks, and ``evaluate`` adds ``top{k}_accuracy`` = 100 x sum(hist[:k]) / total.  The two kernels rank by one order, so
hist[0] is ``correct``: ``evaluate`` raises if they differ.  Without it nothing changes: the same launches, keys and printed text.
"""
from __future__ import annotations

import os.path as osp
from collections import OrderedDict

import torch

from . import capi, metrics

MAX_ROWS = 2 ** 31 - 1  # the counts are int32
HEAD = 4                # total, correct, invalid, reserved
RANK_HEAD = 2           # the rank state: total, invalid, then hist[max k]


class DeviceClassification:
    """Dassl's EvaluatorBase protocol: ``reset()``, ``process(mo, gt)`` per batch, ``evaluate() -> OrderedDict``.  The class count is
    len(lab2cname) when given, else the width of the first logits; the state is allocated by the first ``process``."""

    def __init__(self, cfg, lab2cname=None, evaluator=None, topk=(), **kwargs):
        if evaluator not in (None, "hip", "torch"):
            raise ValueError(f"unknown evaluator {evaluator!r}")
        self._topk = tuple(int(k) for k in topk)
        if any(not 1 <= k <= metrics.MAX_K for k in self._topk):
            raise ValueError(f"topk = {self._topk}: every k must lie in 1 .. {metrics.MAX_K}")
        if lab2cname is not None:
            self._check_topk(len(lab2cname))
        self.cfg, self._lab2cname, self.evaluator = cfg, lab2cname, evaluator
        test = getattr(cfg, "TEST", None)
        self._per_class = bool(getattr(test, "PER_CLASS_RESULT", False))
        self._with_cmat = bool(getattr(test, "COMPUTE_CMAT", False))
        if self._per_class:
            assert lab2cname is not None  # dassl/evaluation/evaluator.py: the table prints class names
        self._n_cls = len(lab2cname) if lab2cname is not None else None
        self._state = self._kind = self._rank_state = None
        self._rows = 0
        self.last = None  # after evaluate(): the six numbers of mudpt_eval_finalize by name

    def _check_topk(self, n_cls):
        if self._topk and max(self._topk) > n_cls:
            raise ValueError(f"topk = {self._topk}: k = {max(self._topk)} is more than the {n_cls} classes")

    # -- the state ---------------------------------------------------------------------------------------------------
    def state_numel(self, n_cls: int) -> int:
        if self._with_cmat and n_cls * n_cls >= 2 ** 31:
            raise AssertionError(f"a confusion matrix of {n_cls} x {n_cls} cells does not fit 2^31")
        return HEAD + 3 * n_cls + (n_cls * n_cls if self._with_cmat else 0)

    def reset(self):
        self._rows = 0
        if self._state is None:
            return
        if self._kind == "hip":
            with torch.cuda.device(self._state.device):
                capi.check(capi.call("mudpt_eval_reset", state=self._state, n_cls=self._n_cls, with_cmat=int(self._with_cmat),
                                     stream=torch.cuda.current_stream(self._state.device).cuda_stream), "eval_reset")
        else:
            self._state.zero_()
        if self._rank_state is not None:
            self._rank_state.zero_()

    def _prepare(self, mo, gt):
        if mo.dim() != 2 or gt.dim() != 1 or gt.shape[0] != mo.shape[0] or mo.shape[0] < 1 or mo.shape[1] < 1:
            raise ValueError(f"process: logits {tuple(mo.shape)} and labels {tuple(gt.shape)} are not [B, C] and [B] with B, C >= 1")
        kind = self.evaluator or ("hip" if mo.is_cuda else "torch")
        if kind == "hip" and not (mo.is_cuda and gt.is_cuda):
            raise capi.MudptError('the "hip" evaluator counts on the GPU: logits and labels must be CUDA tensors (there is no fallback)')
        if self._n_cls is None:
            self._check_topk(mo.shape[1])
            self._n_cls = mo.shape[1]
        if mo.shape[1] != self._n_cls:
            raise ValueError(f"process: logits of {mo.shape[1]} classes, the evaluator counts {self._n_cls}")
        if self._state is not None and (kind != self._kind or (kind == "hip" and self._state.device != mo.device)):
            raise ValueError("process: the batches of one pass must stay on one device and one evaluator")
        if self._rows + mo.shape[0] > MAX_ROWS:
            raise ValueError(f"process: {self._rows} + {mo.shape[0]} rows are more than the {MAX_ROWS} the int32 counts hold")
        if self._state is None:
            numel = self.state_numel(self._n_cls)
            self._kind = kind
            if kind == "hip":
                self._state = torch.empty(numel, dtype=torch.int32, device=mo.device)
                self.reset()
            else:
                self._state = torch.zeros(numel, dtype=torch.int64)
            if self._topk:
                self._rank_state = torch.zeros(RANK_HEAD + max(self._topk), dtype=self._state.dtype, device=self._state.device)
        return kind

    # -- the protocol ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def process(self, mo, gt):
        """mo: logits [B, C]; gt: labels [B].  "hip": one launch on the current stream, no transfer, no sync."""
        kind = self._prepare(mo, gt)
        C, B = self._n_cls, mo.shape[0]
        if kind == "hip":
            z = mo if mo.dtype == torch.float32 else mo.float()
            if z.stride(1) != 1 or z.stride(0) < C or z.stride(0) > MAX_ROWS:
                z = z.contiguous()
            y = gt.to(torch.int64).contiguous()
            with torch.cuda.device(z.device):
                capi.check(capi.call("mudpt_eval_accumulate", logits=z, ldz=z.stride(0), labels=y, rows=B, n_cls=C, state=self._state,
                                     with_cmat=int(self._with_cmat), stream=torch.cuda.current_stream(z.device).cuda_stream), "eval_accumulate")
                if self._topk:
                    capi.check(capi.call("mudpt_rank_accumulate", logits=z, ldz=z.stride(0), labels=y, rows=B, n_cls=C, kmax=max(self._topk),
                                         state=self._rank_state, stream=torch.cuda.current_stream(z.device).cuda_stream), "rank_accumulate")
        else:
            z, y = mo.detach().float().cpu(), gt.detach().to(torch.int64).cpu()
            self._accumulate_torch(z, y)
            if self._topk:
                self._accumulate_ranks_torch(z, y)
        self._rows += B

    def _accumulate_torch(self, z, y):
        """mudpt_eval_accumulate restated: the same cells of the same layout, as int64 on the host."""
        C, s = self._n_cls, self._state
        p = z.max(1)[1]
        valid = (y >= 0) & (y < C)
        y, p = y[valid], p[valid]
        s[0] += int(valid.sum())
        s[1] += int((p == y).sum())
        s[2] += int((~valid).sum())
        s[HEAD:HEAD + C] += torch.bincount(y, minlength=C)
        s[HEAD + C:HEAD + 2 * C] += torch.bincount(p, minlength=C)
        s[HEAD + 2 * C:HEAD + 3 * C] += torch.bincount(y[p == y], minlength=C)
        if self._with_cmat:
            s[HEAD + 3 * C:] += torch.bincount(y * C + p, minlength=C * C)

    def _accumulate_ranks_torch(self, z, y):
        """mudpt_rank_accumulate restated: the labels' ranks by the stable sort, the same cells as int64 on the host."""
        s, kmax = self._rank_state, max(self._topk)
        rank = metrics.label_ranks(z, y)
        s[0] += int((rank >= 0).sum())
        s[1] += int((rank < 0).sum())
        s[RANK_HEAD:] += torch.bincount(rank[(rank >= 0) & (rank < kmax)], minlength=kmax)

    def _finalize_torch(self):
        """mudpt_eval_finalize restated in float64."""
        C, s = self._n_cls, self._state
        support, predicted, hit = (s[HEAD + k * C:HEAD + (k + 1) * C].double() for k in range(3))
        on = support > 0
        n = int(on.sum())
        f1 = float((2.0 * hit[on] / (support[on] + predicted[on])).sum() / n * 100.0) if n else 0.0
        acc = float((100.0 * hit[on] / support[on]).sum() / n) if n else 0.0
        return [float(s[0]), float(s[1]), float(s[2]), float(n), f1, acc]

    def counts(self):
        """(head [4], support, predicted, hit [C] each) as int64 host tensors: a transfer, for tests and tools."""
        if self._state is None:
            raise ValueError("counts: nothing was processed")
        C, s = self._n_cls, self._state[:HEAD + 3 * self._n_cls].cpu().long()
        return s[:HEAD], s[HEAD:HEAD + C], s[HEAD + C:HEAD + 2 * C], s[HEAD + 2 * C:]

    def evaluate(self):
        results = OrderedDict()
        C = self._n_cls
        if self._state is None:  # no batch at all: zeros, never NaN
            six, per_class, cmat = [0.0] * 6, None, None
            if C is not None:
                per_class = torch.zeros(3 * C, dtype=torch.int64)
                cmat = torch.zeros(C, C, dtype=torch.int64)
        else:
            if self._kind == "hip":
                out = torch.empty(6, dtype=torch.float64, device=self._state.device)
                with torch.cuda.device(out.device):
                    capi.check(capi.call("mudpt_eval_finalize", state=self._state, n_cls=C, results=out,
                                         stream=torch.cuda.current_stream(out.device).cuda_stream), "eval_finalize")
                six = out.cpu().tolist()
            else:
                six = self._finalize_torch()
            per_class = self._state[HEAD:HEAD + 3 * C].cpu().long() if self._per_class else None
            cmat = self._state[HEAD + 3 * C:].cpu().long().view(C, C) if self._with_cmat else None
        total, correct, invalid = int(six[0]), int(six[1]), int(six[2])
        if invalid > 0:
            raise ValueError(f"evaluate: {invalid} labels lie outside [0, {C}): they were counted as invalid and in nothing else")
        acc = 100.0 * correct / total if total else 0.0
        err = 100.0 - acc if total else 0.0
        macro_f1 = six[4]
        self.last = {"total": total, "correct": correct, "invalid": invalid, "n_supported": int(six[3]), "macro_f1": macro_f1, "perclass_accuracy": six[5]}
        results["accuracy"], results["error_rate"], results["macro_f1"] = acc, err, macro_f1
        topk_lines = ""
        if self._topk:
            ranks = self._rank_state.cpu().tolist() if self._rank_state is not None else [0] * (RANK_HEAD + max(self._topk))
            if ranks[0] != total or ranks[1] != invalid or ranks[RANK_HEAD] != correct:  # one order in both kernels: a difference is a bug
                raise RuntimeError(f"evaluate: the rank state counts total {ranks[0]}, invalid {ranks[1]}, rank 0 {ranks[RANK_HEAD]}; "
                                   f"the evaluator's state counts total {total}, invalid {invalid}, correct {correct}")
            for k in self._topk:
                results[f"top{k}_accuracy"] = 100.0 * sum(ranks[RANK_HEAD:RANK_HEAD + k]) / total if total else 0.0
                topk_lines += f"\n* top{k}_accuracy: {results[f'top{k}_accuracy']:.1f}%"
        print("=> result\n"
              f"* total: {total:,}\n"
              f"* correct: {correct:,}\n"
              f"* accuracy: {acc:.1f}%\n"
              f"* error: {err:.1f}%\n"
              f"* macro_f1: {macro_f1:.1f}%" + topk_lines)
        if self._per_class:
            print("=> per-class result")
            if per_class is not None:
                support, hit = per_class[:C].tolist(), per_class[2 * C:].tolist()
                for label in range(C):  # Dassl lists the labels that occurred, sorted
                    if support[label] > 0:
                        print(f"* class: {label} ({self._lab2cname[label]})\ttotal: {support[label]:,}\tcorrect: {hit[label]:,}\t"
                              f"acc: {100.0 * hit[label] / support[label]:.1f}%")
            print(f"* average: {six[5]:.1f}%")
            results["perclass_accuracy"] = six[5]
        if self._with_cmat:
            save_path = osp.join(self.cfg.OUTPUT_DIR, "cmat.pt")
            torch.save(normalized_cmat(cmat) if cmat is not None else normalized_cmat(torch.zeros(0, 0, dtype=torch.int64)), save_path)
            print(f"Confusion matrix is saved to {save_path}")
        return results


def normalized_cmat(cmat: torch.Tensor):
    """sklearn's confusion_matrix(y_true, y_pred, normalize="true") from the full C x C counts: a float64 numpy array over the labels that
    occur in y_true or y_pred, each row divided by its support, a row without support left at zero."""
    used = ((cmat.sum(1) > 0) | (cmat.sum(0) > 0)).nonzero().reshape(-1)
    sub = cmat[used][:, used].double()
    support = sub.sum(1, keepdim=True)
    return torch.where(support > 0, sub / support.clamp(min=1.0), torch.zeros_like(sub)).numpy()


try:  # with the real framework: TEST.EVALUATOR "DeviceClassification" makes Dassl's SimpleTrainer.test() drive this class
    from dassl.evaluation import EVALUATOR_REGISTRY
    EVALUATOR_REGISTRY.register()(DeviceClassification)
except ImportError:
    pass
