"""What comes right after the logits: ranked predictions with their softmax probabilities (CLIP's ``(100 * img @ txt.T).softmax(-1).topk(5)``),
the rank of every label, and Dassl's ``compute_accuracy(output, target, topk=(1,))`` (dassl/metrics/accuracy.py, which all nine reference
trainers import).

"Top" is one total order on the columns of a row, the evaluator's (include/mudpt.h at mudpt_topk): column a precedes column b iff z[a] is NaN
and (z[b] is not NaN or a < b), or neither is NaN and (z[a] > z[b] or (z[a] == z[b] and a < b)); +0 == -0.  It is what
``torch.sort(z, 1, descending=True, stable=True)`` gives on the CPU -- NOT ``torch.topk``, which returns ties in no defined order -- and its
first place is ``DeviceClassification``'s prediction.  The rank of a label is the number of columns that precede it.

CUDA logits: ONE launch of mudpt_topk / mudpt_rank_accumulate (csrc/topk.hip) on the current stream, no transfer and no sync; logits that are
not fp32 are widened on the device first, as the evaluator does.  CPU logits: the same results restated with the stable sort, the reference
the tests hold the kernels to (there is no kernel to fall back from: the tensors' device chooses).
"""
from __future__ import annotations

import torch

from . import capi

MAX_K = 64          # a lane of the wave per output
MAX_STRIDE = 2 ** 31 - 1


def _check(logits, k, what):
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"{what}: logits {tuple(logits.shape)} are not [B, C] with B, C >= 1")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k = {k} is outside 1 .. {MAX_K}")
    if k > logits.shape[1]:
        raise ValueError(f"{what}: k = {k} is more than the {logits.shape[1]} classes")


def _device_logits(logits):
    """fp32 with unit column stride and a row stride the library takes, without a copy where the tensor already is that."""
    z = logits.detach()
    z = z if z.dtype == torch.float32 else z.float()
    if z.stride(1) != 1 or z.stride(0) < z.shape[1] or z.stride(0) > MAX_STRIDE:
        z = z.contiguous()
    return z


def _stable_order(logits):
    """(values, indices) of every row in the order, all C places: the CPU's stable descending sort in float32."""
    return torch.sort(logits.detach().float().cpu(), dim=1, descending=True, stable=True)


@torch.no_grad()
def topk(logits, k, probabilities=False, values=False):
    """The first ``k`` columns of every row of ``logits`` [B, C] in the order: ``index`` [B, k] int64.  With ``probabilities`` and / or
    ``values`` a tuple ``(index, prob, value)`` without the parts not asked for: ``prob`` [B, k] fp32, the softmax of the WHOLE row at those
    columns (NaN for a row that holds a NaN, a +inf or only -inf, as torch.softmax), ``value`` [B, k] fp32, the logits there."""
    _check(logits, k, "topk")
    B, C = logits.shape
    if logits.is_cuda:
        z = _device_logits(logits)
        index = torch.empty(B, k, dtype=torch.int32, device=z.device)
        prob = torch.empty(B, k, dtype=torch.float32, device=z.device) if probabilities else None
        value = torch.empty(B, k, dtype=torch.float32, device=z.device) if values else None
        with torch.cuda.device(z.device):
            capi.check(capi.call("mudpt_topk", logits=z, ldz=z.stride(0), rows=B, n_cls=C, k=k, index=index, value=value, prob=prob,
                                 stream=torch.cuda.current_stream(z.device).cuda_stream), "topk")
        index = index.long()
    else:
        z = logits.detach().float()
        sorted_values, order = _stable_order(z)
        index = order[:, :k].contiguous()
        prob = torch.softmax(z, dim=1).gather(1, index) if probabilities else None
        value = sorted_values[:, :k].contiguous() if values else None
    out = (index,) + ((prob,) if probabilities else ()) + ((value,) if values else ())
    return out if len(out) > 1 else index


@torch.no_grad()
def label_ranks(logits, labels):
    """``rank`` [B] int64: the number of columns of row b that precede column ``labels[b]`` (0: the label is the prediction), -1 for a label
    outside [0, C)."""
    _check(logits, 1, "label_ranks")
    B, C = logits.shape
    if labels.dim() != 1 or labels.shape[0] != B:
        raise ValueError(f"label_ranks: labels {tuple(labels.shape)} are not [{B}]")
    if logits.is_cuda:
        return _rank_accumulate(logits, labels, 1, want_rank=True)[1]
    y = labels.detach().to(torch.int64).cpu()
    order = _stable_order(logits)[1]
    place = torch.empty_like(order)
    place.scatter_(1, order, torch.arange(C).expand(B, C))  # the inverse permutation: place[b, order[b, r]] = r
    valid = (y >= 0) & (y < C)
    return torch.where(valid, place.gather(1, y.clamp(0, C - 1).unsqueeze(1)).squeeze(1), torch.full_like(y, -1))


def _rank_accumulate(logits, labels, kmax, want_rank=False, state=None):
    """One mudpt_rank_accumulate launch: (state int32 [2 + kmax] = total, invalid, hist, and the ranks as int64 or None).  ``state``: add to it."""
    z = _device_logits(logits)
    B, C = z.shape
    y = labels.detach().to(device=z.device, dtype=torch.int64).contiguous()
    if state is None:
        state = torch.zeros(2 + kmax, dtype=torch.int32, device=z.device)
    rank = torch.empty(B, dtype=torch.int32, device=z.device) if want_rank else None
    with torch.cuda.device(z.device):
        capi.check(capi.call("mudpt_rank_accumulate", logits=z, ldz=z.stride(0), labels=y, rows=B, n_cls=C, kmax=kmax, state=state, rank=rank,
                             stream=torch.cuda.current_stream(z.device).cuda_stream), "rank_accumulate")
    return state, (rank.long() if want_rank else None)


@torch.no_grad()
def compute_accuracy(output, target, topk=(1,)):
    """Dassl's ``compute_accuracy``: ``output`` the logits [B, C], or a tuple / list whose first item they are; ``target`` [B]; returns a list
    with, per k of ``topk``, a 1-element float tensor on the logits' device: 100 x (rows whose label is among the first k) / B.  A label
    outside [0, C) is among nothing.  max(topk) <= 64.  CUDA: one launch with kmax = max(topk), then the prefix sums of its histogram as a
    device op; nothing comes to the host."""
    if isinstance(output, (tuple, list)):
        output = output[0]
    topk = tuple(int(k) for k in topk)
    if not topk:
        raise ValueError("compute_accuracy: topk is empty")
    kmax = max(topk)
    _check(output, kmax, "compute_accuracy")
    _check(output, min(topk), "compute_accuracy")
    B = output.shape[0]
    if target.dim() != 1 or target.shape[0] != B:
        raise ValueError(f"compute_accuracy: target {tuple(target.shape)} is not [{B}]")
    if output.is_cuda:
        state, _ = _rank_accumulate(output, target, kmax)
        hits = state[2:].cumsum(0)
    else:
        rank = label_ranks(output, target)
        hits = torch.bincount(rank[(rank >= 0) & (rank < kmax)], minlength=kmax).cumsum(0)
    return [hits[k - 1:k].float().mul_(100.0 / B) for k in topk]
