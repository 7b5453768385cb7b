"""Timing of top-k on the device (mudpt_amd/csrc/topk.hip) on one MI355X.  One process, warmed up; the versions of a measurement alternate round
by round, median and spread of the rounds; device events around back-to-back launches.

    python tools/topk_bench.py [--iters 2000] [--rounds 5] [--k 5]
At 256 x 1000, 100 x 1000, 256 x 11 and 256 x 2048 (above 1027 columns mudpt_topk walks the row again in every round instead of keeping it in registers):
    mudpt_topk             index, value and the softmax probabilities of the first k columns, one launch
    mudpt_rank_accumulate  the labels' ranks into the histogram (top-k accuracy for every k <= kmax), one launch
beside, on the device: torch.softmax(z, 1) + torch.topk (two launches and a [rows, C] intermediate: CLIP's recipe as torch runs it; ties in no
defined order), mudpt_eval_accumulate (the evaluator's one arg-max launch), and a device copy of the same logits."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import capi

SHAPES = ((256, 1000), (100, 1000), (256, 11), (256, 2048))


def fmt(v, unit):
    return f"{statistics.median(v):9.3f} {unit} (rounds {min(v):.3f} .. {max(v):.3f})"


def event_rounds(fns, iters, rounds):
    """fns: {name: callable}; they alternate round by round.  {name: [microseconds per call of each round]}, device events around back-to-back calls."""
    out = {k: [] for k in fns}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(rounds):
        for name, fn in fns.items():
            ev[0].record()
            for _ in range(iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]) / iters * 1e3)
    return out


def bench(rows, n_cls, a):
    k = min(a.k, n_cls)
    g = torch.Generator().manual_seed(rows + n_cls)
    z, y = (torch.randn(rows, n_cls, generator=g) * 8.0).cuda(), torch.randint(0, n_cls, (rows,), generator=g).cuda()
    index = torch.empty(rows, k, dtype=torch.int32, device="cuda")
    value, prob = (torch.empty(rows, k, dtype=torch.float32, device="cuda") for _ in range(2))
    ranks = torch.zeros(2 + k, dtype=torch.int32, device="cuda")
    state = torch.zeros(capi.call("mudpt_eval_state_numel", n_cls=n_cls, with_cmat=0), dtype=torch.int32, device="cuda")
    dst, s = torch.empty_like(z), torch.cuda.current_stream().cuda_stream
    kept = {}

    def torch_pair():
        kept["topk"] = torch.softmax(z, 1).topk(k)
    fns = {"topk": lambda: capi.call("mudpt_topk", logits=z, ldz=n_cls, rows=rows, n_cls=n_cls, k=k, index=index, value=value, prob=prob, stream=s),
           "rank": lambda: capi.call("mudpt_rank_accumulate", logits=z, ldz=n_cls, labels=y, rows=rows, n_cls=n_cls, kmax=k, state=ranks, stream=s),
           "torch": torch_pair,
           "eval": lambda: capi.call("mudpt_eval_accumulate", logits=z, ldz=n_cls, labels=y, rows=rows, n_cls=n_cls, state=state, with_cmat=0, stream=s),
           "copy": lambda: dst.copy_(z)}
    for name, fn in fns.items():
        for _ in range(10):
            rc = fn()
            assert not isinstance(rc, int) or rc == 0, (name, capi.load().mudpt_last_error().decode())  # a launcher's code
    ranks.zero_()
    state.zero_()
    us = event_rounds(fns, a.iters, a.rounds)
    torch.cuda.synchronize()
    # what was timed computed the right thing: the same columns as torch's pair on tie-free logits, the evaluator's counts in the histogram
    assert torch.equal(index.long(), kept["topk"][1]) and int(ranks[0]) == int(state[0]) == rows * a.iters * a.rounds and int(ranks[2]) == int(state[1])
    tag = f"{rows} x {n_cls}"
    labels = {"topk": f"mudpt_topk k = {k}, with prob", "rank": f"mudpt_rank_accumulate kmax = {k}", "torch": "torch.softmax + torch.topk",
              "eval": "mudpt_eval_accumulate", "copy": "device copy of the logits"}
    for name, label in labels.items():
        print(f"[{tag:>10s}] {label:34s} {fmt(us[name], 'us')}", flush=True)
    med = {name: statistics.median(v) for name, v in us.items()}
    spread = max(max(v) - min(v) for v in us.values())
    print(f"[{tag:>10s}] topk / torch's pair = {med['topk'] / med['torch']:.2f}, rank / eval_accumulate = {med['rank'] / med['eval']:.2f}, "
          f"topk / copy = {med['topk'] / med['copy']:.2f}; largest spread of the rounds {spread:.3f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench: no GPU: nothing is measured without one")
    capi.load()
    for rows, n_cls in SHAPES:
        bench(rows, n_cls, a)


if __name__ == "__main__":
    main()
