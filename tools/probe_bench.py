"""Timing of the linear probe (mudpt_amd/lpclip.py: LogisticProbe over csrc/probe.hip and mudpt_amd/lbfgs.py) on one MI355X, synthetic features.
One process, warmed up, device-synchronised timing; the two versions of an evaluation alternate round by round, median and spread of the rounds.

    python tools/probe_bench.py [--iters 20] [--rounds 7] [--shapes 1000x16x512,100x16x512] [--no-sklearn]
Per shape (classes x shots x features; N = classes x shots rows):
(a) one objective evaluation (f and its gradient): the probe's kernels, and beside them, in the same process and alternating, the same
    evaluation built from the exports the library had before -- mudpt_sgemm for Z = X W^T + b and for dW = P^T X + beta W, mudpt_colsum for db
    -- around the same row kernel.  Results of the two are compared at the timed size.
(b) each GEMM form alone (device events around back-to-back launches), as TF/s of its 2 M N K, new and old;
(c) one full fit at C = 1: iterations, evaluations, ms per iteration split into evaluator (evaluations x (a)) and driver (the rest: the
    direction, the dot products the host needs, one host synchronisation per evaluation), library launches per iteration;
(d) 100 classes only, where sklearn is importable: LogisticRegression(solver="lbfgs", max_iter=1000, C=1) on 16 CPU threads."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mudpt_amd import capi, lpclip

MFMA_F32_PEAK = 157.3e12  # FLOP/s, v_mfma_f32_32x32x2_f32 on 256 compute units (specification)


def synthetic(n_cls, shots, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n_cls, K, generator=g) * 0.05
    y = torch.arange(n_cls).repeat_interleave(shots)
    X = mu[y] + torch.randn(n_cls * shots, K, generator=g) * 0.04  # rows of norm about 1.4, like unnormalised CLIP features scaled down
    perm = torch.randperm(len(y), generator=g)
    return X[perm].contiguous(), y[perm].contiguous()


class OldLogistic:
    """The evaluation of lpclip.HipLogistic from mudpt_sgemm / mudpt_colsum (16 x 16 tiles read straight from memory; one thread per column
    walking all rows) and the same row kernel."""

    def __init__(self, X, labels, n_cls, C):
        self.new = lpclip.HipLogistic(X, labels, n_cls, C)

    def value_and_grad(self, x):
        n = self.new
        nW, s = n.nW, torch.cuda.current_stream().cuda_stream
        n.x32.copy_(x)
        W, b = n.x32[:nW], n.x32[nW:]
        ck = capi.check
        ck(capi.call("mudpt_sgemm", transA=0, transB=1, M=n.N, N=n.n_cls, K=n.K, alpha=1.0, A=n.X, lda=n.K, B=W, ldb=n.K, beta=0.0, C=n.Z, ldc=n.n_cls, bias=b, stream=s))
        lpclip.probe_rows(n.Z, n.labels, n.row_loss, n.loss_sum)
        n.g32[:nW].copy_(W)
        ck(capi.call("mudpt_sgemm", transA=1, transB=0, M=n.n_cls, N=n.K, K=n.N, alpha=1.0, A=n.Z, lda=n.n_cls, B=n.X, ldb=n.K, beta=float(np.float32(n.reg)),
                     C=n.g32, ldc=n.K, bias=None, stream=s))
        ck(capi.call("mudpt_colsum", A=n.Z, M=n.N, N=n.n_cls, lda=n.n_cls, out=n.g32[nW:], accumulate=0, stream=s))
        f = n.loss_sum[0] / n.N + (0.5 * n.reg) * torch.dot(x[:nW], x[:nW])
        return f, n.g32.to(torch.float64)


def time_rounds(fns, iters, rounds):
    """fns: {name: callable}; the callables alternate round by round.  Returns {name: [ms per call of each round]}."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / iters * 1e3)
    return out


def event_rounds(fns, iters, rounds):
    """the same with device events around back-to-back launches"""
    out = {k: [] for k in fns}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(rounds):
        for name, fn in fns.items():
            ev[0].record()
            for _ in range(iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]) / iters)
    return out


def fmt(ms):
    return f"{statistics.median(ms):8.3f} ms (rounds {min(ms):.3f} .. {max(ms):.3f})"


def bench_shape(n_cls, shots, K, a):
    X, y = synthetic(n_cls, shots, K)
    N = n_cls * shots
    tag = f"{n_cls} x {shots} x {K}"
    Xd, yd = X.cuda(), y.int().cuda()
    new, old = lpclip.HipLogistic(Xd, yd, n_cls, 1.0), OldLogistic(Xd, yd, n_cls, 1.0)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(new.numel(), generator=g, dtype=torch.float64) * 0.5).cuda()
    # the two agree at the timed size (reordered fp32 sums: last bits)
    (f_new, g_new), (f_old, g_old) = new.value_and_grad(x), old.value_and_grad(x)
    print(f"[{tag}] new against old at the timed point: f {float(f_new):.9f} / {float(f_old):.9f}, max |g_new - g_old| {float((g_new - g_old).abs().max()):.2e} "
          f"of max |g| {float(g_old.abs().max()):.2e}", flush=True)
    # (a)
    for fn in (new, old):
        for _ in range(3):
            fn.value_and_grad(x)
    ms = time_rounds({"new": lambda: new.value_and_grad(x), "old": lambda: old.value_and_grad(x)}, a.iters, a.rounds)
    med = {k: statistics.median(v) for k, v in ms.items()}
    flop = 2 * 2.0 * N * n_cls * K
    print(f"(a) [{tag}] evaluation, probe kernels   {fmt(ms['new'])}  = {flop / med['new'] / 1e9:6.1f} TF/s of the two GEMMs' 2 x {flop / 2e9:.1f} GFLOP, "
          f"{new.slices} slices in the gradient GEMM", flush=True)
    print(f"(a) [{tag}] evaluation, sgemm + colsum  {fmt(ms['old'])}  = {flop / med['old'] / 1e9:6.1f} TF/s", flush=True)
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"(a) [{tag}] old / new = {med['old'] / med['new']:.2f}; difference of the medians {med['old'] - med['new']:.3f} ms against a run-to-run spread of {spread:.3f} ms",
          flush=True)
    # (b)
    W, b = new.x32[:new.nW].view(n_cls, K), new.x32[new.nW:]
    Z = torch.randn(N, n_cls, device="cuda") / N
    dW, db, s = new.g32[:new.nW].view(n_cls, K), new.g32[new.nW:], torch.cuda.current_stream().cuda_stream
    fns = {
        "nt new": lambda: lpclip.probe_gemm_nt(Xd, W, b, new.Z),
        "nt old": lambda: capi.call("mudpt_sgemm", transA=0, transB=1, M=N, N=n_cls, K=K, alpha=1.0, A=Xd, lda=K, B=W, ldb=K, beta=0.0, C=new.Z, ldc=n_cls, bias=b, stream=s),
        "tn new": lambda: lpclip.probe_gemm_tn(Z, Xd, dW, beta=0.5, W=W, db=db, scratch=new.scratch, slices=new.slices),
        "tn old": lambda: capi.call("mudpt_sgemm", transA=1, transB=0, M=n_cls, N=K, K=N, alpha=1.0, A=Z, lda=n_cls, B=Xd, ldb=K, beta=0.0, C=dW, ldc=K, bias=None, stream=s),
        "colsum old": lambda: capi.call("mudpt_colsum", A=Z, M=N, N=n_cls, lda=n_cls, out=db, accumulate=0, stream=s),
    }
    for fn in fns.values():
        fn()
    ev = event_rounds(fns, a.iters, a.rounds)
    for name, v in ev.items():
        m = statistics.median(v)
        rate = "" if name.startswith("colsum") else f" = {flop / 2 / m / 1e9:6.1f} TF/s ({flop / 2 / m / 1e9 / (MFMA_F32_PEAK / 1e12) * 100:4.1f} % of the fp32 matrix peak)"
        print(f"(b) [{tag}] {name:10s} {fmt(v)}{rate}", flush=True)
    # (c)
    clf = lpclip.LogisticProbe(C=1.0)
    clf.fit(Xd, y)  # warm
    fits = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf.fit(Xd, y)
        torch.cuda.synchronize()
        fits.append((time.perf_counter() - t0) * 1e3)
    r = clf.result_
    fit_ms = statistics.median(fits)
    per_iter, ev_iter = fit_ms / max(r.n_iter, 1), r.n_eval / max(r.n_iter, 1) * med["new"]
    print(f"(c) [{tag}] one fit at C = 1: {fit_ms:8.1f} ms (three fits {min(fits):.1f} .. {max(fits):.1f}), {r.n_iter} iterations, {r.n_eval} evaluations, {r.message}; "
          f"train accuracy {clf.score(Xd, y):.3f}", flush=True)
    print(f"(c) [{tag}] per iteration {per_iter:6.3f} ms = evaluator {ev_iter:6.3f} + driver {per_iter - ev_iter:6.3f}; library launches per iteration "
          f"{lpclip.HipLogistic.LAUNCHES * r.n_eval / max(r.n_iter, 1):.1f} ({lpclip.HipLogistic.LAUNCHES} per evaluation); the driver adds about 14 torch launches per "
          f"evaluation (casts, the regulariser, y, two small products, the packed transfer) and 5 per iteration (the direction, the kept pair), whatever "
          f"the number of pairs; one host synchronisation per evaluation", flush=True)
    # (d)
    if n_cls <= 100 and not a.no_sklearn:
        try:
            from sklearn.linear_model import LogisticRegression
            from threadpoolctl import threadpool_limits
        except ImportError:
            print("(d) sklearn is not importable here: not measured", flush=True)
            return
        Xn, yn = X.numpy(), y.numpy()
        with threadpool_limits(limits=16):
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                sk = LogisticRegression(solver="lbfgs", max_iter=1000, C=1.0).fit(Xn, yn)
                times.append((time.perf_counter() - t0) * 1e3)
        dev = np.abs(sk.coef_ - clf.coef_).max() / np.abs(sk.coef_).max()
        print(f"(d) [{tag}] sklearn on 16 CPU threads: {statistics.median(times):8.1f} ms per fit ({min(times):.1f} .. {max(times):.1f}), {int(sk.n_iter_[0])} iterations; "
              f"the probe's coefficients differ by {dev:.2e} of max|coef| ({int(clf.n_iter_[0])} iterations)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="1000x16x512,100x16x512")
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_bench: no GPU: nothing is measured without one")
    capi.load()
    for shape in a.shapes.split(","):
        bench_shape(*(int(v) for v in shape.split("x")), a)


if __name__ == "__main__":
    main()
