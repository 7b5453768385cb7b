"""Timing of the custom-loss step (CustomCLIP.differentiable, mudpt_forward_train / mudpt_backward_logits) and of its head kernel
(mudpt_head_grad) on one MI355X.  One process, warmed up; the versions of a measurement alternate round by round; median (min .. max) of the rounds.

    python tools/custom_loss_bench.py [--steps 10] [--iters 200] [--classes 11 50 ...] [--rounds 5]
Step, bf16 MuDPT on a random-init ViT-B/16 at the script shape (batch 4, 50 classes) and at batch 256 / 11 classes, wall clock around `steps` steps:
    fused           model.forward_backward(images, labels)                                        the library's one call
    differentiable  model.differentiable(images) + F.cross_entropy(out.logits, labels) + backward  the same tower work, the head in two halves,
                                                                                                   torch's autograd and the bucket accumulate
and the split step's own pieces (forward, loss + autograd + backward) with a device synchronisation between them.
Kernel, at (B, C, e) = (256, 1000, 512) and (32, 1000, 1024) and, for the dispatch rule, over the class counts of --classes at (256, C, 512),
(4, C, 512) and (32, C, 1024); device events around back-to-back calls:
    mudpt_head_grad path 2 (fused: head_dimg_kernel + head_dtxt_kernel) against path 1 (unfused: sgemm twice + a row kernel twice), and which
    of the two path 0 (the dispatch) takes."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from mudpt_amd import capi, synth
from mudpt_amd.model import CustomCLIP, ModelShape


def fmt(v, unit="ms"):
    return f"{statistics.median(v):8.3f} {unit} (rounds {min(v):.3f} .. {max(v):.3f})"


def make(C, B):
    shape = ModelShape(n_ctx=4, depth=12)
    return CustomCLIP(shape, synth.random_clip_state(shape, 0), synth.synthetic_tokenized_prompts(C, 4), max_batch=B, dtype="bf16", seed=1)


def wall(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def step_bench(B, C, a):
    g = torch.Generator().manual_seed(0)
    images, labels = torch.randn(B, 3, 224, 224, generator=g).cuda(), torch.randint(0, C, (B,), generator=g).cuda()
    m = make(C, B)
    pieces = {"forward": 0.0, "backward": 0.0}

    def fused():
        m.forward_backward(images, labels)

    def custom():
        m.flat_grads.zero_()
        F.cross_entropy(m.differentiable(images).logits, labels).backward()

    def custom_in_pieces():
        m.flat_grads.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.differentiable(images)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        F.cross_entropy(out.logits, labels).backward()
        torch.cuda.synchronize()
        pieces["forward"] += (t1 - t0) * 1e3
        pieces["backward"] += (time.perf_counter() - t1) * 1e3

    fns = {"fused": fused, "differentiable": custom}
    for fn in fns.values():
        wall(fn, 3)
    fused()
    want = m.flat_grads.clone()
    custom()
    torch.cuda.synchronize()
    rel = ((m.flat_grads - want).norm() / want.norm()).item()
    assert rel < 0.05, rel  # what is timed computes the fused step's gradient (bf16: the two heads round differently)
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            ms[k].append(wall(fn, a.steps))
    tag = f"ViT-B/16 bf16 B={B} C={C}"
    for k in fns:
        print(f"[{tag}] {k:15s} {fmt(ms[k])} per step", flush=True)
    for _ in range(a.steps):
        custom_in_pieces()
    d = statistics.median(ms["differentiable"]) - statistics.median(ms["fused"])
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"[{tag}] differentiable - fused = {d:+.3f} ms ({statistics.median(ms['differentiable']) / statistics.median(ms['fused']):.3f} x); largest spread of the "
          f"rounds {spread:.3f} ms; synchronised pieces of the split step: forward {pieces['forward'] / a.steps:.3f} ms, loss + autograd + backward "
          f"{pieces['backward'] / a.steps:.3f} ms; bucket {m.flat_grads.numel() * 4 / 1e6:.2f} MB; gradient vs the fused step's: {rel:.2e} relative", flush=True)
    m.close()
    torch.cuda.empty_cache()


def kernel_bench(B, C, e, a):
    g = torch.Generator().manual_seed(B + C + e)
    img, txt = torch.randn(B, e, generator=g), torch.randn(C, e, generator=g)
    t = {"img_n": img / img.norm(dim=1, keepdim=True), "img_inv": 1 / img.norm(dim=1), "txt_n": txt / txt.norm(dim=1, keepdim=True), "txt_inv": 1 / txt.norm(dim=1),
         "G": (torch.softmax(3 * torch.randn(B, C, generator=g), 1) - F.one_hot(torch.randint(0, C, (B,), generator=g), C)) / B}
    t = {k: v.float().cuda().contiguous() for k, v in t.items()}
    out = {p: (torch.empty(B, e, device="cuda"), torch.empty(C, e, device="cuda")) for p in (2, 1)}
    s = torch.cuda.current_stream().cuda_stream

    def call(path):
        return capi.call("mudpt_head_grad", **t, ldg=C, scale=14.2857, gmul=128.0 * B, B=B, C=C, e=e, dimg=out[path][0], dtxt=out[path][1], path=path, stream=s)

    for p in (2, 1):
        for _ in range(10):
            assert call(p) == 0, capi.load().mudpt_last_error().decode()
    torch.cuda.synchronize()
    for x, y in zip(out[2], out[1]):  # the two forms computed the same thing
        assert (x - y).abs().max().item() <= 2e-5 * y.pow(2).mean().sqrt().item()
    taken = ctypes.c_int32(-1)
    assert capi.call("mudpt_head_grad", **t, ldg=C, scale=14.2857, gmul=128.0 * B, B=B, C=C, e=e, dimg=out[1][0], dtxt=out[1][1], path=0,
                     path_taken=ctypes.byref(taken), stream=s) == 0
    us = {2: [], 1: []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(a.rounds):
        for p in (2, 1):
            ev[0].record()
            for _ in range(a.iters):
                call(p)
            ev[1].record()
            torch.cuda.synchronize()
            us[p].append(ev[0].elapsed_time(ev[1]) / a.iters * 1e3)
    tag = f"head_grad B={B} C={C} e={e}"
    print(f"[{tag}] fused (path 2)   {fmt(us[2], 'us')}", flush=True)
    print(f"[{tag}] unfused (path 1) {fmt(us[1], 'us')}", flush=True)
    print(f"[{tag}] fused / unfused = {statistics.median(us[2]) / statistics.median(us[1]):.2f}; the dispatch takes the {'fused' if taken.value == 0 else 'unfused'} form",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--classes", type=int, nargs="*", default=[11, 50, 100, 200, 400], help="class counts of the dispatch sweep (none: no sweep)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("custom_loss_bench: no GPU: nothing is measured without one")
    capi.load()
    for B, C, e in [(256, 1000, 512), (32, 1000, 1024)] + [(B, C, e) for B, e in ((256, 512), (4, 512), (32, 1024)) for C in a.classes]:
        kernel_bench(B, C, e, a)
    for B, C in ((4, 50), (256, 11)):
        step_bench(B, C, a)


if __name__ == "__main__":
    main()
