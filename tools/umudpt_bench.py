"""Timing of the UMuDPT step (trainers/umudpt.py) on one MI355X against MuDPT's at equal prompt shape: forward + cross-entropy + backward +
SGD, bf16, synthetic images, random-init CLIP ViT-B/16, n_ctx 2, depth 8 (train.py:122-126).

    python tools/umudpt_bench.py [--steps 20] [--rounds 5]
Shapes: the script shape (batch 4, 50 classes) and batch 256 with 11 classes.  At each shape the two models live in one process and are
timed alternately, round by round, after a warm-up; the MEDIAN over the rounds is reported with the rounds themselves.  The prompt
generator's forward + backward alone (mudpt_promptgen_forward / _backward: the code the model path runs, 11 + 11 launches on 16 rows) is
timed the same way, and so are the MuDPT prompt learner's launches it replaces (the difference of the two steps bounds what shows)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import capi, synth
from mudpt_amd.model import CustomCLIP, ModelShape

N_CTX, DEPTH = 2, 8


def make(variant, C, B):
    shape = ModelShape(n_ctx=N_CTX, depth=DEPTH)
    tok = synth.synthetic_tokenized_prompts(C, N_CTX)
    return CustomCLIP(shape, synth.random_clip_state(shape, 0), tok, max_batch=B, dtype="bf16", seed=1, variant=variant)


def timed(m, images, labels, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.forward_backward(images, labels)
        m.sgd_step(0.002)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def generator_alone(steps, rounds):
    """ms per forward + backward of the generator at the default shape (16 rows of 512 -> 768), median over the rounds."""
    lib = capi.load()
    d, dv, R = 512, 768, DEPTH * N_CTX
    g = torch.Generator().manual_seed(0)
    n = lib.mudpt_promptgen_param_numel(d, dv)
    params = (0.03 * torch.randn(n, generator=g)).cuda()
    X, dG = (0.02 * torch.randn(R, d, generator=g)).cuda(), torch.randn(R, dv, generator=g).cuda()
    G, dX, grads = torch.empty(R, dv, device="cuda"), torch.empty(R, d, device="cuda"), torch.empty(n, device="cuda")
    ws_n = lib.mudpt_promptgen_workspace(DEPTH, N_CTX, d, dv)
    ws = torch.empty(ws_n, device="cuda")
    P = capi.ptr

    def once():
        capi.check(lib.mudpt_promptgen_forward(DEPTH, N_CTX, d, dv, P(params), P(X), P(G), P(ws), ws_n, None), "promptgen_forward")
        capi.check(lib.mudpt_promptgen_backward(DEPTH, N_CTX, d, dv, P(params), P(X), P(dG), P(dX), P(grads), P(ws), ws_n, None), "promptgen_backward")
    for _ in range(10):
        once()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps * 10):
            once()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / (steps * 10) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("umudpt_bench needs an MI355X: a timing without the GPU says nothing")
    g = torch.Generator().manual_seed(0)
    for B, C in ((4, 50), (256, 11)):
        images = torch.randn(B, 3, 224, 224, generator=g).cuda()
        labels = torch.randint(0, C, (B,), generator=g).cuda()
        models = {v: make(v, C, B) for v in ("umudpt", "mudpt")}
        for m in models.values():
            timed(m, images, labels, 5)
        ms = {v: [] for v in models}
        for _ in range(a.rounds):
            for v, m in models.items():
                ms[v].append(timed(m, images, labels, a.steps))
        med = {v: statistics.median(ms[v]) for v in models}
        for v in models:
            print(f"ViT-B/16 B={B:3d} C={C:4d} bf16 n_ctx {N_CTX} depth {DEPTH} {v.upper():6s} median {med[v]:7.3f} ms/step "
                  f"(rounds {', '.join(f'{x:.3f}' for x in ms[v])}), {B / med[v] * 1e3:.0f} images/s", flush=True)
        print(f"B={B} C={C}: UMuDPT / MuDPT {med['umudpt'] / med['mudpt']:.3f} ({med['umudpt'] - med['mudpt']:+.3f} ms)", flush=True)
        for m in models.values():
            m.close()
        del models
        torch.cuda.empty_cache()
    gen = generator_alone(a.steps, a.rounds)
    print(f"generator alone (depth {DEPTH}, n_ctx {N_CTX}, 512 -> 768): forward + backward median {statistics.median(gen):.3f} ms "
          f"(rounds {', '.join(f'{x:.3f}' for x in gen)}), 22 launches", flush=True)


if __name__ == "__main__":
    main()
