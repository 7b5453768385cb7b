"""Timing of the UUMuDPT step (trainers/uumudpt.py) on one MI355X against UMuDPT's and MuDPT's at equal prompt shape: forward + cross-entropy +
backward + SGD, bf16, synthetic images, random-init CLIP ViT-B/16, n_ctx 2, depth 8 (train.py:129-133).

    python tools/uumudpt_bench.py [--steps 20] [--rounds 5]
Shapes: the script shape (batch 4, 50 classes) and batch 256 with 11 classes.  At each shape the three models live in one process and are
timed alternately, round by round, after a warm-up; the MEDIAN over the rounds is reported with the rounds themselves.  Each generator's
forward + backward alone (mudpt_promptgen_forward / _backward, the code the model path runs: 11 + 11 launches) is timed the same way: Gen1 on
the 16 rows of 512 -> 768, Gen2 on the 14 rows of 768 -> 512.  In the step the two chains run on the two streams beside each other and beside
the towers, so UUMuDPT's step should cost clearly less over UMuDPT's than Gen2's chain alone."""
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
VARIANTS = ("uumudpt", "umudpt", "mudpt")


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


def generator_alone(layers, d, d_out, steps, rounds):
    """ms per forward + backward of one generator on `layers` groups of N_CTX rows of width d, one figure per round."""
    lib = capi.load()
    R = layers * N_CTX
    g = torch.Generator().manual_seed(0)
    n = lib.mudpt_promptgen_param_numel(d, d_out)
    params = (0.03 * torch.randn(n, generator=g)).cuda()
    X, dG = (0.02 * torch.randn(R, d, generator=g)).cuda(), torch.randn(R, d_out, generator=g).cuda()
    G, dX, grads = torch.empty(R, d_out, device="cuda"), torch.empty(R, d, device="cuda"), torch.empty(n, device="cuda")
    ws_n = lib.mudpt_promptgen_workspace(layers, N_CTX, d, d_out)
    ws = torch.empty(ws_n, device="cuda")
    P = capi.ptr

    def once():
        capi.check(lib.mudpt_promptgen_forward(layers, N_CTX, d, d_out, P(params), P(X), P(G), P(ws), ws_n, None), "promptgen_forward")
        capi.check(lib.mudpt_promptgen_backward(layers, N_CTX, d, d_out, P(params), P(X), P(dG), P(dX), P(grads), P(ws), ws_n, None), "promptgen_backward")
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
        raise SystemExit("uumudpt_bench needs an MI355X: a timing without the GPU says nothing")
    g = torch.Generator().manual_seed(0)
    for B, C in ((4, 50), (256, 11)):
        images = torch.randn(B, 3, 224, 224, generator=g).cuda()
        labels = torch.randint(0, C, (B,), generator=g).cuda()
        models = {v: make(v, C, B) for v in VARIANTS}
        for m in models.values():
            timed(m, images, labels, 5)
        ms = {v: [] for v in models}
        for _ in range(a.rounds):
            for v, m in models.items():
                ms[v].append(timed(m, images, labels, a.steps))
        med = {v: statistics.median(ms[v]) for v in models}
        for v in models:
            print(f"ViT-B/16 B={B:3d} C={C:4d} bf16 n_ctx {N_CTX} depth {DEPTH} {v.upper():7s} median {med[v]:7.3f} ms/step "
                  f"(rounds {', '.join(f'{x:.3f}' for x in ms[v])}), {B / med[v] * 1e3:.0f} images/s", flush=True)
        print(f"B={B} C={C}: UUMuDPT - UMuDPT {med['uumudpt'] - med['umudpt']:+.3f} ms, UMuDPT - MuDPT {med['umudpt'] - med['mudpt']:+.3f} ms, "
              f"UUMuDPT / MuDPT {med['uumudpt'] / med['mudpt']:.3f}", flush=True)
        for m in models.values():
            m.close()
        del models
        torch.cuda.empty_cache()
    for name, layers, d, d_out in (("Gen1", DEPTH, 512, 768), ("Gen2", DEPTH - 1, 768, 512)):
        gen = generator_alone(layers, d, d_out, a.steps, a.rounds)
        print(f"{name} alone ({layers} layers of {N_CTX} rows, {d} -> {d_out}): forward + backward median {statistics.median(gen):.3f} ms "
              f"(rounds {', '.join(f'{x:.3f}' for x in gen)}), 22 launches", flush=True)


if __name__ == "__main__":
    main()
