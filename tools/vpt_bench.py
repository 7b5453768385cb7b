"""Timing of the VPT and MPT steps (trainers/vpt.py, trainers/mpt.py) on one MI355X against MuDPT's: forward + cross-entropy + backward +
SGD, bf16, synthetic images, random-init CLIP ViT-B/16.

    python tools/vpt_bench.py [--steps 10] [--rounds 3]
Shapes: the script shape (configs/trainers/VPT|MPT/vit_b16_c2_ep5_batch4.yaml: batch 4, 50 classes) and batch 256 with 11 and with 1000
classes.  VPT: DEEP_VISUAL_N_CTX 8, depth 12; MPT: 2 / 2 / 12 / 12; MuDPT: n_ctx 4, depth 12 (the yardstick).  At each shape the three
models live in one process and are timed alternately, round by round; the minimum over the rounds is reported."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import synth
from mudpt_amd.model import CustomCLIP, ModelShape

SHAPES = {"vpt": (0, 0, 8, 12), "mpt": (2, 12, 2, 12)}


def make(variant, C, B):
    shape = ModelShape(n_ctx=4, depth=12 if variant == "mudpt" else 1)
    tok = synth.synthetic_tokenized_prompts(C, 4)
    return CustomCLIP(shape, synth.random_clip_state(shape, 0), tok, max_batch=B, dtype="bf16", seed=1, variant=variant,
                      prompt_shape=SHAPES.get(variant))


def timed(m, images, labels, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.forward_backward(images, labels)
        m.sgd_step(0.002)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    for B, C in ((4, 50), (256, 11), (256, 1000)):
        images = torch.randn(B, 3, 224, 224, generator=g).cuda()
        labels = torch.randint(0, C, (B,), generator=g).cuda()
        models = {v: make(v, C, B) for v in ("vpt", "mpt", "mudpt")}
        for m in models.values():
            timed(m, images, labels, 3)
        ms = {v: [] for v in models}
        for _ in range(a.rounds):
            for v, m in models.items():
                ms[v].append(timed(m, images, labels, a.steps))
        for v, m in models.items():
            print(f"ViT-B/16 B={B:3d} C={C:4d} bf16 {v.upper():5s} {min(ms[v]):7.2f} ms/step (rounds {', '.join(f'{x:.2f}' for x in ms[v])}), "
                  f"{B / min(ms[v]) * 1e3:.0f} images/s", flush=True)
        print(f"B={B} C={C}: VPT / MuDPT {min(ms['vpt']) / min(ms['mudpt']):.3f}, MPT / MuDPT {min(ms['mpt']) / min(ms['mudpt']):.3f}", flush=True)
        for m in models.values():
            m.close()
        del models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
