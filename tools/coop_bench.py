"""Timing of the CoOp step (trainers/coop.py) on one MI355X: forward + cross-entropy + backward w.r.t. the context + SGD.

    python tools/coop_bench.py [--steps 10] [--rounds 3]
Shapes: the reference's script shape (scripts/coop/*.sh: ViT-B/32, batch 32, N_CTX 4, 50 classes, end) and the ImageNet shape (ViT-B/16,
batch 32, N_CTX 16, 1000 classes; shared and CSC, end and middle), bf16.  Then, in the same process and alternating round by round, a CoOp
step (shared context, end) against a MuDPT step (depth 12) at equal n_ctx 4 on ViT-B/16, batch 32, 1000 classes: at this shape both text
towers run the same sequences, so CoOp's work is a strict subset (no vision backward, no deep prompts).  Synthetic images, random-init CLIP."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import synth
from mudpt_amd.model import CustomCLIP, ModelShape


def make(variant, patch, n_ctx, C, B, position="end"):
    shape = ModelShape(patch=patch, n_ctx=n_ctx, depth=12 if variant == "mudpt" else 1)
    tok = synth.synthetic_tokenized_prompts(C, n_ctx)
    kw = {}
    if variant != "mudpt":  # "<X x n> <name> ." : the name runs from row 1 + n to the row before "." (EOT - 1)
        kw = dict(class_token_position=position, name_lens=(tok.long().argmax(-1) - 2 - n_ctx).tolist())
    return CustomCLIP(shape, synth.random_clip_state(shape, 0), tok, max_batch=B, dtype="bf16", seed=1, variant=variant, **kw)


def timed(m, images, labels, steps):
    def step():
        m.forward_backward(images, labels)
        m.sgd_step(0.002)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    B = 32
    g = torch.Generator().manual_seed(0)
    images = torch.randn(B, 3, 224, 224, generator=g).cuda()
    for name, variant, patch, n_ctx, C, pos in (("script   ViT-B/32 n_ctx 4  C 50   end   ", "coop", 32, 4, 50, "end"),
                                                ("imagenet ViT-B/16 n_ctx 16 C 1000 end   ", "coop", 16, 16, 1000, "end"),
                                                ("imagenet ViT-B/16 n_ctx 16 C 1000 middle", "coop", 16, 16, 1000, "middle"),
                                                ("imagenet ViT-B/16 n_ctx 16 C 1000 end   CSC", "coop_csc", 16, 16, 1000, "end"),
                                                ("imagenet ViT-B/16 n_ctx 16 C 1000 middle CSC", "coop_csc", 16, 16, 1000, "middle")):
        labels = torch.randint(0, C, (B,), generator=g).cuda()
        m = make(variant, patch, n_ctx, C, B, pos)
        timed(m, images, labels, 3)
        ms = min(timed(m, images, labels, a.steps) for _ in range(a.rounds))
        print(f"CoOp {name} B={B} bf16: {ms:.2f} ms/step, {B / ms * 1e3:.0f} images/s (text rows {m.text_layout()[0]})", flush=True)
        m.close()
    # equal n_ctx: CoOp (shared, end) against MuDPT (depth 12), alternating
    labels = torch.randint(0, 1000, (B,), generator=g).cuda()
    ms = {"coop": [], "mudpt": []}
    models = {v: make(v, 16, 4, 1000, B) for v in ("coop", "mudpt")}
    for m in models.values():
        timed(m, images, labels, 3)
    for _ in range(a.rounds):
        for v, m in models.items():
            ms[v].append(timed(m, images, labels, a.steps))
    for v, m in models.items():
        print(f"equal n_ctx 4, ViT-B/16 B={B} C=1000 bf16: {'CoOp  (shared, end)' if v == 'coop' else 'MuDPT (depth 12)   '} "
              f"{min(ms[v]):.2f} ms/step (rounds {', '.join(f'{x:.2f}' for x in ms[v])}), text rows {m.text_layout()[0]}", flush=True)
        m.close()
    print(f"CoOp / MuDPT step time: {min(ms['coop']) / min(ms['mudpt']):.3f}")


if __name__ == "__main__":
    main()
