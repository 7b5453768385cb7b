"""Timing of CoOp / CoCoOp training steps on CLIP's ResNet image tower (mudpt_create_resnet) and of the training head without an image
gradient, on one MI355X: random-init weights, synthetic images.  A measurement, not a test: nothing here is a bound.

    python tools/resnet_train_bench.py [--dtype fp16] [--iters 5] [--rounds 5] [--skip-steps] [--skip-heads]

One process, alternating rounds (a, b, c, a, b, c, ...): median and min-max of `rounds` rounds of `iters` device-synchronised calls.
  steps  CoOp forward_backward at B 32, N_CTX 16, with 1000 and with 100 classes, on RN50, on RN50 with the fused convolutions
         (set_resnet_conv_path(1): one mudpt_conv2d launch per convolution) and on the ViT-B/16 handle; CoCoOp on RN50 at B 1 with 100 classes (the
         reference script's batch)
  heads  mudpt_head_ex in training, e = 1024: at (B, C) = (32, 1000) and (256, 1000) the fused head without dimg against the unfused launchers,
         without dimg and with it (where a training call with dimg lands at these shapes); at (32, 496), where both fused forms fit, the
         fused head with and without dimg.  A call includes the export's own scratch allocation and stream synchronisation, the same for
         every form."""
import argparse
import ctypes as C
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mudpt_amd import capi, synth
from mudpt_amd.model import CustomCLIP, ModelShape


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(fns, iters, rounds):
    for fn in fns.values():
        fn(); fn()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters))
    return ms


def report(tag, ms):
    print(f"{tag}: " + "; ".join(f"{k} {statistics.median(v):8.3f} ms ({min(v):.3f}-{max(v):.3f})" for k, v in ms.items()), flush=True)


def steps(dtype, iters, rounds):
    rn50 = ModelShape(**synth.RESNET_SHAPES["RN50"], n_ctx=16, depth=1)
    vit = ModelShape(n_ctx=16, depth=1)
    states = {"RN50": (rn50, synth.random_clip_state(rn50, 0)), "ViT-B/16": (vit, synth.random_clip_state(vit, 0))}
    g = torch.Generator().manual_seed(0)
    images = torch.randn(32, 3, 224, 224, generator=g).cuda()
    for n_cls in (1000, 100):
        tok = synth.synthetic_tokenized_prompts(n_cls, 16)  # "X .. X <name>." with name lengths mixed like ImageNet's; class token at the end
        labels = torch.randint(0, n_cls, (32,), generator=g).cuda()
        models = {k: CustomCLIP(s, sd, tok, max_batch=32, dtype=dtype, seed=1, variant="coop") for k, (s, sd) in states.items()}
        models["RN50 fused conv"] = CustomCLIP(*states["RN50"], tok, max_batch=32, dtype=dtype, seed=1, variant="coop")
        models["RN50"].set_resnet_conv_path(0)  # whatever MUDPT_RN_FUSED_CONV says
        models["RN50 fused conv"].set_resnet_conv_path(1)
        for m in models.values():
            m.train()
        ms = alternate({k: (lambda m=m: m.forward_backward(images, labels)) for k, m in models.items()}, iters, rounds)
        report(f"CoOp step B=32 C={n_cls} N_CTX=16 {dtype}", ms)
        for m in models.values():
            m.close()
        del models
        torch.cuda.empty_cache()
    shape = dataclasses.replace(rn50, n_ctx=4)
    tok = synth.synthetic_tokenized_prompts(100, 4)
    m = CustomCLIP(shape, states["RN50"][1], tok, max_batch=1, dtype=dtype, seed=1, variant="cocoop")
    m.train()
    lab = torch.tensor([7]).cuda()
    report(f"CoCoOp step B=1 C=100 N_CTX=4 {dtype}", alternate({"RN50": lambda: m.forward_backward(images[:1], lab)}, iters, rounds))
    m.close()


def heads(iters, rounds):
    lib = capi.load()
    P = capi.ptr
    e = 1024
    for B, Cn, forms in ((32, 1000, ("fused, no dimg", "unfused, no dimg", "unfused, dimg")), (256, 1000, ("fused, no dimg", "unfused, no dimg", "unfused, dimg")),
                         (32, 496, ("fused, no dimg", "fused, dimg", "unfused, no dimg"))):
        g = torch.Generator().manual_seed(B + Cn)
        img, txt = (torch.randn(B, e, generator=g) * 3).cuda(), (torch.randn(Cn, e, generator=g) * 0.2).cuda()
        lab = torch.randint(0, Cn, (B,), generator=g).cuda()
        txt_n, txt_inv, logits = torch.empty(Cn, e, device="cuda"), torch.empty(Cn, device="cuda"), torch.empty(B, Cn, device="cuda")
        loss, rows, dimg, dtxt = torch.empty(1, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, e, device="cuda"), torch.empty(Cn, e, device="cuda")

        def call(form):
            taken = C.c_int32(-1)
            rc = lib.mudpt_head_ex(P(img), P(txt), P(lab), 100.0, 1.0, B, 0, Cn, e, P(txt_n), P(txt_inv), P(logits), P(loss), P(rows),
                                   P(dimg) if form.endswith(", dimg") else None, P(dtxt), 1 if form.startswith("unfused") else 0, C.byref(taken), None)
            capi.check(rc, "head_ex")
            assert taken.value == (1 if form.startswith("unfused") else 0), (form, taken.value)
        report(f"training head B={B} C={Cn} e={e}", alternate({f: (lambda f=f: call(f)) for f in forms}, iters, rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-heads", action="store_true")
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if not a.skip_heads:
        heads(a.iters, a.rounds)
    if not a.skip_steps:
        steps(a.dtype, a.iters, a.rounds)


if __name__ == "__main__":
    main()
