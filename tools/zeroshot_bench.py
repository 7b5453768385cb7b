"""Timing of the zero-shot path (trainers/zsclip.py over a frozen handle, mudpt_create_frozen) on one MI355X, random-init CLIP ViT-B/16,
synthetic images and prompts.  One process, warmed up, device-synchronised timing, medians of 5 rounds.

    python tools/zeroshot_bench.py [--iters 10] [--rounds 5] [--only a|b]
(a) evaluation throughput: 1000 classes, batch 100 (the reference's test batch) and 256, in all three modes; beside it, in the same process, a
    CoOp handle's eval forward with MUDPT_FWD_REUSE_TEXT at the same shape -- the closest inference path without the frozen handle, and the
    same vision forward.
(b) text-feature build: 1000 classes, 7 and 80 templates (prompt lengths: synth.synthetic_tokenized_prompts' mix, one draw per template):
    total and per template; the embed kernel alone on one template's rows, as achieved bytes/s (rows x d x 4 x 2 plus the position table
    once) against the HBM peak; and the host alternative for one template: index the fp32 table on the host, add the positions, copy to the
    device."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import capi, synth
from mudpt_amd.model import CustomCLIP, ModelShape
from mudpt_amd.zsclip import FrozenCLIP

HBM_PEAK = 8.0e12      # bytes/s, HBM3E specification of the MI355X
HBM_COPY = 6.29e12     # bytes/s, what a float4 streaming copy reaches on it


def median_ms(fn, iters, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(out), out


def tokens_for(C_, T):
    return torch.stack([synth.synthetic_tokenized_prompts(C_, 4, seed=7 + t) for t in range(T)])


def eval_throughput(state, shape, a):
    g = torch.Generator().manual_seed(0)
    Cn = 1000
    tok = tokens_for(Cn, 1)
    for B in (100, 256):
        images = torch.randn(B, 3, 224, 224, generator=g).cuda()
        for dtype in ("bf16", "fp16", "fp32"):
            zs = FrozenCLIP(shape, state, tok, max_batch=B, dtype=dtype)
            coop = CustomCLIP(ModelShape(n_ctx=4, depth=1), state, tok[0], max_batch=B, dtype=dtype, seed=1, variant="coop")
            coop.eval()
            for m in (zs, coop):  # warm up; the second CoOp forward reuses its text features
                m(images); m(images)
            ms = {}
            for name, m in (("frozen", zs), ("coop_reuse_text", coop)):
                ms[name], rounds = median_ms(lambda m=m: m(images), a.iters, a.rounds)
                print(f"(a) ViT-B/16 C={Cn} B={B:3d} {dtype:4s} {name:16s} {ms[name]:7.2f} ms/forward ({B / ms[name] * 1e3:7.0f} images/s; rounds "
                      f"{', '.join(f'{x:.2f}' for x in rounds)})", flush=True)
            print(f"(a) B={B} {dtype}: frozen / CoOp with reused text {ms['frozen'] / ms['coop_reuse_text']:.3f}", flush=True)
            zs.close(); coop.close()
            del zs, coop
            torch.cuda.empty_cache()


def text_build(state, shape, a):
    Cn, d = 1000, shape.t_width
    lib = capi.load()
    for T in (7, 80):
        tok = tokens_for(Cn, T)
        m = FrozenCLIP(shape, state, tok, max_batch=1, dtype="fp16")
        rows, buckets, max_len = m.text_layout()
        bias = state["ln_final.bias"]

        def rebuild():
            m.set_weight("ln_final.bias", bias)  # invalidates the kept features (a host-side copy of 2 KB)
            m.text_features()
        rebuild()
        ms, rounds = median_ms(rebuild, 1 if T > 7 else 3, a.rounds)
        print(f"(b) text features C={Cn} T={T:2d} fp16: {ms:8.2f} ms total, {ms / T:6.2f} ms per template ({rows} token rows, <= {buckets} buckets, "
              f"longest {max_len}; rounds {', '.join(f'{x:.1f}' for x in rounds)})", flush=True)
        m.close()
    # the embed kernel alone on one template's packed rows
    r1 = rows // 80
    g = torch.Generator().manual_seed(1)
    table = state["token_embedding.weight"].float().cuda()
    pos = state["positional_embedding"].float().cuda()
    ids = torch.randint(0, table.shape[0], (r1,), generator=g, dtype=torch.int32).cuda()
    p = (torch.arange(r1, dtype=torch.int32) % 9).cuda()
    out = torch.empty(r1, d, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: capi.check(lib.mudpt_embed_tokens(capi.ptr(table), table.shape[0], capi.ptr(ids), capi.ptr(p), capi.ptr(pos), capi.ptr(out), r1, d, s))  # noqa: E731
    call()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = []
    for _ in range(a.rounds):
        ev[0].record()
        for _ in range(50):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        per.append(ev[0].elapsed_time(ev[1]) / 50)
    us = statistics.median(per) * 1e3
    nbytes = r1 * d * 4 * 2 + pos.numel() * 4
    print(f"(b) embed kernel, {r1} rows x {d}: {us:7.2f} us per launch (back to back, stream order), {nbytes / 1e6:.1f} MB -> {nbytes / us / 1e6:.2f} TB/s = "
          f"{nbytes / us * 1e6 / HBM_PEAK * 100:.0f} % of the HBM peak ({HBM_PEAK / 1e12:.1f} TB/s; a streaming copy reaches {HBM_COPY / 1e12:.2f}); the "
          f"{table.numel() * 4 / 1e6:.0f} MB table fits the 256 MiB Infinity Cache, so re-read rows need not come from HBM", flush=True)
    # the host alternative for one template: what mudpt_set_class_prompts' callers do today
    emb_w, pos_h, tok1 = state["token_embedding.weight"].float(), state["positional_embedding"].float(), tok[0].long()

    def host():
        x = emb_w[tok1] + pos_h
        return x.cuda()
    host()
    hms, rounds = median_ms(host, 1, a.rounds)
    print(f"(b) host alternative, one template [{Cn}, 77, {d}] ({Cn * 77 * d * 4 / 1e6:.0f} MB): index + add + copy to the device {hms:8.1f} ms "
          f"(rounds {', '.join(f'{x:.1f}' for x in rounds)})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    a = ap.parse_args()
    shape = ModelShape(n_ctx=0, depth=1)
    state = synth.random_clip_state(shape, 0)
    if a.only != "b":
        eval_throughput(state, shape, a)
    if a.only != "a":
        text_build(state, shape, a)


if __name__ == "__main__":
    main()
