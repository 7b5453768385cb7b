#!/usr/bin/env python3
"""Headline benchmark: MuDPT ViT-B/16 forward+backward(+SGD step) images/s, batch 256 per MI355X, bf16.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python bench.py --gpus 1 --steps 50 --warmup 10 --full                     # + roofline, HBM kernels, parity modes, CPU baselines
    python bench.py --gpus 1 --steps 50 --warmup 10 --dump-outputs DIR         # + the last timed step's outputs as DIR/*.npy
    python bench.py --gpus N --steps K --warmup W          # N > 1 with WORLD_SIZE unset: starts N fresh child processes itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = BASELINE.json configs[1]: forward + cross-entropy + backward through both prompted CLIP towers
for 256 synthetic 224x224 images and 11 class prompts (n_ctx 4, depth 12), the RCCL all-reduce of the 10
trainable tensors when N > 1, and the SGD update.  Inputs, weights and parameters are resident in HBM before
the timed region.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the headline line; every other figure (the HIP-event roofline of
the GEMMs and HBM-bound kernels, the parity-mode timings, the CPU baselines, the all-reduce timing at N > 1) is measured
only with --full.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between the ranks of a node needs it on this driver

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_MFMA_TFLOPS = 2500.0  # gfx950 dense bf16/fp16 MFMA peak (MI355X_MICROARCH.md, spec)


def flops_per_step(shape, B: int, C: int) -> float:
    """Algorithmic FLOPs of one step: per token per block GEMM 24 d^2 and attention 4 L d forward;
    backward = dX-only GEMMs (1x forward) + attention 2x forward; patch embed forward only; text tower once per step."""
    def tower(d, L, layers):
        return L * layers * (2 * 24 * d * d + 3 * 4 * L * d)
    P = (shape.image_size // shape.patch) ** 2
    Lv = 1 + P + shape.n_ctx
    vis = tower(shape.v_width, Lv, shape.v_layers) + 2 * P * (3 * shape.patch ** 2) * shape.v_width  # patch embed forward only
    txt = tower(shape.t_width, shape.ctx_len, shape.t_layers)
    return float(B) * vis + float(C) * txt


def cpu_baseline(n_cls: int = 11, iters: int = 12):
    """The CPU oracle (oracle/, a restatement of the reference's arithmetic pinned by tests/golden) timed on the host
    cores at BASELINE config 1's shape: ViT-B/16, n_ctx 4, depth 12, batch 4, fp32; n_cls = 11 (the benchmark's class list) or
    50 (Caltech-101's base split)."""
    from oracle import mudpt_oracle as O
    from mudpt_amd.synth import bench_tokenized_prompts, synthetic_tokenized_prompts, CTX_INIT_TOKENS
    # a one-GPU box owns a 16-core share of the host; more torch threads than that only oversubscribe it
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    cfg = O.VIT_B16
    frozen = O.make_frozen_state(cfg, 0)
    tok = (bench_tokenized_prompts() if n_cls == 11 else synthetic_tokenized_prompts(n_cls)).long()
    emb, eot = frozen["token_embedding.weight"][tok], tok.argmax(-1)
    params = O.make_trainable_state(cfg, 1, frozen, CTX_INIT_TOKENS)
    g = torch.Generator().manual_seed(1234)
    images, labels = torch.randn(4, 3, 224, 224, generator=g), torch.tensor([0, 3, 6, 9])
    times = []
    for i in range(2 + iters):
        t0 = time.perf_counter()
        O.forward_backward(cfg, frozen, params, emb, eot, images, labels)
        if i >= 2:
            times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    return {"value": round(4 / med, 3), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{iters} fwd+bwd iterations of BASELINE config 1 (batch 4, {n_cls} classes, fp32), median {med * 1e3:.0f} ms"}


PEAK_HBM_GBS = 8000.0  # HBM3E spec (MI355X_MICROARCH.md; ~6300 GB/s achievable by a streaming copy)
# tools/prof_join.py output of the same command under rocprofv3 (separate --pmc FETCH_SIZE / WRITE_SIZE passes; tools/profile_round.sh),
# committed per workload: (arch, batch, classes, dtype) -> profiles/<tag>_bytes_per_step.json
TRAFFIC_TAGS = {("vit_b16", 256, 11, "bf16"): "r04", ("vit_b16", 256, 11, "fp16"): "r04_fp16", ("vit_b16", 256, 11, "fp32"): "r04_fp32",
                ("vit_b16", 256, 1000, "bf16"): "r04_c1000", ("vit_l14_336", 128, 1000, "bf16"): "r04_vitl"}


def traffic_json(arch, B, C, dtype):
    tag = TRAFFIC_TAGS.get((arch, B, C, dtype))
    return os.path.join(ROOT, "profiles", f"{tag}_bytes_per_step.json") if tag else None


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): start N fresh child processes of this same command line, one per
    GPU -- RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, rendezvous on 127.0.0.1 -- and wait for them.  This parent has
    not touched the GPU (no HIP call, no torch.cuda.is_available()) and never replaces itself: the children are ordinary subprocesses.
    Rank 0's stdout (the ONE JSON line) is this process's stdout; every rank's stderr is passed on line by line behind a "[rank r]" prefix.
    Replaces nn.DataParallel's single-process fan-out (trainers/mudpt.py:230-233) at the bench level.

    The job has a DEADLINE (MUDPT_BENCH_DEADLINE_S, default 480 s): a rank that hangs in the rendezvous or in a collective is not a dead
    rank, so nothing else would ever end the job -- after the deadline the parent terminates the children it started (exact PIDs), says on
    stderr which ranks were still running and for how long, and exits 124."""
    import socket
    import subprocess
    import threading
    deadline_s = float(os.environ.get("MUDPT_BENCH_DEADLINE_S", "480"))
    with socket.socket() as sk:  # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs, pumps = [], []

    def pump(r, pipe):  # rank-prefixed stderr, line by line: what a hung or failing rank said last is on the parent's stderr
        for line in iter(pipe.readline, b""):
            sys.stderr.write(f"[rank {r}] " + line.decode(errors="replace"))
            sys.stderr.flush()
        pipe.close()

    t_start = time.monotonic()
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE))
        pumps.append(threading.Thread(target=pump, args=(r, procs[r].stderr), daemon=True))
        pumps[-1].start()
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    sys.stderr.write(f"bench.py: rank {r} exited with code {code} after {time.monotonic() - t_start:.0f} s; ending ranks {sorted(pending)}\n")
                    for q in pending:  # a dead rank leaves its peers in a collective: end them (exact PIDs we started)
                        procs[q].terminate()
            if pending and time.monotonic() - t_start > deadline_s:
                sys.stderr.write(f"bench.py: deadline of {deadline_s:.0f} s passed with ranks {sorted(pending)} of {n} still running "
                                 f"(hung in the rendezvous or a collective?); terminating them\n")
                for q in pending:
                    procs[q].terminate()
                t_kill = time.monotonic() + 10
                while any(procs[q].poll() is None for q in pending) and time.monotonic() < t_kill:
                    time.sleep(0.05)
                rc = 124
                break
            time.sleep(0.05)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
        for th in pumps:
            th.join(timeout=2)
    return rc


def rendezvous_timeout():
    """Timeout of init_process_group and of every collective of the bench (MUDPT_DIST_TIMEOUT_S, default 120 s)."""
    from datetime import timedelta
    return timedelta(seconds=float(os.environ.get("MUDPT_DIST_TIMEOUT_S", "120")))


def stub_worker(args, rank: int, world: int):
    """MUDPT_BENCH_STUB=1: the launcher / rendezvous / timing / JSON contract of the N > 1 path with a stand-in step (a CPU bucket of the
    real size, one all-reduce per step over gloo): what tests/test_bench_launcher_cpu.py drives, no GPU and no library involved.  The
    line it prints says "data": "stub" and carries no roofline: it is not a measurement."""
    import torch.distributed as dist
    if os.environ.get("MUDPT_BENCH_STUB_FAIL_RANK") == str(rank):
        raise SystemExit(3)  # test hook: a rank that dies before the rendezvous
    if os.environ.get("MUDPT_BENCH_STUB_HANG_RANK") == str(rank):
        print("stub rank: sleeping past the deadline", file=sys.stderr, flush=True)
        time.sleep(3600)  # test hook: a rank that hangs (alive, never reaches the rendezvous)
    if world > 1:
        dist.init_process_group("gloo", timeout=rendezvous_timeout())
    bucket = torch.full((1243136,), float(rank + 1))

    def fence():
        if world > 1:
            dist.barrier()
    for _ in range(args.warmup):
        if world > 1:
            dist.all_reduce(bucket)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        bucket.fill_(float(rank + 1))
        if world > 1:
            dist.all_reduce(bucket)
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    assert bucket[0].item() == world * (world + 1) / 2, "all-reduce(sum) over the ranks"
    if rank == 0:
        print(json.dumps({"metric": "images/sec fwd+bwd ViT-B/16 MuDPT", "value": round(world * args.batch * args.steps / elapsed, 2), "unit": "images/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "stub",
                          "config": {"workload": "launcher rehearsal: stand-in step, NOT a measurement", "global_batch": world * args.batch, "parallelism": f"dp{world}"},
                          "collective": {"backend": "gloo" if world > 1 else None, "world_size": world, "bucket_bytes": bucket.numel() * 4}}), flush=True)
    if world > 1:
        dist.destroy_process_group()


DUMP_BYTES = 64 << 20  # --dump-outputs: budget of all files together


def last_step_outputs(model, loss):
    """What a caller of the timed step holds after it: the loss (this rank's), the gradients of the trainable tensors (summed over the
    ranks at N > 1) and the tensors' values after the SGD update; host float32 copies, by name."""
    out = {"loss": loss.detach().float().reshape(1).cpu()}
    for k, p in model.named_parameters():
        out[f"grad.{k}"] = p.grad.detach().float().cpu().clone()
        out[f"param.{k}"] = p.detach().float().cpu().clone()
    return out


def dump_outputs(path: str, outputs) -> None:
    """DIR/<name>.npy per array, at most DUMP_BYTES in all.  Beyond that budget every array above 4096 elements keeps its share of it as
    a fixed sample: the flat elements at the sorted first indices of torch.randperm(numel, generator seeded 0) -- the same positions
    on every run and every build."""
    import math
    import numpy as np
    os.makedirs(path, exist_ok=True)
    total = sum(t.numel() for t in outputs.values()) * 4
    frac = min(1.0, (DUMP_BYTES - (1 << 20)) / total)
    for name, t in outputs.items():
        if frac < 1.0 and t.numel() > 4096:
            keep = math.ceil(t.numel() * frac)
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:keep].sort().values
            t = t.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), t.numpy().astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)   # 10 warm-up, >= 50 timed steps, the median next to the mean
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU")
    ap.add_argument("--classes", type=int, default=11)
    ap.add_argument("--arch", default="vit_b16", choices=["vit_b16", "vit_l14_336"], help="vit_l14_336 = BASELINE configs[4] (not the headline line)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"], help="bf16 = the throughput mode (headline); fp16 = fp16 operands (logits within "
                    "1e-3 at logit scale 14.29 only); fp32 = the parity mode (split operands: text tower fp16 pairs + fp32 attention, vision tower fp16 + "
                    "e4m3 remainders on the fp8 matrix pipe: 3.5e-4 at logit scale 100)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true", help="do not bracket GEMM launches with HIP events")
    ap.add_argument("--prof-stride", type=int, default=4, help="bracket every n-th persistent-GEMM launch with HIP events (1 = all; an event pair "
                    "costs ~4 us of queue time, and the launch counter runs across steps so every launch site is sampled equally often)")
    ap.add_argument("--gemm-variant", type=int, default=0, help="tuning knob passed to mudpt_model_set (A/B runs on one box)")
    ap.add_argument("--attn-two-kernels", action="store_true", help="attention backward as the round-1 dQ + dK/dV kernel pair (A/B of the single-sweep kernel)")
    ap.add_argument("--no-last-single", action="store_true", help="last block through the general attention kernels on all rows (A/B of the single-query path)")
    ap.add_argument("--class-parallel", action="store_true", help="N > 1: each rank encodes C / N class prompts (two extra [C, embed] sums per step); "
                    "meant for --classes 1000 (BASELINE configs[2])")
    ap.add_argument("--no-split-k", action="store_true", help="never split the contraction of the small-grid GEMMs (A/B at small batches)")
    ap.add_argument("--knob", action="append", default=[], metavar="NAME=VALUE", help="any mudpt_model_set knob (include/mudpt.h), e.g. --knob defer_reduce=0 (A/B runs)")
    ap.add_argument("--no-attn-window", action="store_true", help="block 0's attention backward on all rows (A/B of the prompt-row window form)")
    ap.add_argument("--txt-buckets", type=int, default=0, help="maximum number of length buckets of the class prompts (0 = library default 3; 1 = none)")
    ap.add_argument("--fp32-streams", action="store_true", help="keep the gradient stream (and in bf16 mode the update stream) in fp32 (A/B of the T streams)")
    ap.add_argument("--graph", action="store_true", help="replay forward+backward from a captured hipGraph (implies --no-profile)")
    ap.add_argument("--no-parity-mode", action="store_true", help="skip the short fp16 (parity configuration) timing appended to the bf16 line")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: roofline and HBM-kernel figures (HIP "
                    "events), parity-mode timings, CPU baselines, the all-reduce alone at N > 1 (--no-profile / --no-parity-mode / "
                    "--no-cpu-baseline drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed -- loss, the gradients and the updated "
                    "values of the trainable tensors -- as DIR/<name>.npy (float32; at most 64 MB, a seeded sample of each array beyond that)")
    args = ap.parse_args()
    if not args.full:
        args.no_profile = args.no_parity_mode = args.no_cpu_baseline = True

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus))  # the bare command: this process only starts and reaps the ranks
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world size and --gpus must agree")
    if os.environ.get("MUDPT_BENCH_STUB"):
        return stub_worker(args, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the MuDPT path has no CPU fallback")
    if os.environ.get("MUDPT_BENCH_ONE_DEVICE"):  # rehearsal of the N > 1 path on a one-GPU box: every rank on cuda:0, gloo collectives
        local = 0
    torch.cuda.set_device(local)
    if world > 1:  # N ranks build their (seeded, CPU-side) synthetic weights at the same time: share the host cores instead of oversubscribing them N-fold
        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
    dist = None
    if world > 1:
        import torch.distributed as dist
        # "nccl" is RCCL over xGMI on ROCm.  A bounded rendezvous / collective timeout: the default (10 min) is the driver's whole bench limit
        dist.init_process_group(os.environ.get("MUDPT_BENCH_BACKEND", "nccl"), timeout=rendezvous_timeout())

    from mudpt_amd.model import CustomCLIP, ModelShape
    from mudpt_amd import synth, capi, parallel
    knobs = {}
    if args.gemm_variant:
        knobs["gemm_variant"] = args.gemm_variant
    for kv in args.knob:
        knobs[kv.split("=")[0]] = int(kv.split("=")[1])
    if args.fp32_streams:
        knobs["lp_grad"] = 0
    if args.attn_two_kernels:
        knobs["attn_two_kernels"] = 1
    if args.txt_buckets:
        knobs["txt_buckets"] = args.txt_buckets
    if args.no_split_k:
        knobs["split_k"] = 0
    if args.no_attn_window:
        knobs["attn_window"] = 0
    if args.no_last_single:
        knobs["last_single"] = 0
    shape = ModelShape()  # CLIP ViT-B/16, n_ctx 4, depth 12
    if args.arch == "vit_l14_336":
        shape = ModelShape(image_size=336, patch=14, v_width=1024, v_layers=24, v_heads=16, t_width=768, t_layers=12, t_heads=12, embed_dim=768, n_ctx=4, depth=24)
    B, C = args.batch, args.classes
    tok = synth.bench_tokenized_prompts() if C == 11 else synth.synthetic_tokenized_prompts(C)
    model = CustomCLIP(shape, synth.random_clip_state(shape, seed=0), tok, ctx_token_ids=synth.CTX_INIT_TOKENS,
                       max_batch=B, dtype=args.dtype, device=f"cuda:{local}", seed=1, knobs=knobs,  # same seeds on every rank: replicas
                       class_shard=parallel.class_range(C, rank, world) if args.class_parallel and world > 1 else None)
    g = torch.Generator().manual_seed(1234 + rank)
    images = torch.randn(B, 3, shape.image_size, shape.image_size, generator=g).cuda()
    labels = torch.randint(0, C, (B,), generator=g).cuda()
    lr = 0.0025  # configs/trainers/MuDPT/vit_b16_bz4_ep10_nctx4_depth9.yaml OPTIM.LR

    graph = None
    if args.graph:
        args.no_profile = True
        for _ in range(2):  # first-use initialisation (function attributes, allocations) must happen outside the capture
            model.forward_backward(images, labels, grad_scale=1.0 / world)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            model.forward_backward(images, labels, grad_scale=1.0 / world)

    def step():
        if graph is not None:
            graph.replay()
            loss = model._loss[0]
        else:
            loss = model.forward_backward(images, labels, grad_scale=1.0 / world)
        if dist is not None:
            dist.all_reduce(model.flat_grads)  # ONE collective per step: the 4.97 MB bucket of the 10 trainable tensors
        model.sgd_step(lr, momentum=0.9, weight_decay=5e-4)
        return loss

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    stride = max(1, args.prof_stride)
    if not args.no_profile:
        model.set_knob("prof_stride", stride)
        model.profile(True)
    # one marker event per step on the stream the steps run on (the library launches on torch's current stream): per-step GPU times for
    # the median; `value` stays the wall clock of the whole window over K steps, as the contract says
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    for i in range(args.steps):
        marks[i].record()
        loss = step()
    marks[args.steps].record()
    fence()
    elapsed = time.perf_counter() - t0
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    median_ms = step_ms[len(step_ms) // 2]
    outputs = last_step_outputs(model, loss) if args.dump_outputs and rank == 0 else None  # before any further step moves them
    classes, exec_flop = model.profile_read_classes() if not args.no_profile else ({}, 0.0)
    gemm_ms, gemm_flop, gemm_n = classes.get("gemm_pp", (0.0, 0.0, 0))  # of the SAMPLED launches (every stride-th)
    model.profile(False)
    model.set_knob("prof_stride", 1)
    # The HBM-bound kernel classes (LayerNorm, attention) are measured in their own short pass AFTER the timed region: an event pair costs
    # ~5 us of queue time per bracketed launch, and bracketing all 157 big launches of a step slowed the timed steps by 0.8 ms (3 %).
    hbm_steps = 0
    if not args.no_profile and graph is None:
        hbm_steps = max(2, min(5, args.steps))
        model.profile(0b11110)
        for _ in range(hbm_steps):
            step()
        fence()
        hbm_classes, _ = model.profile_read_classes()
        model.profile(False)
        classes.update({k: v for k, v in hbm_classes.items() if k != "gemm_pp"})
    collective = None
    if dist is not None:
        t = torch.tensor([elapsed], device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
        collective = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "op": "all_reduce(sum) of the flat gradient bucket, one per step",
                      "bucket_bytes": model.flat_grads.numel() * 4}
    if dist is not None and args.full:
        # what the one collective of a step costs on its own: the 4.97 MB bucket, timed by events around dist.all_reduce (untimed extra calls)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
        dist.barrier()
        for e0, e1 in evs:
            e0.record()
            dist.all_reduce(model.flat_grads)
            e1.record()
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in evs)
        collective.update(allreduce_us_median=round(us[len(us) // 2], 1), allreduce_us_min=round(us[0], 1))
    loss_v = float(loss.item())
    if not (loss_v == loss_v) or abs(loss_v) == float("inf"):
        raise SystemExit(f"non-finite loss {loss_v}")
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs)
    model.close()
    del model

    # The parity configurations, timed on the same box right after the bf16 headline so that the driver's record carries them:
    #   parity ("fp32", include/mudpt.h MUDPT_F32): split forward GEMM operands -- text tower fp16 pairs + fp32 attention, vision tower fp16 + e4m3
    #       remainders contracted on the fp8 matrix pipe -- the mode that meets north_star's 1e-3 logit bound at the logit scale pretrained CLIP
    #       carries (100): tests/test_exact_gpu.py, max 3.5e-4 (the per-site ablation that chose it: DESIGN.md 2);
    #   fp16: fp16 operands, fp32 streams, split text-tower operands -- within 1e-3 at the init logit scale 14.29 only (4e-3 at 100).
    parity_ms = {}
    if rank == 0 and world == 1 and args.dtype == "bf16" and not args.no_parity_mode and not args.graph:
        for mode in ("fp32", "fp16", "fp32x"):
            pm = CustomCLIP(shape, synth.random_clip_state(shape, seed=0), tok, ctx_token_ids=synth.CTX_INIT_TOKENS, max_batch=B, dtype=mode[:4],
                            device=f"cuda:{local}", seed=1, knobs={"vis_lo": 1, "vis_exact_attn": 1} if mode == "fp32x" else None)
            for _ in range(3):
                pm.forward_backward(images, labels)
                pm.sgd_step(lr, momentum=0.9, weight_decay=5e-4)
            torch.cuda.synchronize()
            n_par = max(5, args.steps // (2 if mode != "fp32x" else 5))
            t1 = time.perf_counter()
            for _ in range(n_par):
                pm.forward_backward(images, labels)
                pm.sgd_step(lr, momentum=0.9, weight_decay=5e-4)
            torch.cuda.synchronize()
            parity_ms[mode] = (time.perf_counter() - t1) / n_par * 1e3
            pm.close()
            del pm

    if rank == 0:
        ms = elapsed / args.steps * 1e3
        step_flop = flops_per_step(shape, B, C)
        out = {
            "metric": "images/sec fwd+bwd ViT-B/16 MuDPT" if args.arch == "vit_b16" else "images/sec fwd+bwd ViT-L/14@336 MuDPT", "value": round(world * B * args.steps / elapsed, 2), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "ms_per_step_median": round(median_ms, 3),
            "ms_per_step_min": round(step_ms[0], 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"MuDPT {'ViT-B/16' if args.arch == 'vit_b16' else 'ViT-L/14@336'} fwd+bwd+SGD, batch {B}/GPU, {C} class prompts, n_ctx {shape.n_ctx}, depth {shape.depth}, "
                                   f"synthetic {shape.image_size}x{shape.image_size} N(0,1) images, random-init frozen CLIP (BASELINE configs[{1 if args.arch == 'vit_b16' else 4}])",
                       "global_batch": world * B, "parallelism": f"dp{world}" + ("+class-parallel text tower" if args.class_parallel and world > 1 else ""), "final_loss": round(loss_v, 4),
                       "step_tflop": round(step_flop / 1e12, 3)},
        }
        tj = traffic_json(args.arch, B, C, args.dtype)
        traffic_doc = json.load(open(tj)) if tj and os.path.exists(tj) else {}
        # stale-profile guard: the PMC passes were taken on the kernels whose source hash is stamped in the file (tools/profile_round.sh);
        # if the loaded library was built from other sources the byte counts are not this run's -> null
        from mudpt_amd import build as _build
        traffic_stale = bool(traffic_doc) and traffic_doc.get("source_hash") != _build.source_hash()
        traffic_db = {} if traffic_stale else traffic_doc.get("classes", {})
        if gemm_n:
            ach = gemm_flop / (gemm_ms * 1e-3) / 1e12
            # HBM-side bytes per launch come from separate rocprofv3 --pmc passes of this same command (PMC counters cannot be read from
            # inside the process); the joined summary is committed under profiles/ (tools/prof_join.py).
            pmc = traffic_db.get("gemm_pp")
            hbm = {}
            for cls in ("ln_fwd", "ln_bwd", "attn_fwd", "attn_bwd"):
                c_ms, c_bytes, c_n = classes.get(cls, (0.0, 0.0, 0))
                if not c_n:
                    continue
                gbs = c_bytes / (c_ms * 1e-3) / 1e9
                hbm[cls] = {"achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                            "algorithmic_bytes_per_launch": round(c_bytes / c_n), "launches_per_step": c_n // hbm_steps, "avg_launch_us": round(c_ms * 1e3 / c_n, 2),
                            "ms_per_step": round(c_ms / hbm_steps, 3),
                            "traffic": round(traffic_db[cls]["traffic_bytes_per_launch"]) if cls in traffic_db else None}
            out["roofline"] = {"bound": "mfma", "achieved": round(ach, 1), "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(ach / PEAK_MFMA_TFLOPS, 4), "traffic": round(pmc["traffic_bytes_per_launch"]) if pmc else None,
                               "traffic_unit": "bytes/launch (2 x FETCH_SIZE + WRITE_SIZE of separate --pmc passes: " + (os.path.relpath(tj, ROOT).replace(".json", ".md") if traffic_db else
                                                ("the tracked profile was taken on other kernel sources than the loaded library: stale, not reported" if traffic_stale else "no tracked profile for this workload")) + ")",
                               "flop_per_launch": round(gemm_flop / gemm_n),
                               "kernel": f"gemm_pp_kernel (persistent MFMA GEMM: the {round(gemm_n * stride / args.steps)} big vision-tower GEMM launches per step; "
                                         f"achieved = executed 2MNK / HIP-event time of the bracketed launches: every {stride}-th launch, counted across "
                                         "steps, so each launch site is sampled equally often)",
                               "executed_gemm_tflop_per_step": round(gemm_flop * stride / args.steps / 1e12, 3),
                               "launches_per_step": round(gemm_n * stride / args.steps), "sampled_launches": gemm_n, "sample_stride": stride,
                               "avg_launch_us": round(gemm_ms * 1e3 / gemm_n, 2),
                               "gemm_share_of_step": round(gemm_ms * stride / (elapsed * 1e3), 4),
                               # whole step.  step_* use the reference's ALGORITHMIC FLOPs (73.5 GFLOP per image): the library skips
                               # rows nothing uses (the last block's tail, block 0's backward, text positions behind the last EOT), so
                               # that figure credits eliminated work and is NOT a utilisation.  executed_* counts what ran on the matrix cores
                               # (every GEMM and attention launch of both towers): executed_frac is the step's MFMA utilisation against the 2.5 PF peak.
                               "step_achieved": round(step_flop / (ms * 1e-3) / 1e12, 1), "step_frac": round(step_flop / (ms * 1e-3) / 1e12 / PEAK_MFMA_TFLOPS, 4),
                               "executed_tflop_per_step": round(exec_flop / args.steps / 1e12, 3),
                               "executed_frac": round(exec_flop / args.steps / (ms * 1e-3) / 1e12 / PEAK_MFMA_TFLOPS, 4),
                               # the HBM-bound kernels of the step (LayerNorm with the fused residual add / splice; attention): algorithmic bytes /
                               # HIP-event time of the vision tower's launches, against the 8 TB/s spec; measured in hbm_kernels_steps extra
                               # steps right after the timed region (event pairs on every launch would slow the timed steps by 3 %)
                               "hbm_kernels": hbm, "hbm_kernels_steps": hbm_steps}
        if parity_ms:
            out["parity_mode_ms_per_step"] = round(parity_ms["fp32"], 3)
            out["parity_mode"] = ("dtype fp32 (parity mode): split forward GEMM operands -- text tower (hi, lo) fp16 pairs + fp32 attention forward; vision tower "
                                  "hi fp16 + e4m3 remainders contracted against e4m3 weights on v_mfma_scale_f32_16x16x128_f8f6f4, pixels included, fp16 attention -- "
                                  "fp32 residual / update streams; logits within 1e-3 of the reference at logit scale 100 (measured max 3.5e-4 on the reference "
                                  "fixtures: tests/test_exact_gpu.py; knobs vis_lo = 1 + vis_exact_attn = 1 give round 3's exact mode, 2.5e-5)")
            out["fast_parity_mode_ms_per_step"] = round(parity_ms["fp16"], 3)
            out["fast_parity_mode"] = "dtype fp16: fp16 operands, fp32 streams, split text-tower operands; logits within 1e-3 at the init logit scale 14.29 only (4e-3 at 100)"
            if "fp32x" in parity_ms:
                out["exact_mode_ms_per_step"] = round(parity_ms["fp32x"], 3)
                out["exact_mode"] = "dtype fp32 + knobs vis_lo = 1, vis_exact_attn = 1 (round 3's exact mode: fp16 pairs + fp32 attention in both towers; 2.5e-5 at logit scale 100)"
        if collective is not None:
            out["collective"] = collective
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(11, 12)
            out["cpu_baseline_c50"] = cpu_baseline(50, 6)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
