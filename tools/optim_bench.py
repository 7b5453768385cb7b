"""The optimizer step on one MI355X: torch.optim (its default path on the device: foreach) against the fused step (mudpt_amd/optim.py,
BucketOptimizer(backend="hip"): one mudpt_optim_step launch), and its share of the plugin's training step.

    python tools/optim_bench.py [--steps 50] [--rounds 5] [--skip-plugin]
One process; the two sides of every comparison are timed alternately, round by round, after a warm-up, and the MEDIAN (min - max) over the
rounds is reported.
  1. The step alone, for sgd / adam / amsgrad / adamw / rmsprop (Dassl's names and defaults, dassl_lite.build_optimizer), over the trainables
     of a MuDPT model (n_ctx 4, depth 12: 10 tensors, 1 243 136 elements) and of a UUMuDPT model (n_ctx 2, depth 8: 40 tensors), gradients
     fixed.  "host": wall time the host spends issuing one step (the loop is not synchronised inside); "device": HIP events around the same
     loop, per step -- on a step that is bound by launches the two are the same number.
  2. The plugin's step (dassl_lite harness, MuDPT, ViT-B/16, B 4, PREC fp16, a resident device batch, loss.item() every step) under
     OPTIM.NAME sgd and adam, without and with MUDPT_FUSED_OPTIM=1.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import dassl_lite, synth, trainer  # noqa: F401
from mudpt_amd.model import CustomCLIP, ModelShape
from mudpt_amd.optim import BucketOptimizer

NAMES = ("sgd", "adam", "amsgrad", "adamw", "rmsprop")


def spread(xs, unit=1e3, fmt="{:.1f}"):
    return f"{fmt.format(statistics.median(xs) * unit)} ({fmt.format(min(xs) * unit)} - {fmt.format(max(xs) * unit)})"


def time_steps(opt, steps):
    """(host seconds, device seconds) per step of `steps` consecutive opt.step() calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    host = time.perf_counter() - t0
    stop.record()
    torch.cuda.synchronize()
    return host / steps, start.elapsed_time(stop) * 1e-3 / steps


def step_alone(variant, n_ctx, depth, steps, rounds):
    shape = ModelShape(n_ctx=n_ctx, depth=depth)
    m = CustomCLIP(shape, synth.random_clip_state(shape, 0), synth.synthetic_tokenized_prompts(11, n_ctx), max_batch=4, dtype="fp16", seed=1, variant=variant)
    params = list(m.parameters())
    g = torch.Generator().manual_seed(0)
    m.flat_grads.copy_(1e-3 * torch.randn(m.flat_grads.numel(), generator=g))
    start = m.flat_params.clone()
    cfg = dassl_lite.default_cfg().OPTIM
    print(f"\n{variant}: {len(params)} tensors, {m.flat_params.numel()} elements; microseconds per step, median (min - max) of {rounds} rounds of {steps} steps")
    print("| OPTIM.NAME | torch.optim host | torch.optim device | fused host | fused device | device ratio |")
    print("|---|---|---|---|---|---|")
    for name in NAMES:
        cfg.NAME = name
        theirs = dassl_lite.build_optimizer(m, cfg)
        mine = BucketOptimizer.from_torch(theirs, model=m, backend="hip")
        res = {"torch": ([], []), "fused": ([], [])}
        for opt in (theirs, mine):
            time_steps(opt, 10)
        for _ in range(rounds):
            for key, opt in (("torch", theirs), ("fused", mine)):
                h, d = time_steps(opt, steps)
                res[key][0].append(h)
                res[key][1].append(d)
        ratio = statistics.median(res["torch"][1]) / statistics.median(res["fused"][1])
        print(f"| {name} | {spread(res['torch'][0], 1e6)} | {spread(res['torch'][1], 1e6)} | {spread(res['fused'][0], 1e6)} | {spread(res['fused'][1], 1e6)} | {ratio:.1f}x |", flush=True)
        with torch.no_grad():
            m.flat_params.copy_(start)
    m.close()


def plugin_step(steps, rounds):
    def make(name, fused):
        if fused:
            os.environ["MUDPT_FUSED_OPTIM"] = "1"
        else:
            os.environ.pop("MUDPT_FUSED_OPTIM", None)
        cfg = dassl_lite.default_cfg()
        cfg.OUTPUT_DIR = "/tmp/mudpt_optim_bench"
        cfg.OPTIM.NAME, cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH = name, 1, 0
        cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 8, 4
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 4, 4
        cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH, cfg.TRAINER.MUDPT.PREC = 4, 12, "fp16"
        t = dassl_lite.build_trainer(cfg)
        t.set_model_mode("train")
        t.batch_idx, t.num_batches = 0, 10 ** 9
        assert isinstance(t.optim, BucketOptimizer) == fused
        return t

    def timed(t, batch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            t.forward_backward(batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    print(f"\nplugin step, MuDPT ViT-B/16 B 4 fp16, resident batch; milliseconds per step, median (min - max) of {rounds} rounds of {steps} steps")
    print("| OPTIM.NAME | torch.optim | MUDPT_FUSED_OPTIM=1 | difference |")
    print("|---|---|---|---|")
    for name in ("sgd", "adam"):
        pair = {"torch": make(name, False), "fused": make(name, True)}
        batch = next(iter(pair["torch"].train_loader_x))
        ms = {k: [] for k in pair}
        for t in pair.values():
            timed(t, batch)
        for _ in range(rounds):
            for k, t in pair.items():
                ms[k].append(timed(t, batch))
        diff = (statistics.median(ms["torch"]) - statistics.median(ms["fused"])) * 1e3
        print(f"| {name} | {spread(ms['torch'], 1e3, '{:.3f}')} | {spread(ms['fused'], 1e3, '{:.3f}')} | {diff:+.3f} ms |", flush=True)
        for t in pair.values():
            t.model.close()
    os.environ.pop("MUDPT_FUSED_OPTIM", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-plugin", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs an MI355X: a timing without the GPU says nothing")
    step_alone("mudpt", 4, 12, a.steps, a.rounds)
    step_alone("uumudpt", 2, 8, a.steps, a.rounds)
    if not a.skip_plugin:
        plugin_step(a.steps, a.rounds)


if __name__ == "__main__":
    main()
