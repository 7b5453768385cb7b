"""Timing of the test pass's evaluator (mudpt_amd/evaluator.py over csrc/evaluate.hip) and of the device-resident test loader on one MI355X.
One process, warmed up; the versions of a measurement alternate round by round, median and spread of the rounds.

    python tools/eval_bench.py [--iters 200] [--rounds 7] [--images 2000] [--classes 1000] [--batch 100] [--skip-pass]
(a) mudpt_eval_accumulate at 100 x 1000, 256 x 1000 and 256 x 11 (device events around back-to-back launches), beside a device copy of the same
    logits and beside torch's argmax + == + sum on the device (three launches and no transfer: what a transfer-free loop in torch would cost);
(b) a full test pass of --images synthetic images through the dassl_lite MuDPT plugin (ViT-B/16, --classes classes, --batch images a batch, text
    features cached after the first batch), wall clock with a device synchronisation at the end:
      parent     the loop test() had before the evaluator: argmax, then int((pred == y).sum()) -- one device-to-host transfer per batch -- on the host loader
      evaluator  test() as it is now (DeviceClassification: one launch per batch, one transfer at the end) on the same host loader
      device     the same test() on the DeviceEvalLoader (MUDPT_DEVICE_TEST: resize, center crop and normalize in one HIP launch per batch from a
                 uint8 store in HBM; other images than the host loader's fp32 noise, the same number and size of batches)"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import capi


def fmt(v, unit):
    return f"{statistics.median(v):9.3f} {unit} (rounds {min(v):.3f} .. {max(v):.3f})"


def event_rounds(fns, iters, rounds):
    """fns: {name: callable}; they alternate round by round.  {name: [microseconds per call of each round]}, device events around back-to-back calls."""
    out = {k: [] for k in fns}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(rounds):
        for name, fn in fns.items():
            ev[0].record()
            for _ in range(iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]) / iters * 1e3)
    return out


def bench_accumulate(rows, n_cls, a):
    g = torch.Generator().manual_seed(rows + n_cls)
    z, y = torch.randn(rows, n_cls, generator=g).cuda(), torch.randint(0, n_cls, (rows,), generator=g).cuda()
    state = torch.zeros(capi.call("mudpt_eval_state_numel", n_cls=n_cls, with_cmat=0), dtype=torch.int32, device="cuda")
    dst, s = torch.empty_like(z), torch.cuda.current_stream().cuda_stream
    count = torch.zeros((), dtype=torch.int64, device="cuda")

    def torch_count():
        count.add_((z.argmax(dim=1) == y).sum())
    fns = {"accumulate": lambda: capi.call("mudpt_eval_accumulate", logits=z, ldz=n_cls, labels=y, rows=rows, n_cls=n_cls, state=state, with_cmat=0, stream=s),
           "copy": lambda: dst.copy_(z), "torch": torch_count}
    for fn in fns.values():
        for _ in range(10):
            fn()
    state.zero_()
    us = event_rounds(fns, a.iters, a.rounds)
    torch.cuda.synchronize()
    assert int(state[0]) == rows * a.iters * a.rounds and int(state[1]) * 1 == int((z.argmax(dim=1) == y).sum()) * a.iters * a.rounds
    tag = f"{rows} x {n_cls}"
    for name, label in (("accumulate", "mudpt_eval_accumulate"), ("copy", "device copy of the logits"), ("torch", "torch argmax + == + sum")):
        print(f"(a) [{tag:>10s}] {label:28s} {fmt(us[name], 'us')}", flush=True)
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = max(max(v) - min(v) for v in us.values())
    print(f"(a) [{tag:>10s}] accumulate / copy = {med['accumulate'] / med['copy']:.2f}, torch / accumulate = {med['torch'] / med['accumulate']:.2f}; "
          f"largest spread of the rounds {spread:.3f} us", flush=True)


@torch.no_grad()
def parent_test(t):
    """dassl_lite.TrainerX.test() as it was before the evaluator"""
    t.set_model_mode("eval")
    correct = total = 0
    for batch in t.test_loader:
        x, y = t.parse_batch_test(batch)
        pred = t.model_inference(x).argmax(dim=1)
        correct += int((pred == y).sum())
        total += int(y.numel())
    return 100.0 * correct / max(total, 1)


def bench_pass(a):
    import contextlib
    import io
    from mudpt_amd import dassl_lite, synth, trainer
    from mudpt_amd.augment import DeviceEvalLoader
    if a.classes > len(synth.BENCH_CLASSNAMES):  # "class<i>" names need CLIP's merge table; without one, synthetic token ids of the same shapes
        trainer.tokenize_prompts = lambda prompts, ctx_len=77, near=None: synth.synthetic_tokenized_prompts(len(prompts), n_ctx=4, ctx_len=ctx_len)
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = "/tmp/mudpt_eval_bench"
    cfg.DATASET.NUM_CLASSES, cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = a.classes, 4, a.images
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 4, a.batch
    cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH, cfg.TRAINER.MUDPT.PREC = 4, 12, "fp16"
    cfg.INPUT.TRANSFORMS, cfg.INPUT.INTERPOLATION = ("random_resized_crop", "random_flip", "normalize"), "bicubic"
    with contextlib.redirect_stdout(io.StringIO()):
        t = dassl_lite.build_trainer(cfg)
    host = t.test_loader
    store = t.dm.uint8_test_store("cuda:0")
    device = DeviceEvalLoader(store, a.batch, cfg.INPUT.SIZE[0])
    assert len(host) == len(device) == a.images // a.batch, (len(host), len(device))

    def run(fn, loader):
        t.test_loader = loader
        with contextlib.redirect_stdout(io.StringIO()):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, acc
    versions = {"parent": (lambda: parent_test(t), host), "evaluator": (t.test, host), "device": (t.test, device)}
    accs = {k: run(*v)[1] for k, v in versions.items()}  # warm-up; the two passes over the host loader see the same logits
    assert accs["parent"] == accs["evaluator"], accs
    ms = {k: [] for k in versions}
    for _ in range(a.rounds):
        for k, v in versions.items():
            ms[k].append(run(*v)[0])
    n = len(host)
    tag = f"{a.images} images, {a.classes} classes, B {a.batch}"
    labels = {"parent": "parent's loop, host loader", "evaluator": "evaluator, host loader", "device": "evaluator, DeviceEvalLoader"}
    for k in versions:
        print(f"(b) [{tag}] {labels[k]:30s} {fmt(ms[k], 'ms')} = {statistics.median(ms[k]) / n:7.3f} ms per batch", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"(b) [{tag}] parent - evaluator = {med['parent'] - med['evaluator']:.3f} ms, evaluator - device = {med['evaluator'] - med['device']:.3f} ms, "
          f"against a largest spread of the rounds of {spread:.3f} ms; store {store.nbytes / 2 ** 20:.0f} MiB of uint8", flush=True)
    t.model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--skip-pass", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU: nothing is measured without one")
    capi.load()
    for rows, n_cls in ((100, 1000), (256, 1000), (256, 11)):
        bench_accumulate(rows, n_cls, a)
    if not a.skip_pass:
        bench_pass(a)


if __name__ == "__main__":
    main()
