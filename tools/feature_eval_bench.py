"""Timing of the test pass from cached image features (mudpt_amd/featcache.py) on one MI355X, beside the two passes over images.  One process,
warmed up; the three versions alternate round by round; median and spread of the rounds, wall clock with a device synchronisation at the end.

    python tools/feature_eval_bench.py [--images 2000] [--cocoop-images 200] [--batch 100] [--rounds 5] [--trainers ZeroshotCLIP,CoOp,CoCoOp]
For ZeroshotCLIP and CoOp at 1 000 classes and for CoCoOp at 100 (ViT-B/16, fp16, dassl_lite plugins, test() as users call it):
      host      the host loader (fp32 images, one host-to-device copy per batch)
      device    the DeviceEvalLoader (resize, center crop and normalize in one HIP launch per batch from a uint8 store in HBM)
      features  a FeatureStore of the device loader's images (trainer.test_features): model.forward_features per batch, no vision tower
The feature pass and the device pass see the same images and must give the same accuracy; that is asserted.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

CLASSES = {"ZeroshotCLIP": 1000, "ZeroshotCLIP2": 1000, "CoOp": 1000, "CoCoOp": 100}


def bench_trainer(name, images, a):
    from mudpt_amd import cocoop, coop, dassl_lite, synth, trainer, zsclip  # noqa: F401 -- the plugins register themselves
    from mudpt_amd.augment import DeviceEvalLoader
    from mudpt_amd.featcache import FeatureStore
    classes = CLASSES[name]
    if classes > len(synth.BENCH_CLASSNAMES):  # "class<i>" names need CLIP's merge table; without one, synthetic token ids of the same shapes
        trainer.tokenize_prompts = zsclip.tokenize_prompts = lambda prompts, ctx_len=77, near=None: synth.synthetic_tokenized_prompts(len(prompts), n_ctx=4, ctx_len=ctx_len)
        coop.name_lengths = lambda names, near=None: (synth.synthetic_tokenized_prompts(len(names), n_ctx=4).long().argmax(-1) - 2 - 4).tolist()  # as tools/coop_bench.py
    cfg = dassl_lite.default_cfg()
    cfg.TRAINER.NAME = name
    cfg.OUTPUT_DIR = "/tmp/mudpt_feature_eval_bench"
    cfg.DATASET.NAME = "Caltech101"  # ZeroshotCLIP's template is keyed by it
    cfg.DATASET.NUM_CLASSES, cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = classes, 4, images
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 4, a.batch
    cfg.TRAINER.COOP.N_CTX = 4
    cfg.INPUT.TRANSFORMS, cfg.INPUT.INTERPOLATION = ("random_resized_crop", "random_flip", "normalize"), "bicubic"
    with contextlib.redirect_stdout(io.StringIO()):
        t = dassl_lite.build_trainer(cfg)
    host = t.test_loader
    store = t.dm.uint8_test_store("cuda:0")
    device = DeviceEvalLoader(store, a.batch, cfg.INPUT.SIZE[0])
    assert len(host) == len(device) == images // a.batch, (len(host), len(device))
    feats = []
    with torch.no_grad():
        for batch in device:  # what a first pass under MUDPT_TEST_FEATURES collects
            t.model(batch["img"])
            feats.append(t.model.image_features())
    features = FeatureStore(torch.cat(feats), store.labels, name="<bench>")

    def run(loader, cached):
        t.test_loader = loader
        t.test_features = features if cached else None
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = t.test()
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert ("Cached test features: " in out.getvalue()) == cached and "refused" not in out.getvalue(), out.getvalue()
        return ms, acc
    versions = {"host": (host, False), "device": (device, False), "features": (device, True)}  # the feature pass checks its labels against the device loader's
    accs = {k: run(*v)[1] for k, v in versions.items()}  # warm-up
    assert accs["features"] == accs["device"], accs
    ms = {k: [] for k in versions}
    for _ in range(a.rounds):
        for k, v in versions.items():
            ms[k].append(run(*v)[0])
    t.model.close()
    return {"classes": classes, "images": images, "batch": a.batch, "batches": len(device), "accuracy": accs,
            **{k + "_ms": {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            "device_over_features": round(statistics.median(ms["device"]) / statistics.median(ms["features"]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--cocoop-images", type=int, default=200, help="CoCoOp runs images x classes text sequences: fewer images")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trainers", default="ZeroshotCLIP,CoOp,CoCoOp")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_eval_bench: no GPU: nothing is measured without one")
    result = {"tool": "feature_eval_bench", "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for name in a.trainers.split(","):
        result[name] = bench_trainer(name, a.cocoop_images if name == "CoCoOp" else a.images, a)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
