"""Images/s THROUGH THE PLUGIN (dassl_lite harness): host batches from the loader, parse_batch_train, forward_backward with the
torch optimizer step and loss.item() every step, as trainers/mudpt.py:235-261 -- with and without the DevicePrefetcher.

    python tools/plugin_bench.py [--batch 256] [--steps 12] [--device-data]

--device-data: the opt-in device-resident input path instead (mudpt_amd/augment.py, MUDPT_DEVICE_DATA=1 with the shipped transforms): batches cropped,
flipped and normalised by one HIP launch per step from a uint8 store in HBM, beside the same step on one resident batch (no input work at all).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import dassl_lite, trainer  # noqa: F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--device-data", action="store_true")
    a = ap.parse_args()
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = "/tmp/mudpt_plugin_bench"
    cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH = 1, 0
    cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = a.batch * a.steps, 8
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = a.batch, 8
    cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH, cfg.TRAINER.MUDPT.PREC = 4, 12, "amp"
    if a.device_data:
        os.environ["MUDPT_DEVICE_DATA"] = "1"
        cfg.INPUT.TRANSFORMS, cfg.INPUT.INTERPOLATION = ("random_resized_crop", "random_flip", "normalize"), "bicubic"
    t = dassl_lite.build_trainer(cfg)
    t.set_model_mode("train")
    t.num_batches = 10 ** 9
    if a.device_data:
        from mudpt_amd.augment import DeviceAugmentLoader
        assert isinstance(t.train_loader_x, DeviceAugmentLoader), "the device-resident path was refused"
        resident = next(iter(t.train_loader_x))
        loaders = (("device store (crop + flip + normalize: one HIP launch per step)", t.train_loader_x), ("resident (one device batch, reused)", [resident] * a.steps))
    else:
        loaders = (("prefetched (side-stream copy of the next batch)", t.train_loader_x), ("plain (.to(device) at the top of the step)", t.train_loader_x.loader))
    for name, loader in loaders:
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for t.batch_idx, batch in enumerate(loader):
                t.forward_backward(batch)
                n += a.batch
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print(f"{name}: {dt / a.steps * 1e3:.2f} ms/step, {n / dt:.0f} images/s", flush=True)


if __name__ == "__main__":
    main()
