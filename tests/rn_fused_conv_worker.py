"""Child process of tests/test_resnet_conv_gpu.py: the CoOp plugin on RN50 (synthetic weights, B 2) as the environment configures it; saves the
logits of one inference forward and the paths the handle was switched to while it was built.  ``trainer_cfg`` is the configuration both sides use."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trainer_cfg(out_dir):
    from mudpt_amd import dassl_lite
    cfg = dassl_lite.default_cfg()
    cfg.TRAINER.NAME = "CoOp"
    cfg.MODEL.BACKBONE.NAME, cfg.MODEL.BACKBONE.SYNTHETIC_SEED = "RN50", 3
    cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 4, 4
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 2, 2
    cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.LR = 1, 0, 0.02
    cfg.OUTPUT_DIR = str(out_dir)
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    return cfg


def recorded_paths():
    """Wrap LibraryModel.set_resnet_conv_path so that every call is listed; returns the list."""
    from mudpt_amd.model import LibraryModel
    calls, inner = [], LibraryModel.set_resnet_conv_path

    def record(self, path):
        calls.append(int(path))
        return inner(self, path)
    LibraryModel.set_resnet_conv_path = record
    return calls


def plugin_logits(out_dir):
    from mudpt_amd import coop, dassl_lite  # noqa: F401 -- the plugin registers itself
    t = dassl_lite.build_trainer(trainer_cfg(out_dir))
    batch = t.train_loader_x[0]
    return t, batch["img"]


if __name__ == "__main__":
    paths = recorded_paths()
    t, img = plugin_logits(sys.argv[1])
    logits = t.model_inference(img.cuda()).cpu()
    t.model.close()
    torch.save({"logits": logits, "paths": paths}, sys.argv[2])
