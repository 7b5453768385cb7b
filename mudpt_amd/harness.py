"""Dassl-free launcher for the MuDPT plugin on synthetic data (no datasets / checkpoints / network on the box).

    python -m mudpt_amd.harness --epochs 2 --batch 4 --n-ctx 4 --depth 12 [--prec fp16|amp] [--eval-only --model-dir D]
    python -m mudpt_amd.harness --trainer CoOp --epochs 2 [--csc] [--class-token-position end|middle|front]
    python -m mudpt_amd.harness --trainer VPT|MPT --epochs 2 [--deep-text-n-ctx N --text-prompt-depth D --deep-visual-n-ctx N --visual-prompt-depth D]
    python -m mudpt_amd.harness --trainer UMuDPT|UUMuDPT --epochs 2 [--n-ctx N --depth D]
    [MUDPT_FUSED_OPTIM=1] python -m mudpt_amd.harness --optim adam|amsgrad|adamw|rmsprop|sgd [--lr 0.0025]

Mirrors what ``train.py`` (reference :153-173) does after config assembly: build_trainer(cfg) -> train() / test()."""
from __future__ import annotations

import argparse

import torch

from . import cocoop, coop, dassl_lite, parallel, trainer, umudpt, uumudpt, vpt, zsclip  # noqa: F401  (importing the plugin modules registers MuDPT / CoCoOp / CoOp / VPT, MPT / UMuDPT / UUMuDPT / ZeroshotCLIP, ZeroshotCLIP2)


def run(argv=None):
    """Build the trainer the arguments name, then train (or, with --eval-only, load and test); returns the trainer, its outcome in ``.result``."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainer", default="MuDPT", choices=["MuDPT", "CoCoOp", "CoOp", "VPT", "MPT", "UMuDPT", "UUMuDPT"])
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--classes", type=int, default=11)
    ap.add_argument("--train-images", type=int, default=32)
    ap.add_argument("--n-ctx", type=int, default=4)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--prec", default="fp16", choices=["fp16", "fp32", "amp"])
    ap.add_argument("--csc", action="store_true", help="CoOp: class-specific contexts (TRAINER.COOP.CSC)")
    ap.add_argument("--class-token-position", default="end", choices=["end", "middle", "front"], help="CoOp: TRAINER.COOP.CLASS_TOKEN_POSITION")
    # VPT / MPT: TRAINER.<NAME>.DEEP_TEXT_N_CTX / TEXT_PROMPT_DEPTH / DEEP_VISUAL_N_CTX / VISUAL_PROMPT_DEPTH; default: the shipped yaml's
    for flag in ("--deep-text-n-ctx", "--text-prompt-depth", "--deep-visual-n-ctx", "--visual-prompt-depth"):
        ap.add_argument(flag, type=int, default=None, help="VPT / MPT prompt shape (default: configs/trainers/<NAME>/vit_b16_c2_ep5_batch4.yaml)")
    ap.add_argument("--optim", default="sgd", choices=list(dassl_lite.AVAI_OPTIMS), help="OPTIM.NAME (MUDPT_FUSED_OPTIM=1: its step as one HIP launch)")
    ap.add_argument("--lr", type=float, default=None, help="OPTIM.LR (default: the shipped MuDPT yaml's 0.0025)")
    ap.add_argument("--output-dir", default="output/mudpt_amd")
    ap.add_argument("--backbone-path", default="")
    ap.add_argument("--eval-only", action="store_true")
    ap.add_argument("--model-dir", default="")
    ap.add_argument("--load-epoch", type=int, default=None)
    a = ap.parse_args(argv)

    parallel.init()
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = a.output_dir
    cfg.OPTIM.MAX_EPOCH = a.epochs
    cfg.OPTIM.NAME = a.optim
    if a.lr is not None:
        cfg.OPTIM.LR = a.lr
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = a.batch
    cfg.DATALOADER.TEST.BATCH_SIZE = max(a.batch, 8)
    cfg.DATASET.NUM_CLASSES, cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = a.classes, a.train_images, 16
    cfg.MODEL.BACKBONE.PATH = a.backbone_path
    cfg.TRAINER.NAME = a.trainer
    cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH, cfg.TRAINER.MUDPT.PREC = a.n_ctx, a.depth, a.prec
    cfg.TRAINER.UMUDPT.N_CTX, cfg.TRAINER.UMUDPT.DEEP_PROMPT_DEPTH, cfg.TRAINER.UMUDPT.PREC = a.n_ctx, a.depth, a.prec
    cfg.TRAINER.UUMUDPT.N_CTX, cfg.TRAINER.UUMUDPT.DEEP_PROMPT_DEPTH, cfg.TRAINER.UUMUDPT.PREC = a.n_ctx, a.depth, a.prec
    cfg.TRAINER.COCOOP.PREC = a.prec
    cfg.TRAINER.COOP.N_CTX, cfg.TRAINER.COOP.PREC, cfg.TRAINER.COOP.CSC = a.n_ctx, a.prec, a.csc
    cfg.TRAINER.COOP.CLASS_TOKEN_POSITION = a.class_token_position
    for name in ("VPT", "MPT"):
        node = getattr(cfg.TRAINER, name)
        node.PREC = a.prec
        given = (a.deep_text_n_ctx, a.text_prompt_depth, a.deep_visual_n_ctx, a.visual_prompt_depth)
        shape = [g if g is not None else y for g, y in zip(given, vpt.YAML_PROMPTS[name])]
        node.DEEP_TEXT_N_CTX, node.TEXT_PROMPT_DEPTH, node.DEEP_VISUAL_N_CTX, node.VISUAL_PROMPT_DEPTH = shape
    torch.manual_seed(cfg.SEED)
    t = trainer.TRAINER_REGISTRY.get(a.trainer)(cfg) if not trainer.HAVE_DASSL else None
    if t is None:
        raise SystemExit("Dassl is installed: use the reference's train.py --trainer MuDPT / CoCoOp / CoOp / VPT / MPT / UMuDPT / UUMuDPT (see INTEGRATION.md)")
    if a.eval_only:
        t.load_model(a.model_dir, epoch=a.load_epoch)
        t.result = t.test()
    else:
        t.result = t.train()
    return t


def main(argv=None):
    return run(argv).result


if __name__ == "__main__":
    main()
