"""Generate the VPT / MPT golden vectors (tests/golden/vpt_*.npz, mpt_*.npz) by running the REFERENCE's own ``trainers.vpt.CustomCLIP`` /
``trainers.mpt.CustomCLIP``.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/gen_golden_vpt.py          # every vpt_*.npz and mpt_*.npz

What runs: ``trainers.vpt.CustomCLIP`` / ``trainers.mpt.CustomCLIP`` over ``clip.model.CLIP(..., cfg)`` with ``TRAINER.NAME = "VPT" / "MPT"``
(the prompted blocks of clip/model.py:202-251,443-496), imported with the placeholders of gen_golden.py, on torch CPU fp32.  One patch: VPT's
``TextPromptLearner.forward`` returns ``self.prompts.cuda()`` (trainers/vpt.py:69); for this CPU run it returns ``self.prompts`` (the identity
on the values).  The frozen weights follow ``oracle.mudpt_oracle.make_frozen_state``; every per-layer prompt is overwritten from the seeded
draw of ``tests/vpt_reference.seeded_prompts`` (the fixture stores the seed, not the values); MPT's text ctx keeps the reference's own
TEXT_CTX_INIT init.  Stored per fixture: config, trainer, the four prompt counts, class names, tokenized prompts, the init tokens, seeds,
labels, the images' checksum, eval logits, training loss, every trainable's gradient, logit_scale and, for the ViT-B fixtures, sampled rows
of the vision block inputs 1 and 11 (after the splice) and, MPT, of text block 1.
"""
from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import CLASSNAMES, ROOT, O, import_reference, seeded_images, with_logit_scale  # noqa: E402

sys.path.insert(0, ROOT)
from tests import vpt_reference as R  # noqa: E402

TINY_NAMES = ["face", "water lily", "hawksbill turtle", "leopard", "stop sign"]
CTX_INIT = "a photo of a"


def run_vpt(cfg: O.Config, name: str, trainer: str, shape, batch: int, frozen_seed: int, train_seed: int, image_seed: int,
            classnames=None, logit_scale=None, taps=()):
    names = list(classnames or CLASSNAMES)
    t_n, t_depth, v_n, v_depth = shape
    _clip, cm, _mudpt, CN = import_reference()
    from trainers import mpt, vpt
    mod = vpt if trainer == "VPT" else mpt
    if trainer == "VPT":
        vpt.TextPromptLearner.forward = lambda self: self.prompts  # trainers/vpt.py:69 calls .cuda(): the identity on this CPU run
    node = CN(DEEP_TEXT_N_CTX=t_n, DEEP_VISUAL_N_CTX=v_n, TEXT_PROMPT_DEPTH=t_depth, VISUAL_PROMPT_DEPTH=v_depth, TEXT_CTX_INIT=CTX_INIT, PREC="fp32")
    ycfg = CN(TRAINER=CN(NAME=trainer, **{trainer: node}), INPUT=CN(SIZE=(cfg.image_size, cfg.image_size)))
    ref_clip = cm.CLIP(cfg.embed_dim, cfg.image_size, cfg.v_layers, cfg.v_width, cfg.patch, cfg.ctx_len,
                       cfg.vocab, cfg.t_width, cfg.t_heads, cfg.t_layers, ycfg).float()
    frozen = with_logit_scale(O.make_frozen_state(cfg, frozen_seed), logit_scale)
    missing, unexpected = ref_clip.load_state_dict(frozen, strict=False)
    assert not unexpected and all(k.endswith("visual_ctx") for k in missing), (missing, unexpected)
    model = mod.CustomCLIP(ycfg, names, ref_clip)
    for k, p in model.named_parameters():  # freeze rules, trainers/vpt.py:141-146 and mpt.py:195-202
        p.requires_grad_("visual_ctx" in k or (trainer == "MPT" and "ctx" in k))
    trainable = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    assert [(k, tuple(p.shape)) for k, p in trainable] == R.trainable_keys(cfg, trainer, shape), [k for k, _ in trainable]
    tok = model.tokenized_prompts
    ctx_ids = _clip.tokenize(CTX_INIT)[0, 1:1 + t_n].tolist() if trainer == "MPT" else []
    text_ctx = frozen["token_embedding.weight"][ctx_ids] if trainer == "MPT" else None
    values = R.seeded_prompts(cfg, trainer, shape, train_seed, text_ctx)
    with torch.no_grad():
        for k, p in trainable:
            if k == R.TEXT_CTX:
                assert torch.equal(p, values[k])  # the reference's own init (mpt.py:55-62) is what the restatement rebuilds
            p.copy_(values[k])
    images = seeded_images(cfg, batch, image_seed)
    labels = (torch.arange(batch) * 3 + 1) % len(names)
    got = {}
    hooks = []
    for tower, i in taps:  # the input of ln_1 = the block input after its splice (clip/model.py:240-250), LND
        blocks = model.image_encoder.transformer.resblocks if tower == "vis" else model.text_encoder.transformer.resblocks
        hooks.append(blocks[i].ln_1.register_forward_pre_hook(lambda _m, a, key=f"{tower}.{i}": got.__setitem__(key, a[0].detach().permute(1, 0, 2))))
    model.eval()
    with torch.no_grad():
        logits = model(images)
    for h in hooks:
        h.remove()
    model.train()
    loss = torch.nn.functional.cross_entropy(model(images), labels)
    loss.backward()
    out = {
        "config": np.array(repr(cfg.asdict())), "trainer": np.array(trainer), "prompt_shape": np.array(shape, dtype=np.int32),
        "classnames": np.array(names), "tokenized_prompts": tok.numpy().astype(np.int32),
        "ctx_token_ids": np.array(ctx_ids, dtype=np.int64),
        "seeds": np.array([frozen_seed, train_seed, image_seed], dtype=np.int64), "labels": labels.numpy().astype(np.int64),
        "images_checksum": np.array([images.double().sum().item(), images.double().abs().sum().item()]),
        "logits": logits.numpy(), "loss": np.array(loss.item(), dtype=np.float64),
        "logit_scale": np.array(frozen["logit_scale"].item(), dtype=np.float32),
    }
    for k, p in trainable:
        out["grad." + k] = p.grad.detach().numpy()
    for key, x in got.items():
        L = x.shape[1]
        if key.startswith("vis"):
            rows = sorted(set([0, 1, L // 2] + list(range(L - v_n, L))))
        else:
            rows = list(range(0, t_n + 2))
        out["tap." + key] = x[:, rows].numpy().astype(np.float32)
        out["tap." + key + ".rows"] = np.array(rows, dtype=np.int32)
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss {loss.item():.6f}, {len(trainable)} trainables, {os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    tiny = O.TINY
    b16 = O.VIT_B16
    run_vpt(tiny, "vpt_tiny", "VPT", (0, 0, 4, 3), 3, 21, 22, 23, TINY_NAMES)                  # splice in every block
    run_vpt(tiny, "vpt_tiny_shallow", "VPT", (0, 0, 4, 1), 3, 21, 24, 23, TINY_NAMES)          # input prompt only
    run_vpt(tiny, "mpt_tiny", "MPT", (2, 3, 3, 2), 3, 21, 25, 23, TINY_NAMES)                  # unequal counts and depths
    run_vpt(tiny, "mpt_tiny_textonly", "MPT", (2, 3, 3, 0), 3, 21, 26, 23, TINY_NAMES)         # vanilla vision tower
    run_vpt(b16, "vpt_vitb16_b2", "VPT", (0, 0, 8, 12), 2, 0, 2, 4321, taps=(("vis", 1), ("vis", 11)))  # configs/trainers/VPT yaml
    run_vpt(b16, "mpt_vitb16_b2", "MPT", (2, 12, 2, 12), 2, 0, 3, 4321, taps=(("vis", 1), ("vis", 11), ("txt", 1)))  # configs/trainers/MPT yaml
    run_vpt(b16, "vpt_vitb16_b2_s100", "VPT", (0, 0, 8, 12), 2, 0, 2, 4321, logit_scale=100.0)
    run_vpt(b16, "mpt_vitb16_b2_s100", "MPT", (2, 12, 2, 12), 2, 0, 3, 4321, logit_scale=100.0)
