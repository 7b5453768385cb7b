"""Generate the UUMuDPT golden vectors (tests/golden/uumudpt_*.npz) by running the REFERENCE's own ``trainers.uumudpt.CustomCLIP``.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/gen_golden_uumudpt.py

What runs: ``trainers.uumudpt.CustomCLIP`` over ``clip.model.CLIP(..., cfg)`` with ``TRAINER.NAME = "UUMuDPT"`` (the blocks of
``ResidualAttentionBlock_UUMuDPT`` and the vision tower of clip/model.py:600-664), imported with the placeholders of gen_golden.py, on torch
CPU fp32.  The frozen weights follow ``oracle.mudpt_oracle.make_frozen_state``; ``CLIP.load_state_dict`` must report exactly the 20
``visual.visual_ctx*`` keys as missing (stored) and nothing unexpected.  All 40 trainables are overwritten from the seeded draw of
``tests/uumudpt_reference.seeded_params`` (the fixture stores the seed, not the values), ctx keeping the reference's own CTX_INIT rows.
Stored per fixture: what gen_golden_umudpt.py stores -- config, class names, tokenized prompts, init tokens, seeds, labels, the images'
checksum, eval logits, training loss, logit_scale, every trainable's gradient (a tensor above 65 536 elements as 16 seeded rows plus its rms;
the tiny fixtures already above 32 768, or Gen2's 0.45 M gradient elements at width 192 alone would make each file 2.6 MB), sampled rows of
the tapped block inputs -- and two checksums (sum, abs-sum) per tensor of the reference's own FRESHLY CONSTRUCTED modules.  Those are drawn at two points, each right behind its own ``torch.manual_seed(seeds[1])``: the vision tower's 20 when ``CLIP(...)`` is
constructed, the prompt learner's 20 when ``CustomCLIP(...)`` is; they pin ``mudpt_amd.model.uumudpt_init_tensors``.
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
from tests import uumudpt_reference as R  # noqa: E402

TINY_NAMES = ["face", "water lily", "hawksbill turtle", "leopard", "stop sign"]
CTX_INIT = "a photo of a"


def run_uumudpt(base: O.Config, name: str, n_ctx: int, depth: int, batch: int, frozen_seed: int, train_seed: int, image_seed: int,
                classnames=None, logit_scale=None, taps=(), sample_above=R.SAMPLE_ABOVE):
    cfg = dataclasses.replace(base, n_ctx=n_ctx, depth=depth)
    names = list(classnames or CLASSNAMES)
    _clip, cm, _mudpt, CN = import_reference()
    from trainers import uumudpt
    ycfg = CN(TRAINER=CN(NAME="UUMuDPT", UUMUDPT=CN(N_CTX=n_ctx, CTX_INIT=CTX_INIT, DEEP_PROMPT_DEPTH=depth, PREC="fp32")),
              INPUT=CN(SIZE=(cfg.image_size, cfg.image_size)))
    torch.manual_seed(train_seed)  # seed point 1: the vision tower's 20 are drawn while CLIP is constructed
    ref_clip = cm.CLIP(cfg.embed_dim, cfg.image_size, cfg.v_layers, cfg.v_width, cfg.patch, cfg.ctx_len,
                       cfg.vocab, cfg.t_width, cfg.t_heads, cfg.t_layers, ycfg).float()
    frozen = with_logit_scale(O.make_frozen_state(cfg, frozen_seed), logit_scale)
    missing, unexpected = ref_clip.load_state_dict(frozen, strict=False)
    vis_keys = [k for k, _ in R.trainable_keys(cfg) if k.startswith(R.V)]
    assert not unexpected and sorted(missing) == sorted("visual." + k[len("image_encoder."):] for k in vis_keys), (missing, unexpected)
    torch.manual_seed(train_seed)  # seed point 2: the prompt learner's 20 are drawn while CustomCLIP is constructed
    model = uumudpt.CustomCLIP(ycfg, names, ref_clip)
    for k, p in model.named_parameters():  # freeze rule, trainers/uumudpt.py:255-261
        p.requires_grad_("prompt_learner" in k or "visual_ctx" in k)
    trainable = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    assert [(k, tuple(p.shape)) for k, p in trainable] == R.trainable_keys(cfg), [k for k, _ in trainable]
    init_checksums = {k: [p.detach().double().sum().item(), p.detach().double().abs().sum().item()] for k, p in trainable}
    tok = model.tokenized_prompts
    ctx_ids = _clip.tokenize(CTX_INIT)[0, 1:1 + n_ctx].tolist()
    values = R.seeded_params(cfg, train_seed, frozen["token_embedding.weight"][ctx_ids])
    with torch.no_grad():
        for k, p in trainable:
            if k == R.CTX:
                assert torch.equal(p, values[k])  # the reference's own init (uumudpt.py:97-104) is what the restatement rebuilds
            p.copy_(values[k])
    images = seeded_images(cfg, batch, image_seed)
    labels = (torch.arange(batch) * 3 + 1) % len(names)
    got = {}
    hooks = []
    for tower, i in taps:  # the input of ln_1 = the block input after its splice, LND
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
        "config": np.array(repr(cfg.asdict())), "trainer": np.array("UUMuDPT"),
        "classnames": np.array(names), "tokenized_prompts": tok.numpy().astype(np.int32),
        "ctx_token_ids": np.array(ctx_ids, dtype=np.int64),
        "seeds": np.array([frozen_seed, train_seed, image_seed], dtype=np.int64), "labels": labels.numpy().astype(np.int64),
        "images_checksum": np.array([images.double().sum().item(), images.double().abs().sum().item()]),
        "logits": logits.numpy(), "loss": np.array(loss.item(), dtype=np.float64),
        "logit_scale": np.array(frozen["logit_scale"].item(), dtype=np.float32),
        "clip_missing_keys": np.array(list(missing)), "sample_above": np.array(sample_above, dtype=np.int64),
    }
    for k, p in trainable:
        g = p.grad.detach() if p.grad is not None else torch.zeros_like(p)
        out["init_checksum." + k] = np.array(init_checksums[k])
        if g.numel() > sample_above:
            rows = R.sample_rows(k, g.shape[0], train_seed)
            out["grad_rows." + k] = g[rows].numpy()
            out["grad_rows." + k + ".idx"] = np.array(rows, dtype=np.int32)
            out["grad_rms." + k] = np.array(g.double().pow(2).mean().sqrt().item())
        else:
            out["grad." + k] = g.numpy()
    for key, x in got.items():
        L = x.shape[1]
        rows = sorted(set([0, 1, L // 2] + list(range(L - n_ctx, L)))) if key.startswith("vis") else list(range(0, n_ctx + 2))
        out["tap." + key] = x[:, rows].numpy().astype(np.float32)
        out["tap." + key + ".rows"] = np.array(rows, dtype=np.int32)
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss {loss.item():.6f}, {len(trainable)} trainables, {os.path.getsize(path) / 1e6:.3f} MB")


if __name__ == "__main__":
    tiny, b16 = O.TINY, O.VIT_B16
    small = R.TINY_SAMPLE_ABOVE
    run_uumudpt(tiny, "uumudpt_tiny", 2, 3, 3, 21, 42, 23, TINY_NAMES, sample_above=small)       # a splice in every block
    run_uumudpt(tiny, "uumudpt_tiny_d1", 3, 1, 3, 21, 43, 23, TINY_NAMES, sample_above=small)    # empty tensors, Gen2 idle, odd L
    run_uumudpt(tiny, "uumudpt_tiny_d5", 2, 5, 3, 21, 44, 23, TINY_NAMES, sample_above=small)    # deeper than the 3-layer towers: unconsumed rows in both directions
    vit_taps = (("vis", 1), ("vis", 7), ("txt", 1))
    run_uumudpt(b16, "uumudpt_vitb16_b2", 2, 8, 2, 0, 6, 4321, taps=vit_taps)  # train.py:129-133 defaults
    run_uumudpt(b16, "uumudpt_vitb16_b2_s100", 2, 8, 2, 0, 6, 4321, logit_scale=100.0)
