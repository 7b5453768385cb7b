"""Generate the ResNet zero-shot golden vectors (tests/golden/rn_*.npz) by running the REFERENCE's own ``ModifiedResNet`` inside its own
``trainers.zsclip.ZeroshotCLIP`` / ``ZeroshotCLIP2``.

Run in the build container only (needs the reference checkout, which never travels to the GPU box), on the CPU:

    python tests/golden/gen_golden_resnet.py

What runs: as tests/golden/gen_golden_zsclip.py -- the reference's ``build_model`` and ``model_inference`` on a bare trainer instance, torch CPU
fp32 -- with ``load_clip_to_cpu`` replaced by ``clip.model.CLIP(embed_dim, image_size, (l1, l2, l3, l4), width, 0, ...)``: the tuple selects
``ModifiedResNet`` (clip/model.py:686-694).  Its text side is loaded from ``oracle.mudpt_oracle.make_frozen_state``, its tower from
``tests.resnet_reference.make_rn_state``; the fixture stores the seeds (frozen, tower, images), not the weights.  Stored per fixture: config
(the text side; its ViT fields only seed the draws), rn_stages, rn_width, trainer, dataset, class names, templates, ``tokens`` int32
[T, C, 77], seeds, labels, the images' checksum, logits, the final ``text_features`` [C, e], the raw ``image_features`` [B, e]
(clip_model.visual(image)), logit_scale and ``emulated_rel`` [fp16, bf16]: the float64 restatement of tests/resnet_reference.py with rounding
to T at the library's five sites, against the reference's features (max over images of |F - ref| / |ref|) -- the error of the number formats
alone, which the GPU test's feature bound is three times -- and ``emulated_logit`` [fp16 max, rms, bf16 max, rms]: the logits of those
emulated features (against the reference's own text features) minus the reference's logits, i.e. what the formats alone cost at the logits;
tests/test_resnet_cpu.py holds it inside helpers.check_logits' bounds with a factor 2 to spare, so the GPU test's logit bound is one a correct
implementation can meet.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import CLASSNAMES, ROOT, O, import_reference, seeded_images, with_logit_scale  # noqa: E402
from gen_golden_zsclip import ZS_TINY_NAMES  # noqa: E402
from tests import resnet_reference as R  # noqa: E402


def run_rn(name: str, stages, width: int, image_size: int, embed_dim: int, text: dict, trainer: str, dataset: str, classnames, batch: int, frozen_seed: int,
           rn_seed: int, image_seed: int, logit_scale=None):
    names = list(classnames)
    # the ViT fields are no tower of this fixture: they only take part in make_frozen_state's draws (v_layers = the tower's blocks, so that
    # helpers.check_logits gives the real shape its real bound)
    cfg = O.Config(image_size=image_size, patch=32, v_width=64, v_layers=sum(stages), v_heads=1, embed_dim=embed_dim, n_ctx=0, depth=1, **text)
    clip, cm, _mudpt, CN = import_reference()
    from trainers import zsclip
    frozen = with_logit_scale(O.make_frozen_state(cfg, frozen_seed), logit_scale)
    rn = R.make_rn_state(R.RnShape(stages, width, image_size, embed_dim), rn_seed)
    state = {k: v for k, v in frozen.items() if not k.startswith("visual.")}
    state.update(rn)

    def load_clip_to_cpu(_cfg):
        model = cm.CLIP(embed_dim, image_size, tuple(stages), width, 0, cfg.ctx_len, cfg.vocab, cfg.t_width, cfg.t_heads, cfg.t_layers, None).float()
        assert type(model.visual).__name__ == "ModifiedResNet"
        missing, unexpected = model.load_state_dict(state, strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
        return model.eval()
    zsclip.load_clip_to_cpu = load_clip_to_cpu
    zsclip.ZeroshotCLIP2.templates = list(zsclip.ZeroshotCLIP2.templates[:7])
    cls = getattr(zsclip, trainer)
    t = cls.__new__(cls)
    t.cfg = CN(DATASET=CN(NAME=dataset), MODEL=CN(BACKBONE=CN(NAME="synthetic", PATH="")))
    t.dm = types.SimpleNamespace(dataset=types.SimpleNamespace(classnames=names))
    t.device = "cpu"
    with torch.no_grad():
        t.build_model()
        templates = list(t.templates) if trainer == "ZeroshotCLIP2" else [zsclip.CUSTOM_TEMPLATES[dataset]]
        images = seeded_images(cfg, batch, image_seed)
        logits = t.model_inference(images)
        raw = t.clip_model.visual(images)
        heads = width * 32 // 64
        exact = R.feature_error(R.image_features(rn, images, stages, heads), raw)
        emulated = R.emulated_rel(rn, images, stages, heads, raw)
        # what the number formats alone do to the logits: the emulated features against the reference's own text features
        emulated_logit = []
        for T in (torch.float16, torch.bfloat16):
            d = frozen["logit_scale"].exp().double() * O.unit(R.image_features(rn, images, stages, heads, T)) @ t.text_features.double().t() - logits.double()
            emulated_logit += [d.abs().max().item(), d.pow(2).mean().sqrt().item()]
    tokens = torch.stack([torch.cat([clip.tokenize(tp.format(c.replace("_", " "))) for c in names]) for tp in templates])
    labels = (torch.arange(batch) * 3 + 1) % len(names)
    out = {
        "config": np.array(repr(cfg.asdict())), "rn_stages": np.array(stages, dtype=np.int64), "rn_width": np.array(width, dtype=np.int64),
        "trainer": np.array(trainer), "dataset": np.array(dataset), "classnames": np.array(names),
        "templates": np.array(templates), "tokens": tokens.numpy().astype(np.int32),
        "seeds": np.array([frozen_seed, rn_seed, image_seed], dtype=np.int64), "labels": labels.numpy().astype(np.int64),
        "images_checksum": np.array([images.double().sum().item(), images.double().abs().sum().item()]),
        "logits": logits.numpy().astype(np.float32), "text_features": t.text_features.numpy().astype(np.float32),
        "image_features": raw.numpy().astype(np.float32), "logit_scale": np.array(frozen["logit_scale"].item(), dtype=np.float32),
        "emulated_rel": emulated.astype(np.float64), "emulated_logit": np.array(emulated_logit, dtype=np.float64),
    }
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(templates)} templates, logits {tuple(logits.shape)}, |features| {raw.norm(dim=1).tolist()}, float64 restatement {exact:.2e}, "
          f"emulated fp16 {emulated[0]:.2e} bf16 {emulated[1]:.2e}, emulated logits (max, rms) fp16 {emulated_logit[0]:.2e} {emulated_logit[1]:.2e} bf16 {emulated_logit[2]:.2e} {emulated_logit[3]:.2e}, {os.path.getsize(path) / 1e3:.1f} KB")


if __name__ == "__main__":
    tiny_text = dict(t_width=128, t_layers=3, t_heads=2, ctx_len=77, vocab=49408)
    rn50_text = dict(t_width=512, t_layers=12, t_heads=8, ctx_len=77, vocab=49408)
    # embed_dim = 16 width, RN50's own ratio (2048 channels -> 1024): the text tower's projection is [t_width, embed_dim] with embed_dim != t_width
    run_rn("rn_tiny", (1, 1, 1, 1), 32, 64, 512, tiny_text, "ZeroshotCLIP", "Caltech101", ZS_TINY_NAMES, 3, 31, 33, 35)
    run_rn("rn_tiny2", (2, 1, 2, 1), 64, 96, 1024, tiny_text, "ZeroshotCLIP2", "Caltech101", ZS_TINY_NAMES, 2, 31, 37, 39)  # 7 + the dataset's own
    run_rn("rn50_b2", (3, 4, 6, 3), 64, 224, 1024, rn50_text, "ZeroshotCLIP", "OxfordPets", CLASSNAMES, 2, 0, 41, 4321)
