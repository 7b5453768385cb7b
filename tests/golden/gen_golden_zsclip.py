"""Generate the zero-shot golden vectors (tests/golden/zsclip*.npz, zsclip_templates.json, zsclip_merges.json) by running the REFERENCE's own
``trainers.zsclip.ZeroshotCLIP`` / ``ZeroshotCLIP2``.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/gen_golden_zsclip.py

What runs: the reference's ``build_model`` and ``model_inference`` (trainers/zsclip.py:53-79,89-118), unmodified, on a bare instance that
carries what they read -- ``cfg.DATASET.NAME`` / ``cfg.MODEL.BACKBONE.NAME``, ``dm.dataset.classnames`` and ``device = "cpu"`` -- imported with
the placeholders of gen_golden.py, on torch CPU fp32.  One patch: ``trainers.zsclip.load_clip_to_cpu`` (a download or a checkpoint file) is
replaced by a function that returns ``clip.model.CLIP(..., cfg=None).float()`` loaded with ``oracle.mudpt_oracle.make_frozen_state`` (the
fixture stores the seed, not the weights).  ``ZeroshotCLIP2.templates`` is reset to its first 7 entries before each run: ``build_model``
appends to the class-level list in place (:101-102).  Stored per fixture: config, trainer, dataset name, class names, the template strings,
``tokens`` int32 [T, C, 77] (clip.tokenize of every template and class), seeds, labels, the images' checksum, logits, the final
``text_features`` [C, e], the raw ``image_features`` [B, e] (clip_model.visual(image), what lpclip/feat_extractor.py:125 extracts) and
logit_scale.  The two JSON files: the reference's CUSTOM_TEMPLATES / IMAGENET_TEMPLATES_SELECT as data, and the BPE merge rows the fixtures'
prompts use (the rule of gen_golden.run_tokenizer_merges), so the native tokenizer is held to the recorded ids without the full table.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import CLASSNAMES, REFERENCE, ROOT, O, import_reference, seeded_images, with_logit_scale  # noqa: E402
from gen_golden_vpt import TINY_NAMES  # noqa: E402

ZS_TINY_NAMES = TINY_NAMES + ["crocodile_head"]  # a Caltech-101 name with an underscore (zsclip.py:62 replaces it by a space)
PROMPTS_SEEN = []


def run_zs(cfg: O.Config, name: str, trainer: str, dataset: str, classnames, batch: int, frozen_seed: int, image_seed: int, logit_scale=None):
    names = list(classnames)
    clip, cm, _mudpt, CN = import_reference()
    from trainers import zsclip
    frozen = with_logit_scale(O.make_frozen_state(cfg, frozen_seed), logit_scale)

    def load_clip_to_cpu(_cfg):
        model = cm.CLIP(cfg.embed_dim, cfg.image_size, cfg.v_layers, cfg.v_width, cfg.patch, cfg.ctx_len, cfg.vocab, cfg.t_width,
                        cfg.t_heads, cfg.t_layers, None).float()
        missing, unexpected = model.load_state_dict(frozen, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
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
    tokens = torch.stack([torch.cat([clip.tokenize(tp.format(c.replace("_", " "))) for c in names]) for tp in templates])
    PROMPTS_SEEN.extend(tp.format(c.replace("_", " ")) for tp in templates for c in names)
    labels = (torch.arange(batch) * 3 + 1) % len(names)
    out = {
        "config": np.array(repr(cfg.asdict())), "trainer": np.array(trainer), "dataset": np.array(dataset), "classnames": np.array(names),
        "templates": np.array(templates), "tokens": tokens.numpy().astype(np.int32),
        "seeds": np.array([frozen_seed, image_seed], dtype=np.int64), "labels": labels.numpy().astype(np.int64),
        "images_checksum": np.array([images.double().sum().item(), images.double().abs().sum().item()]),
        "logits": logits.numpy().astype(np.float32), "text_features": t.text_features.numpy().astype(np.float32),
        "image_features": raw.numpy().astype(np.float32), "logit_scale": np.array(frozen["logit_scale"].item(), dtype=np.float32),
    }
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(templates)} templates, logits {tuple(logits.shape)}, {os.path.getsize(path) / 1e3:.1f} KB")


def write_templates():
    import_reference()
    from trainers import zsclip
    from trainers.imagenet_templates import IMAGENET_TEMPLATES_SELECT
    path = os.path.join(ROOT, "tests", "golden", "zsclip_templates.json")
    with open(path, "w") as f:
        json.dump({"CUSTOM_TEMPLATES": dict(zsclip.CUSTOM_TEMPLATES), "IMAGENET_TEMPLATES_SELECT": list(IMAGENET_TEMPLATES_SELECT)}, f, indent=1)
    print(f"wrote {path}")


def write_merges(texts):
    """zsclip_merges.json by the rule of gen_golden.run_tokenizer_merges: every merge greedy BPE applies to the fixtures' prompts, plus every
    merge that spells the same token as one of them, under their ranks."""
    from mudpt_amd import tokenizer
    tok = tokenizer.BPETokenizer(tokenizer.find_vocab(os.path.join(REFERENCE, "clip", tokenizer.VOCAB_FILE)))
    by_rank = {r: m for m, r in tok.rank.items()}
    used = set()
    orig = tok._merge

    def recording_merge(symbols):
        out = list(symbols)
        while len(out) > 1:
            ranked = [tok.rank[p] for p in zip(out, out[1:]) if p in tok.rank]
            if not ranked:
                break
            used.add(min(ranked))
            (a, b), nxt, i = by_rank[min(ranked)], [], 0
            while i < len(out):
                if i + 1 < len(out) and out[i] == a and out[i + 1] == b:
                    nxt.append(a + b)
                    i += 2
                else:
                    nxt.append(out[i])
                    i += 1
            out = nxt
        assert out == orig(symbols)
        return out
    tok._merge = recording_merge
    for t in sorted(set(texts)):
        tok.encode(t)
    spelled = {"".join(by_rank[r]) for r in used}
    keep = sorted(r for r, m in by_rank.items() if "".join(m) in spelled)
    path = os.path.join(ROOT, "tests", "golden", "zsclip_merges.json")
    with open(path, "w") as f:
        json.dump({"n_merges": tokenizer.N_MERGES, "merges": {str(r): " ".join(by_rank[r]) for r in keep}}, f, ensure_ascii=False, indent=0)
    print(f"wrote {path}: {len(keep)} of {tokenizer.N_MERGES} merges")


if __name__ == "__main__":
    tiny, b16 = O.TINY, O.VIT_B16
    run_zs(tiny, "zsclip_tiny", "ZeroshotCLIP", "Caltech101", ZS_TINY_NAMES, 3, 21, 23)
    run_zs(tiny, "zsclip2_tiny", "ZeroshotCLIP2", "Caltech101", ZS_TINY_NAMES, 3, 21, 23)            # 7 + the dataset's own
    run_zs(tiny, "zsclip2_tiny_imagenet", "ZeroshotCLIP2", "ImageNet", ZS_TINY_NAMES, 3, 21, 23)     # the 7 alone
    run_zs(b16, "zsclip_vitb16_b2", "ZeroshotCLIP", "OxfordPets", CLASSNAMES, 2, 0, 4321)
    run_zs(b16, "zsclip2_vitb16_b2", "ZeroshotCLIP2", "OxfordPets", CLASSNAMES, 2, 0, 4321)
    run_zs(b16, "zsclip_vitb16_b2_s100", "ZeroshotCLIP", "OxfordPets", CLASSNAMES, 2, 0, 4321, logit_scale=100.0)
    run_zs(b16, "zsclip2_vitb16_b2_s100", "ZeroshotCLIP2", "OxfordPets", CLASSNAMES, 2, 0, 4321, logit_scale=100.0)
    write_templates()
    write_merges(PROMPTS_SEEN)
