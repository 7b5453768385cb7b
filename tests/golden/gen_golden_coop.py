"""Generate the CoOp golden vectors (tests/golden/coop_*.npz) by running the REFERENCE's own ``trainers.coop.CustomCLIP``.

Run in the build container only (needs /root/reference, which never travels to the GPU box):

    python tests/golden/gen_golden_coop.py          # every coop_*.npz and coop_name_merges.json

What runs: ``trainers.coop.CustomCLIP`` over ``clip.model.CLIP(..., None)`` (the vanilla CLIP, trainers/coop.py:37), imported unmodified
with the placeholders of gen_golden.py, on torch CPU fp32.  The frozen weights follow ``oracle.mudpt_oracle.make_frozen_state``; the context
is the reference's own N(0, 0.02^2) draw (coop.py:63-71) after ``torch.manual_seed(train_seed)`` and is stored in the fixture (it is small).
Stored per fixture: config, class names, the reference's ``prompt_learner.name_lens``, tokenized prompts, seeds, ctx, labels, the images'
checksum, eval logits, training loss, the ctx gradient and logit_scale.  coop_name_merges.json holds the rows of CLIP's BPE merge table the
class names use (the rule of gen_golden.run_tokenizer_merges), so the native tokenizer's name lengths can be checked without the full table.
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import CLASSNAMES, REFERENCE, ROOT, O, import_reference, many_classnames, seeded_images, with_logit_scale  # noqa: E402

# 7 names of 1, 2 and 3 BPE tokens: the middle / front splices move the context by a different number of rows per class
TINY_NAMES = ["face", "water lily", "hawksbill turtle", "leopard", "stop sign", "brontosaurus", "crayfish"]


def run_coop(cfg: O.Config, name: str, batch: int, csc: bool, position: str, frozen_seed: int, train_seed: int, image_seed: int,
             classnames=None, logit_scale=None):
    names = list(classnames or CLASSNAMES)
    _clip, cm, _mudpt, CN = import_reference()
    from trainers import coop
    ycfg = CN(TRAINER=CN(NAME="CoOp", COOP=CN(N_CTX=cfg.n_ctx, CTX_INIT="", PREC="fp32", CSC=csc, CLASS_TOKEN_POSITION=position)),
              INPUT=CN(SIZE=(cfg.image_size, cfg.image_size)))
    ref_clip = cm.CLIP(cfg.embed_dim, cfg.image_size, cfg.v_layers, cfg.v_width, cfg.patch, cfg.ctx_len,
                       cfg.vocab, cfg.t_width, cfg.t_heads, cfg.t_layers, None).float()
    frozen = with_logit_scale(O.make_frozen_state(cfg, frozen_seed), logit_scale)
    missing, unexpected = ref_clip.load_state_dict(frozen, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    torch.manual_seed(train_seed)  # the reference draws ctx with nn.init.normal_ (coop.py:71) from the global generator
    model = coop.CustomCLIP(ycfg, names, ref_clip)
    for k, p in model.named_parameters():  # freeze rule, trainers/coop.py:240-243
        p.requires_grad_("prompt_learner" in k)
    assert [k for k, p in model.named_parameters() if p.requires_grad] == ["prompt_learner.ctx"]
    ctx = model.prompt_learner.ctx
    assert tuple(ctx.shape) == ((len(names),) if csc else ()) + (cfg.n_ctx, cfg.t_width)
    images = seeded_images(cfg, batch, image_seed)
    labels = (torch.arange(batch) * 3 + 1) % len(names)
    model.eval()
    with torch.no_grad():
        logits = model(images)
    model.train()
    loss = torch.nn.functional.cross_entropy(model(images), labels)  # trainers/coop.py:281-296
    loss.backward()
    out = {
        "config": np.array(repr(cfg.asdict())), "classnames": np.array(names),
        "csc": np.array(csc), "class_token_position": np.array(position),
        "name_lens": np.array(model.prompt_learner.name_lens, dtype=np.int32),
        "seeds": np.array([frozen_seed, train_seed, image_seed], dtype=np.int64),
        "tokenized_prompts": model.tokenized_prompts.numpy().astype(np.int32),
        "ctx": ctx.detach().numpy().astype(np.float32), "labels": labels.numpy().astype(np.int64),
        "images_checksum": np.array([images.double().sum().item(), images.double().abs().sum().item()]),
        "logits": logits.numpy(), "loss": np.array(loss.item(), dtype=np.float64),
        "grad.prompt_learner.ctx": ctx.grad.detach().numpy(),
        "logit_scale": np.array(frozen["logit_scale"].item(), dtype=np.float32),
    }
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss {loss.item():.6f}, name_lens {sorted(set(out['name_lens'].tolist()))}, {os.path.getsize(path) / 1e6:.3f} MB")
    return names


def run_name_merges(names):
    """coop_name_merges.json: the merge-table rows BPE applies to the class names (+ every row spelling the same token), at their ranks."""
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
    for t in names:
        tok.encode(t)
    spelled = {"".join(by_rank[r]) for r in used}
    keep = sorted(r for r, m in by_rank.items() if "".join(m) in spelled)
    path = os.path.join(ROOT, "tests", "golden", "coop_name_merges.json")
    with open(path, "w") as f:
        json.dump({"n_merges": tokenizer.N_MERGES, "merges": {str(r): " ".join(by_rank[r]) for r in keep}}, f, ensure_ascii=False, indent=0)
    print(f"wrote {path}: {len(keep)} of {tokenizer.N_MERGES} merges")


if __name__ == "__main__":
    tiny = dataclasses.replace(O.TINY, n_ctx=5, depth=1)  # odd n_ctx: middle splits it 2 + 3 (coop.py:122)
    b16 = dataclasses.replace(O.VIT_B16, depth=1)
    names = set()
    for csc in (False, True):
        for pos in ("end", "middle", "front"):
            names.update(run_coop(tiny, f"coop_tiny_{pos}" + ("_csc" if csc else ""), 3, csc, pos, 21, 22, 23, TINY_NAMES))
    names.update(run_coop(dataclasses.replace(b16, n_ctx=16), "coop_vitb16_middle_b2", 2, False, "middle", 0, 2, 4321))  # vit_b16_ep50 defaults
    names.update(run_coop(dataclasses.replace(b16, n_ctx=4), "coop_vitb16_csc_front_b2", 2, True, "front", 0, 3, 4321))
    names.update(run_coop(dataclasses.replace(b16, n_ctx=4, patch=32), "coop_vitb32_end_b4", 4, False, "end", 3, 4, 55))  # scripts/coop/train_base2new.sh
    names.update(run_coop(dataclasses.replace(b16, n_ctx=16), "coop_vitb16_c208_middle_b2", 2, False, "middle", 0, 6, 777, many_classnames(208)))
    names.update(run_coop(dataclasses.replace(b16, n_ctx=16), "coop_vitb16_b2_s100", 2, False, "end", 0, 2, 4321, logit_scale=100.0))
    run_name_merges(sorted(n.replace("_", " ") for n in names))
