"""Test-local restatement of the zero-shot trainers (trainers/zsclip.py) in plain torch CPU fp32, and the loader of the zsclip* fixtures.

``text_features`` restates ``encode_text`` (clip/model.py:825-838: token embedding + positional embedding, causal blocks, ln_final, the row
at ``text.argmax(dim=-1)`` times text_projection) followed by ZeroshotCLIP's single normalisation (zsclip.py:67-71) or ZeroshotCLIP2's
ensemble (zsclip.py:107-117); ``image_features`` the vanilla ViT (clip/model.py:478-496); ``forward`` model_inference (zsclip.py:74-79).
Built from ``oracle.mudpt_oracle``'s ``block`` / ``layer_norm`` / ``patchify`` / ``causal_mask``.  Pinned by the fixtures of
tests/golden/gen_golden_zsclip.py, which ran the reference's own classes (tests/test_zsclip_cpu.py).
"""
from __future__ import annotations

import ast
import os

import numpy as np
import torch

from oracle import mudpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["zsclip_tiny", "zsclip2_tiny", "zsclip2_tiny_imagenet", "zsclip_vitb16_b2", "zsclip2_vitb16_b2", "zsclip_vitb16_b2_s100",
            "zsclip2_vitb16_b2_s100"]


def encode_text(cfg: O.Config, sd, tokens: torch.Tensor) -> torch.Tensor:
    """clip/model.py:825-838 on tokens [C, ctx_len] -> raw text features [C, e]."""
    tokens = tokens.long()
    x = sd["token_embedding.weight"][tokens] + sd["positional_embedding"]
    mask = O.causal_mask(x.shape[1])
    for i in range(cfg.t_layers):
        x = O.block(x, sd, f"transformer.resblocks.{i}.", cfg.t_heads, mask)
    x = O.layer_norm(x, sd["ln_final.weight"], sd["ln_final.bias"])
    return x[torch.arange(x.shape[0]), tokens.argmax(dim=-1)] @ sd["text_projection"]


def text_features(cfg: O.Config, sd, tokens: torch.Tensor) -> torch.Tensor:
    """tokens [T, C, ctx_len].  T = 1: zsclip.py:67-71; more: zsclip.py:107-117, the templates in order."""
    if tokens.shape[0] == 1:
        f = encode_text(cfg, sd, tokens[0])
        return f / f.norm(dim=-1, keepdim=True)
    mean = 0
    for t in range(tokens.shape[0]):
        f = encode_text(cfg, sd, tokens[t])
        mean = mean + f / f.norm(dim=-1, keepdim=True)
    mean = mean / tokens.shape[0]
    return mean / mean.norm(dim=-1, keepdim=True)


def image_features(cfg: O.Config, sd, images: torch.Tensor) -> torch.Tensor:
    """clip/model.py:478-496: the vanilla ViT; raw features [B, e]."""
    B = images.shape[0]
    x = O.patchify(images.float(), cfg.patch) @ sd["visual.conv1.weight"].reshape(cfg.v_width, -1).t()
    x = torch.cat([sd["visual.class_embedding"].expand(B, 1, -1), x], dim=1) + sd["visual.positional_embedding"]
    x = O.layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
    for i in range(cfg.v_layers):
        x = O.block(x, sd, f"visual.transformer.resblocks.{i}.", cfg.v_heads, None)
    return O.layer_norm(x[:, 0], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"]


def forward(cfg: O.Config, sd, tokens: torch.Tensor, images: torch.Tensor) -> torch.Tensor:
    """zsclip.py:74-79 -> logits [B, C]."""
    img = image_features(cfg, sd, images)
    img = img / img.norm(dim=-1, keepdim=True)
    return sd["logit_scale"].exp() * img @ text_features(cfg, sd, tokens).t()


class ZsCase:
    """One tests/golden/zsclip*.npz fixture with its frozen weights rebuilt from the seeded recipe."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.name, self.z = name, z
        self.cfg = O.Config(**ast.literal_eval(str(z["config"])))
        fs, is_ = (int(v) for v in z["seeds"])
        self.frozen = O.make_frozen_state(self.cfg, fs)
        self.frozen["logit_scale"] = torch.tensor(float(z["logit_scale"]))
        self.trainer, self.dataset = str(z["trainer"]), str(z["dataset"])
        self.classnames = [str(v) for v in z["classnames"]]
        self.templates = [str(v) for v in z["templates"]]
        self.tokens = torch.from_numpy(z["tokens"])  # int32 [T, C, ctx_len]
        self.labels = torch.from_numpy(z["labels"])
        g = torch.Generator().manual_seed(is_)
        self.images = torch.randn(len(self.labels), 3, self.cfg.image_size, self.cfg.image_size, generator=g)
        chk = [self.images.double().sum().item(), self.images.double().abs().sum().item()]
        assert np.allclose(chk, z["images_checksum"], rtol=1e-12), "the seeded images are not the generator's"
        self.logits = torch.from_numpy(z["logits"])
        self.text_features = torch.from_numpy(z["text_features"])
        self.image_features = torch.from_numpy(z["image_features"])

    def shape(self):
        from mudpt_amd.model import ModelShape
        c = self.cfg
        return ModelShape(c.image_size, c.patch, c.v_width, c.v_layers, c.v_heads, c.t_width, c.t_layers, c.t_heads, c.ctx_len, c.embed_dim, 0, 1)


def merge_table_file(directory) -> str:
    """A gzip merge table (the tokenizer's file format) holding the rows of zsclip_merges.json at their ranks; the other ranks are filled with
    pairs no byte string can form, as tests/test_plugins_cpu.py does."""
    import gzip
    import json
    spec = json.load(open(os.path.join(GOLDEN, "zsclip_merges.json"), encoding="utf-8"))
    path = os.path.join(str(directory), "bpe_simple_vocab_16e6.txt.gz")
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write("\n".join(["#version: 0.2"] + [spec["merges"].get(str(r), f"一{r} 丁") for r in range(spec["n_merges"])]) + "\n")
    return path
