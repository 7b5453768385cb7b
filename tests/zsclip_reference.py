"""Test-local restatement of the zero-shot trainers (trainers/zsclip.py) in plain torch CPU fp32, and the loader of the zsclip* fixtures.

``text_features`` restates ``encode_text`` (clip/model.py:825-838: token embedding + positional embedding, causal blocks, ln_final, the row
at ``text.argmax(dim=-1)`` times text_projection) followed by ZeroshotCLIP's single normalisation (zsclip.py:67-71) or ZeroshotCLIP2's
ensemble (zsclip.py:107-117); ``image_features`` the vanilla ViT (clip/model.py:478-496); ``forward`` model_inference (zsclip.py:74-79).
Both towers are ``oracle.mudpt_oracle``'s, without prompt rows.  Pinned by the fixtures of
tests/golden/gen_golden_zsclip.py, which ran the reference's own classes (tests/test_zsclip_cpu.py).
"""
from __future__ import annotations

import os

import torch

from oracle import mudpt_oracle as O
from tests.helpers import GOLDEN, FixtureCase  # noqa: F401

FIXTURES = ["zsclip_tiny", "zsclip2_tiny", "zsclip2_tiny_imagenet", "zsclip_vitb16_b2", "zsclip2_vitb16_b2", "zsclip_vitb16_b2_s100",
            "zsclip2_vitb16_b2_s100"]


def encode_text(cfg: O.Config, sd, tokens: torch.Tensor) -> torch.Tensor:
    """clip/model.py:825-838 on tokens [C, ctx_len] -> raw text features [C, e]."""
    tokens = tokens.long()
    return O.text_tower(cfg, sd, sd["token_embedding.weight"][tokens], tokens.argmax(dim=-1))


def text_features(cfg: O.Config, sd, tokens: torch.Tensor) -> torch.Tensor:
    """tokens [T, C, ctx_len].  T = 1: zsclip.py:67-71; more: zsclip.py:107-117, the templates in order."""
    if tokens.shape[0] == 1:
        return O.unit(encode_text(cfg, sd, tokens[0]))
    mean = 0
    for t in range(tokens.shape[0]):
        mean = mean + O.unit(encode_text(cfg, sd, tokens[t]))
    mean = mean / tokens.shape[0]
    return O.unit(mean)


def image_features(cfg: O.Config, sd, images: torch.Tensor) -> torch.Tensor:
    """clip/model.py:478-496: the vanilla ViT; raw features [B, e]."""
    return O.vision_tower(cfg, sd, images)


def forward(cfg: O.Config, sd, tokens: torch.Tensor, images: torch.Tensor) -> torch.Tensor:
    """zsclip.py:74-79 -> logits [B, C]."""
    return sd["logit_scale"].exp() * O.unit(image_features(cfg, sd, images)) @ text_features(cfg, sd, tokens).t()


class ZsCase(FixtureCase):
    """One tests/golden/zsclip*.npz fixture: the templates and their tokens, the reference's features."""

    def __init__(self, name: str):
        super().__init__(name)
        z = self.z
        self.trainer, self.dataset = str(z["trainer"]), str(z["dataset"])
        self.templates = [str(v) for v in z["templates"]]
        self.tokens = torch.from_numpy(z["tokens"])  # int32 [T, C, ctx_len]
        self.text_features = torch.from_numpy(z["text_features"])
        self.image_features = torch.from_numpy(z["image_features"])

    def shape(self):
        from mudpt_amd.model import ModelShape
        return ModelShape.from_config(self.cfg, 0, 1)


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
