"""Test-local restatement of the CoOp path (trainers/coop.py) in plain torch CPU fp32, and the loader of the coop_* fixtures.

``construct_prompts`` restates trainers/coop.py:99-164 (the context rows at the end / in the middle / at the front of every class prompt,
shared or class-specific); the towers are the unchanged ``oracle.cocoop_oracle.vision_tower`` (the vanilla ViT, coop.py:37) and
``text_tower`` (coop.py:187-200: positional embedding added AFTER the reordering, features at the EOT row).  Pinned by the fixtures of
tests/golden/gen_golden_coop.py, which ran the reference's own modules (tests/test_coop_cpu.py).
"""
from __future__ import annotations

import ast
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cocoop_oracle as CO
from oracle import mudpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["coop_tiny_end", "coop_tiny_middle", "coop_tiny_front", "coop_tiny_end_csc", "coop_tiny_middle_csc", "coop_tiny_front_csc",
            "coop_vitb16_middle_b2", "coop_vitb16_csc_front_b2", "coop_vitb32_end_b4", "coop_vitb16_c208_middle_b2", "coop_vitb16_b2_s100"]
CTX = "prompt_learner.ctx"


def construct_prompts(ctx: torch.Tensor, class_embedding: torch.Tensor, n_ctx: int, name_lens: Sequence[int], position: str) -> torch.Tensor:
    """trainers/coop.py:99-175: ctx [n, d] (shared) or [C, n, d] (CSC); class_embedding = token_embedding(tokenized) [C, L, d]."""
    C = class_embedding.shape[0]
    if ctx.dim() == 2:
        ctx = ctx.unsqueeze(0).expand(C, -1, -1)
    prefix, suffix = class_embedding[:, :1], class_embedding[:, 1 + n_ctx:]
    if position == "end":
        return torch.cat([prefix, ctx, suffix], dim=1)
    h, rows = n_ctx // 2, []
    for i in range(C):
        nl = int(name_lens[i])
        if position == "middle":
            parts = [prefix[i:i + 1], ctx[i:i + 1, :h], suffix[i:i + 1, :nl], ctx[i:i + 1, h:], suffix[i:i + 1, nl:]]
        elif position == "front":
            parts = [prefix[i:i + 1], suffix[i:i + 1, :nl], ctx[i:i + 1], suffix[i:i + 1, nl:]]
        else:
            raise NotImplementedError(position)
        rows.append(torch.cat(parts, dim=1))
    return torch.cat(rows, dim=0)


def text_features(cfg: O.Config, sd, ctx, class_embedding, eot, name_lens, position) -> torch.Tensor:
    return CO.text_tower(cfg, sd, construct_prompts(ctx, class_embedding, cfg.n_ctx, name_lens, position), eot)


def forward(cfg: O.Config, sd, ctx, class_embedding, eot, name_lens, position, images) -> torch.Tensor:
    """trainers/coop.py:212-226 -> logits [B, C]."""
    img = CO.vision_tower(cfg, sd, images)
    txt = text_features(cfg, sd, ctx, class_embedding, eot, name_lens, position)
    img = img / img.norm(dim=-1, keepdim=True)
    txt = txt / txt.norm(dim=-1, keepdim=True)
    return sd["logit_scale"].exp() * img @ txt.t()


def forward_backward(cfg: O.Config, sd, ctx, class_embedding, eot, name_lens, position, images, labels, taps: Optional[Dict] = None):
    """F.cross_entropy (coop.py:281-296) and its gradient w.r.t. ctx.  taps (tests): "dprompts" [C, L, d] = the gradient w.r.t. every
    class prompt (the per-class terms the shared context's gradient sums over)."""
    leaf = ctx.detach().clone().requires_grad_(True)
    img = CO.vision_tower(cfg, sd, images)
    prompts = construct_prompts(leaf, class_embedding, cfg.n_ctx, name_lens, position)
    if taps is not None:
        prompts.retain_grad()
    txt = CO.text_tower(cfg, sd, prompts, eot)
    img = img / img.norm(dim=-1, keepdim=True)
    txt = txt / txt.norm(dim=-1, keepdim=True)
    logits = sd["logit_scale"].exp() * img @ txt.t()
    loss = F.cross_entropy(logits, labels.long())
    loss.backward()
    if taps is not None:
        taps["dprompts"] = prompts.grad.detach()
    return loss.detach(), logits.detach(), leaf.grad.detach()


def ctx_rows(n_ctx: int, name_len: int, position: str):
    """Prompt rows of the n context rows of one class (coop.py:99-164)."""
    if position == "middle":
        return [1 + j if j < n_ctx // 2 else 1 + name_len + j for j in range(n_ctx)]
    if position == "front":
        return [1 + name_len + j for j in range(n_ctx)]
    return [1 + j for j in range(n_ctx)]


class CoopCase:
    """One tests/golden/coop_*.npz fixture with its frozen weights rebuilt from the seeded recipe."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.name, self.z = name, z
        self.cfg = O.Config(**ast.literal_eval(str(z["config"])))
        fs, _ts, is_ = (int(v) for v in z["seeds"])
        self.frozen = O.make_frozen_state(self.cfg, fs)
        self.frozen["logit_scale"] = torch.tensor(float(z["logit_scale"]))
        self.classnames = [str(v) for v in z["classnames"]]
        self.csc = bool(z["csc"])
        self.position = str(z["class_token_position"])
        self.name_lens = [int(v) for v in z["name_lens"]]
        self.tokens = torch.from_numpy(z["tokenized_prompts"]).long()
        self.eot = self.tokens.argmax(dim=-1)
        self.class_embedding = self.frozen["token_embedding.weight"][self.tokens]
        self.ctx = torch.from_numpy(z["ctx"])
        self.labels = torch.from_numpy(z["labels"])
        g = torch.Generator().manual_seed(is_)
        self.images = torch.randn(len(self.labels), 3, self.cfg.image_size, self.cfg.image_size, generator=g)
        self.logits = torch.from_numpy(z["logits"])
        self.loss = float(z["loss"])
        self.dctx = torch.from_numpy(z["grad." + CTX])

    @property
    def variant(self) -> str:
        return "coop_csc" if self.csc else "coop"
