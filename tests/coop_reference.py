"""Test-local restatement of the CoOp path (trainers/coop.py) in plain torch CPU fp32, and the loader of the coop_* fixtures.

``construct_prompts`` restates trainers/coop.py:99-164 (the context rows at the end / in the middle / at the front of every class prompt,
shared or class-specific); the towers are ``oracle.mudpt_oracle.vision_tower`` without prompt rows (the vanilla ViT, coop.py:37) and
``text_tower`` (coop.py:187-200: positional embedding added AFTER the reordering, features at the EOT row).  Pinned by the fixtures of
tests/golden/gen_golden_coop.py, which ran the reference's own modules (tests/test_coop_cpu.py).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from oracle import mudpt_oracle as O
from tests.helpers import GOLDEN, FixtureCase  # noqa: F401

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


def text_features(cfg: O.Config, sd, ctx, class_embedding, eot, name_lens, position, taps: Optional[Dict] = None) -> torch.Tensor:
    """coop.py:187-200: the positional embedding is added AFTER the reordering.  taps: "prompts" = the class prompts [C, L, d]."""
    prompts = construct_prompts(ctx, class_embedding, cfg.n_ctx, name_lens, position)
    if taps is not None:
        taps["prompts"] = prompts
    return O.text_tower(cfg, sd, prompts, eot)


def forward(cfg: O.Config, sd, ctx, class_embedding, eot, name_lens, position, images, taps: Optional[Dict] = None) -> torch.Tensor:
    """trainers/coop.py:212-226 -> logits [B, C]: the vanilla ViT (coop.py:37) and the text tower on the constructed prompts."""
    img = O.vision_tower(cfg, sd, images)
    return O.cosine_logits(sd, img, text_features(cfg, sd, ctx, class_embedding, eot, name_lens, position, taps))


def forward_backward(cfg: O.Config, sd, ctx, class_embedding, eot, name_lens, position, images, labels, taps: Optional[Dict] = None):
    """F.cross_entropy (coop.py:281-296) and its gradient w.r.t. ctx.  taps (tests): "dprompts" [C, L, d] = the gradient w.r.t. every
    class prompt (the per-class terms the shared context's gradient sums over)."""
    inner = {}
    out = O.loss_and_grads(lambda leaf: forward(cfg, sd, leaf[CTX], class_embedding, eot, name_lens, position, images, inner), {CTX: ctx}, labels,
                           taps=inner, keep=() if taps is None else ("prompts",))
    if taps is not None:
        taps["dprompts"] = out[3]
    return out[0], out[1], out[2][CTX]


def ctx_rows(n_ctx: int, name_len: int, position: str):
    """Prompt rows of the n context rows of one class (coop.py:99-164)."""
    if position == "middle":
        return [1 + j if j < n_ctx // 2 else 1 + name_len + j for j in range(n_ctx)]
    if position == "front":
        return [1 + name_len + j for j in range(n_ctx)]
    return [1 + j for j in range(n_ctx)]


class CoopCase(FixtureCase):
    """One tests/golden/coop_*.npz fixture: the stored context, where the class token sits and how long each class name is."""

    def __init__(self, name: str):
        super().__init__(name)
        z = self.z
        self.csc = bool(z["csc"])
        self.position = str(z["class_token_position"])
        self.name_lens = [int(v) for v in z["name_lens"]]
        self.ctx = torch.from_numpy(z["ctx"])
        self.dctx = torch.from_numpy(z["grad." + CTX])

    @property
    def variant(self) -> str:
        return "coop_csc" if self.csc else "coop"
