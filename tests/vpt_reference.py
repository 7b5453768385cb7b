"""Test-local restatement of the VPT / MPT paths (trainers/vpt.py, trainers/mpt.py) in plain torch CPU fp32, and the loader of the
vpt_* / mpt_* fixtures.

Batch-first restatement of ``ResidualAttentionBlock_VPT`` (clip/model.py:202-251) and the prompted ``VisionTransformer``
(clip/model.py:443-496): vision blocks 1 <= i < depth replace the LAST n_v rows with their own visual_ctx, text blocks replace rows
1..n_t; block 0 never splices.  The input vision prompt is appended after the positional embedding and before ln_pre, only if
0 < VISUAL_PROMPT_DEPTH <= 12; MPT's text_prompt_learner.visual_ctx takes rows 1..n_t of every class prompt BEFORE the positional
embedding is added (trainers/mpt.py:108-125,137).  The towers are ``oracle.mudpt_oracle``'s, fed these rows.  Pinned by the
fixtures of tests/golden/gen_golden_vpt.py, which ran the reference's own modules (tests/test_vpt_cpu.py).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from oracle import mudpt_oracle as O
from tests.helpers import GOLDEN, FixtureCase  # noqa: F401

FIXTURES = ["vpt_tiny", "vpt_tiny_shallow", "mpt_tiny", "mpt_tiny_textonly", "vpt_vitb16_b2", "mpt_vitb16_b2", "vpt_vitb16_b2_s100",
            "mpt_vitb16_b2_s100"]
TEXT_CTX = "text_prompt_learner.visual_ctx"


def vision_prompted(v_n_ctx: int, v_depth: int) -> bool:
    """clip/model.py:459: the vision prompt exists only for 0 < VISUAL_PROMPT_DEPTH <= 12 (and a non-empty row count)."""
    return v_n_ctx > 0 and 0 < v_depth <= 12


def trainable_keys(cfg: O.Config, trainer: str, shape: Sequence[int]) -> List[Tuple[str, Tuple[int, int]]]:
    """The reference's trainables in named_parameters() order (freeze rules vpt.py:141-146, mpt.py:195-202) and their shapes."""
    t_n, t_depth, v_n, v_depth = shape
    out = []
    if trainer == "MPT":
        out.append((TEXT_CTX, (t_n, cfg.t_width)))
        out += [(f"text_encoder.transformer.resblocks.{i}.visual_ctx", (t_n, cfg.t_width)) for i in range(1, min(t_depth, cfg.t_layers))]
    if vision_prompted(v_n, v_depth):
        out.append(("image_encoder.visual_ctx", (v_n, cfg.v_width)))
        out += [(f"image_encoder.transformer.resblocks.{i}.visual_ctx", (v_n, cfg.v_width)) for i in range(1, min(v_depth, cfg.v_layers))]
    return out


def seeded_prompts(cfg: O.Config, trainer: str, shape: Sequence[int], seed: int, text_ctx: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The fixtures' prompt values: 0.02 * N(0, 1) from ONE generator seeded with ``seed``, drawn in key order; MPT's text ctx is not
    drawn -- it keeps the reference's TEXT_CTX_INIT init (``text_ctx``, token_embedding rows 1..n_t of the init words)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shp in trainable_keys(cfg, trainer, shape):
        out[k] = text_ctx.clone() if k == TEXT_CTX else 0.02 * torch.randn(shp, generator=g)
    return out


def deep_rows(params, prefix: str, blocks: int) -> Optional[torch.Tensor]:
    """[blocks - 1, n, d]: the visual_ctx of blocks 1 .. blocks - 1 of one tower (each block owns its rows); None where there are none."""
    rows = [params[f"{prefix}.transformer.resblocks.{i}.visual_ctx"] for i in range(1, blocks)]
    return torch.stack(rows) if rows else None


def forward(cfg, sd, params, trainer, shape, class_embedding, eot, images, taps=None) -> torch.Tensor:
    """CustomCLIP.forward (vpt.py:94-111, mpt.py:156-172) -> logits [B, C].  taps: "vis.x_in.<i>" / "txt.x_in.<i>" = input of block i after
    its splice."""
    t_n, t_depth, v_n, v_depth = shape
    if vision_prompted(v_n, v_depth):
        img = O.vision_tower(cfg, sd, images, params["image_encoder.visual_ctx"], deep_rows(params, "image_encoder", min(v_depth, cfg.v_layers)), taps)
    else:
        img = O.vision_tower(cfg, sd, images, taps=taps)
    prompts, deep = class_embedding, None
    if trainer == "MPT":  # construct_prompts: [prefix, ctx, suffix] (mpt.py:97-125), then the blocks' own rows (mpt.py:129-146)
        C = prompts.shape[0]
        prompts = torch.cat([prompts[:, :1], params[TEXT_CTX].unsqueeze(0).expand(C, -1, -1), prompts[:, 1 + t_n:]], dim=1)
        deep = deep_rows(params, "text_encoder", min(t_depth, cfg.t_layers))
    return O.cosine_logits(sd, img, O.text_tower(cfg, sd, prompts, eot, deep, taps))


def forward_backward(cfg, sd, params, trainer, shape, class_embedding, eot, images, labels):
    """F.cross_entropy (vpt.py:168-200, mpt.py:224-256) and the gradient of every trainable -> (loss, logits, {key: grad})."""
    return O.loss_and_grads(lambda leaves: forward(cfg, sd, leaves, trainer, shape, class_embedding, eot, images), params, labels)


class VptCase(FixtureCase):
    """One tests/golden/vpt_*.npz / mpt_*.npz fixture with its prompts rebuilt from the seeded recipe."""

    def __init__(self, name: str):
        super().__init__(name)
        self.trainer = str(self.z["trainer"])
        self.shape = tuple(int(v) for v in self.z["prompt_shape"])
        text_ctx = self.frozen["token_embedding.weight"][self.ctx_token_ids] if self.trainer == "MPT" else None
        self.params = seeded_prompts(self.cfg, self.trainer, self.shape, self.seeds[1], text_ctx)
        self.keys = [k for k, _ in trainable_keys(self.cfg, self.trainer, self.shape)]
        self.load_grads()

    @property
    def variant(self) -> str:
        return self.trainer.lower()
