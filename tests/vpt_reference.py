"""Test-local restatement of the VPT / MPT paths (trainers/vpt.py, trainers/mpt.py) in plain torch CPU fp32, and the loader of the
vpt_* / mpt_* fixtures.

Batch-first restatement of ``ResidualAttentionBlock_VPT`` (clip/model.py:202-251) and the prompted ``VisionTransformer``
(clip/model.py:443-496): vision blocks 1 <= i < depth replace the LAST n_v rows with their own visual_ctx, text blocks replace rows
1..n_t; block 0 never splices.  The input vision prompt is appended after the positional embedding and before ln_pre, only if
0 < VISUAL_PROMPT_DEPTH <= 12; MPT's text_prompt_learner.visual_ctx takes rows 1..n_t of every class prompt BEFORE the positional
embedding is added (trainers/mpt.py:108-125,137).  The blocks themselves are the unchanged ``oracle.mudpt_oracle.block``.  Pinned by the
fixtures of tests/golden/gen_golden_vpt.py, which ran the reference's own modules (tests/test_vpt_cpu.py).
"""
from __future__ import annotations

import ast
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mudpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
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


def vision_tower(cfg: O.Config, sd, params, shape, images, taps: Optional[Dict] = None) -> torch.Tensor:
    """clip/model.py:478-496 with the VPT prompts -> image features [B, e].  taps: "vis.x_in.<i>" = input of block i after its splice."""
    _t_n, _t_depth, v_n, v_depth = shape
    B = images.shape[0]
    w = sd["visual.conv1.weight"].reshape(cfg.v_width, -1)
    x = O.patchify(images.float(), cfg.patch) @ w.t()
    x = torch.cat([sd["visual.class_embedding"].expand(B, 1, -1), x], dim=1) + sd["visual.positional_embedding"]
    prompted = vision_prompted(v_n, v_depth)
    if prompted:
        x = torch.cat([x, params["image_encoder.visual_ctx"].unsqueeze(0).expand(B, -1, -1)], dim=1)
    x = O.layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
    L = x.shape[1]
    for i in range(cfg.v_layers):
        if prompted and 1 <= i < v_depth:
            x = torch.cat([x[:, :L - v_n], params[f"image_encoder.transformer.resblocks.{i}.visual_ctx"].unsqueeze(0).expand(B, -1, -1)], dim=1)
        if taps is not None:
            taps[f"vis.x_in.{i}"] = x
        x = O.block(x, sd, f"visual.transformer.resblocks.{i}.", cfg.v_heads, None)
    return O.layer_norm(x[:, 0], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"]


def text_tower(cfg: O.Config, sd, params, trainer, shape, class_embedding, eot, taps: Optional[Dict] = None) -> torch.Tensor:
    """trainers/vpt.py:73-91 / mpt.py:129-146 -> text features [C, e]."""
    t_n, t_depth, _v_n, _v_depth = shape
    prompts = class_embedding
    C = prompts.shape[0]
    if trainer == "MPT":  # construct_prompts: [prefix, ctx, suffix] (mpt.py:97-125)
        prompts = torch.cat([prompts[:, :1], params[TEXT_CTX].unsqueeze(0).expand(C, -1, -1), prompts[:, 1 + t_n:]], dim=1)
    x = prompts + sd["positional_embedding"]
    mask = O.causal_mask(x.shape[1])
    for i in range(cfg.t_layers):
        if trainer == "MPT" and 1 <= i < t_depth:
            x = torch.cat([x[:, :1], params[f"text_encoder.transformer.resblocks.{i}.visual_ctx"].unsqueeze(0).expand(C, -1, -1), x[:, 1 + t_n:]], dim=1)
        if taps is not None:
            taps[f"txt.x_in.{i}"] = x
        x = O.block(x, sd, f"transformer.resblocks.{i}.", cfg.t_heads, mask)
    x = O.layer_norm(x, sd["ln_final.weight"], sd["ln_final.bias"])
    return x[torch.arange(C), eot] @ sd["text_projection"]


def forward(cfg, sd, params, trainer, shape, class_embedding, eot, images, taps=None) -> torch.Tensor:
    """CustomCLIP.forward (vpt.py:94-111, mpt.py:156-172) -> logits [B, C]."""
    img = vision_tower(cfg, sd, params, shape, images, taps)
    txt = text_tower(cfg, sd, params, trainer, shape, class_embedding, eot, taps)
    img = img / img.norm(dim=-1, keepdim=True)
    txt = txt / txt.norm(dim=-1, keepdim=True)
    return sd["logit_scale"].exp() * img @ txt.t()


def forward_backward(cfg, sd, params, trainer, shape, class_embedding, eot, images, labels):
    """F.cross_entropy (vpt.py:168-200, mpt.py:224-256) and the gradient of every trainable -> (loss, logits, {key: grad})."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    logits = forward(cfg, sd, leaves, trainer, shape, class_embedding, eot, images)
    loss = F.cross_entropy(logits, labels.long())
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad.detach() for k, v in leaves.items()}


class VptCase:
    """One tests/golden/vpt_*.npz / mpt_*.npz fixture with its frozen weights and prompts rebuilt from the seeded recipe."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.name, self.z = name, z
        self.cfg = O.Config(**ast.literal_eval(str(z["config"])))
        self.trainer = str(z["trainer"])
        self.shape = tuple(int(v) for v in z["prompt_shape"])
        fs, ts, is_ = (int(v) for v in z["seeds"])
        self.frozen = O.make_frozen_state(self.cfg, fs)
        self.frozen["logit_scale"] = torch.tensor(float(z["logit_scale"]))
        self.classnames = [str(v) for v in z["classnames"]]
        self.tokens = torch.from_numpy(z["tokenized_prompts"]).long()
        self.eot = self.tokens.argmax(dim=-1)
        self.class_embedding = self.frozen["token_embedding.weight"][self.tokens]
        self.ctx_token_ids = [int(v) for v in z["ctx_token_ids"]]
        text_ctx = self.frozen["token_embedding.weight"][self.ctx_token_ids] if self.trainer == "MPT" else None
        self.params = seeded_prompts(self.cfg, self.trainer, self.shape, ts, text_ctx)
        self.keys = [k for k, _ in trainable_keys(self.cfg, self.trainer, self.shape)]
        self.labels = torch.from_numpy(z["labels"])
        g = torch.Generator().manual_seed(is_)
        self.images = torch.randn(len(self.labels), 3, self.cfg.image_size, self.cfg.image_size, generator=g)
        self.logits = torch.from_numpy(z["logits"])
        self.loss = float(z["loss"])
        self.grads = {k: torch.from_numpy(z["grad." + k]) for k in self.keys}
        # sampled block inputs: "tap.<vis|txt>.<i>" [seq, rows, d] at the rows "tap.<vis|txt>.<i>.rows"
        self.taps = {k[4:]: (torch.from_numpy(z[k]), [int(r) for r in z[k + ".rows"]]) for k in z.files if k.startswith("tap.") and not k.endswith(".rows")}

    @property
    def variant(self) -> str:
        return self.trainer.lower()
