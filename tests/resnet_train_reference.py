"""Loader of the rn*_coop* / rn*_cocoop* fixtures (tests/golden/gen_golden_resnet_train.py: the reference's own trainers/coop.py and
trainers/cocoop.py ``CustomCLIP`` over a CLIP with the ResNet image tower) and the test-local restatement of both forwards behind the raw
image features: CoOp as tests/coop_reference.py, CoCoOp as oracle/cocoop_oracle.py, the tower as tests/resnet_reference.image_features.

The emulated tower terms of a fixture are what the tower's number formats alone cost: the reference's own modules run once more with
``image_encoder`` replaced by the float64 restatement rounded to T at the library's five sites (tests/resnet_reference.py), and the deviation
of the logits (max, rms) and of every gradient (max and rms of the difference, relative to the gradient's rms) from the unreplaced run.
"""
from __future__ import annotations

import torch

from oracle import cocoop_oracle as CO
from oracle import mudpt_oracle as O
from tests import coop_reference as CR
from tests import resnet_reference as R
from tests.helpers import FixtureCase

FIXTURES = ["rn_coop_tiny", "rn_coop_tiny2_csc", "rn_cocoop_tiny", "rn50_coop_b2", "rn50_cocoop_b1"]
TINY = [f for f in FIXTURES if "tiny" in f]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


class RnTrainCase(FixtureCase):
    """``cfg`` describes the text side and the prompt (its ViT fields only seed ``frozen``'s draws); ``state`` is the CLIP state dict: the
    text side of ``frozen`` and the tower of ``make_rn_state``.  seeds: frozen, tower, trainables, images."""

    def __init__(self, name: str):
        super().__init__(name)
        z = self.z
        self.trainer = str(z["trainer"])
        self.cocoop = self.trainer == "CoCoOp"
        self.stages, self.width = tuple(int(v) for v in z["rn_stages"]), int(z["rn_width"])
        self.heads = self.width * 32 // 64
        self.image_features = torch.from_numpy(z["image_features"])
        self.rn = R.make_rn_state(R.RnShape(self.stages, self.width, self.cfg.image_size, self.cfg.embed_dim), self.seeds[1])
        self.state = {k: v for k, v in self.frozen.items() if not k.startswith("visual.")}
        self.state.update(self.rn)
        if self.cocoop:
            self.keys = list(CO.TRAINABLE_ORDER)
            self.params = CO.make_trainable_state(self.cfg, self.seeds[2], self.frozen, self.ctx_token_ids)
            self.variant, self.csc, self.position, self.name_lens = "cocoop", False, "end", None
        else:
            self.keys = [CR.CTX]
            self.csc, self.position = bool(z["csc"]), str(z["class_token_position"])
            self.name_lens = [int(v) for v in z["name_lens"]]
            self.params = {CR.CTX: torch.from_numpy(z["ctx"])}
            self.variant = "coop_csc" if self.csc else "coop"
        self.load_grads()
        self.emulated_logit = {d: tuple(float(v) for v in z["emulated_logit"][2 * i:2 * i + 2]) for i, d in enumerate(DTYPES)}  # (max, rms)
        self.emulated_grad = {k: {d: tuple(float(v) for v in z["emulated_grad." + k][2 * i:2 * i + 2]) for i, d in enumerate(DTYPES)} for k in self.keys}

    def shape(self):
        from mudpt_amd.model import ModelShape
        return ModelShape.from_state_dict(self.state, self.cfg.n_ctx, 1)


_CASES = {}


def case(name: str) -> RnTrainCase:
    """The fixture, loaded once per process and shared (its tensors are not to be written)."""
    if name not in _CASES:
        _CASES[name] = RnTrainCase(name)
    return _CASES[name]


def logits_from_features(c: RnTrainCase, feat: torch.Tensor, params=None) -> torch.Tensor:
    """The trainer's forward behind ``clip_model.visual(image)`` (trainers/coop.py:214-226, cocoop.py:182-198): the oracle's text tower, in
    fp32 as the reference ran it, on the tower's features rounded to fp32 once (as tests/test_resnet_cpu.py forms its logits)."""
    sd, params, emb, feat = c.frozen, params or c.params, c.class_embedding, feat.float()
    if not c.cocoop:
        return O.cosine_logits(sd, feat, CR.text_features(c.cfg, sd, params[CR.CTX], emb, c.eot, c.name_lens, c.position))
    B, C = feat.shape[0], emb.shape[0]
    img = O.unit(feat)
    prompts = CO.prompts_for(c.cfg, params, emb, img).reshape(B * C, c.cfg.ctx_len, c.cfg.t_width)
    txt = O.unit(O.text_tower(c.cfg, sd, prompts, c.eot.repeat(B)).reshape(B, C, -1))
    return sd["logit_scale"].exp() * torch.einsum("be,bce->bc", img, txt)


def restated_logits(c: RnTrainCase, round_to=None) -> torch.Tensor:
    with torch.no_grad():
        return logits_from_features(c, R.image_features(c.rn, c.images, c.stages, c.heads, round_to))
