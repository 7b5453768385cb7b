"""Test-local restatement of the UUMuDPT path (trainers/uumudpt.py:80-233, clip/model.py:600-664) in plain torch CPU, and the loader of the
uumudpt_* fixtures.

UUMuDPT is UMuDPT with the coupling in both directions.  Gen1, the prompt learner's generator, is UMuDPT's under the prefix
``uumudpt_prompt_learner.``: G [D, n, d_v] = Gen1(cat(ctx, deep_prompts)).  The vision tower owns ``visual_ctx`` [n, d_v],
``visual_ctx_deep_prompts`` [D - 1, n, d_v] and Gen2, the same pipeline (LayerNorm -> one pre-LN block -> LayerNorm -> Linear) at width d_v
with d_v / 64 heads and output width e: T [D - 1, n, e] = Gen2(visual_ctx_deep_prompts).  Vision input prompt rows G[0] + visual_ctx, vision
deep prompts G[1:] + visual_ctx_deep_prompts, text deep prompts deep_prompts + T (uumudpt.py:224: needs e == d_t), text input rows ctx.  The
blocks are MuDPT's (``ResidualAttentionBlock_UUMuDPT``), so both towers are ``oracle.mudpt_oracle``'s, fed the sums.

Both generators ARE :func:`tests.umudpt_reference.generator` / ``generator_backward``: :func:`gen_params` renames one generator's 18 tensors
to the keys those functions read; nothing of them is restated here.  Pinned by the fixtures of tests/golden/gen_golden_uumudpt.py, which ran the
reference's own modules (tests/test_uumudpt_cpu.py).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from oracle import mudpt_oracle as O
from tests import umudpt_reference as U
from tests.umudpt_reference import SAMPLE_ABOVE, SAMPLE_ROWS, sample_rows  # noqa: F401  (the fixtures' sampling rule is UMuDPT's)

GOLDEN = U.GOLDEN
TINY_SAMPLE_ABOVE = 32768  # the tiny fixtures sample already above this (each fixture stores its threshold): every file stays under 1 MiB
FIXTURES = ["uumudpt_tiny", "uumudpt_tiny_d1", "uumudpt_tiny_d5", "uumudpt_vitb16_b2", "uumudpt_vitb16_b2_s100"]
P, V = "uumudpt_prompt_learner.", "image_encoder.visual_ctx"
CTX, DEEP, VCTX, VDEEP = P + "ctx", P + "deep_prompts", V, V + "_deep_prompts"
# (ln_pre, self_attn, ln_post, output Linear) of each generator, as full key prefixes
GEN1 = (P + "ln_pre", P + "self_attn", P + "ln_post", P + "visual_proj")
GEN2 = (V + "_ln_intra_pre", V + "_self_attn", V + "_ln_intra_post", V + "_text_proj")
_INNER = [("attn.in_proj_weight", 3, 1), ("attn.in_proj_bias", 3, 0), ("attn.out_proj.weight", 1, 1), ("attn.out_proj.bias", 1, 0), ("ln_1.weight", 1, 0),
          ("ln_1.bias", 1, 0), ("mlp.c_fc.weight", 4, 1), ("mlp.c_fc.bias", 4, 0), ("mlp.c_proj.weight", 1, 4), ("mlp.c_proj.bias", 1, 0),
          ("ln_2.weight", 1, 0), ("ln_2.bias", 1, 0)]  # (key, rows / d, columns / d or 0 for a vector)


def generator_keys(names, d: int, d_out: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """The 18 tensors of one generator of width d and output width d_out, in named_parameters() order."""
    pre, attn, post, proj = names
    out = [(pre + ".weight", (d,)), (pre + ".bias", (d,))]
    out += [(attn + "." + k, (r * d, c * d) if c else (r * d,)) for k, r, c in _INNER]
    return out + [(post + ".weight", (d,)), (post + ".bias", (d,)), (proj + ".weight", (d_out, d)), (proj + ".bias", (d_out,))]


def trainable_keys(cfg: O.Config) -> List[Tuple[str, Tuple[int, ...]]]:
    """The reference's 40 trainables -- every parameter whose name contains "prompt_learner" or "visual_ctx" (uumudpt.py:255-261) -- in
    named_parameters() order, with their shapes.  cfg.n_ctx / cfg.depth are TRAINER.UUMUDPT.N_CTX / DEEP_PROMPT_DEPTH."""
    n, D, d, dv, e = cfg.n_ctx, cfg.depth, cfg.t_width, cfg.v_width, cfg.embed_dim
    return ([(CTX, (n, d)), (DEEP, (D - 1, n, d))] + generator_keys(GEN1, d, dv)
            + [(VCTX, (n, dv)), (VDEEP, (D - 1, n, dv))] + generator_keys(GEN2, dv, e))


def seeded_params(cfg: O.Config, seed: int, ctx: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The fixtures' values of the 40 tensors from ONE generator, drawn in key order by the rule of tests.umudpt_reference.seeded_params:
    LayerNorm gamma 1 + 0.1 N(0, 1), beta 0.05 N(0, 1), every other bias 0.02 N(0, 1), in_proj xavier-uniform, the Linears
    U(+-1/sqrt(fan_in)), the four prompt tables 0.02 N(0, 1).  ``ctx`` (the reference's CTX_INIT rows) replaces the drawn ctx."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shp in trainable_keys(cfg):
        r = torch.randn(shp, generator=g)
        if k in (CTX, DEEP, VCTX, VDEEP):
            v = 0.02 * r
        elif "ln_" in k:
            v = 1.0 + 0.1 * r if k.endswith("weight") else 0.05 * r
        elif k.endswith("bias"):
            v = 0.02 * r
        else:
            u = torch.rand(shp, generator=g) * 2 - 1
            v = u * (math.sqrt(6.0 / (shp[0] + shp[1])) if k.endswith("in_proj_weight") else 1.0 / math.sqrt(shp[1]))
        out[k] = v
    if ctx is not None:
        out[CTX] = ctx.clone()
    return out


_U_NAMES = (U.P + "ln_pre", U.P + "self_attn", U.P + "ln_post", U.P + "visual_proj")


def gen_params(params: Dict[str, torch.Tensor], names) -> Dict[str, torch.Tensor]:
    """One generator's 18 tensors under the keys tests.umudpt_reference.generator reads."""
    out = {}
    for mine, theirs in zip(names, _U_NAMES):
        for k, v in params.items():
            if k.startswith(mine + "."):
                out[theirs + k[len(mine):]] = v
    assert len(out) == 18, sorted(out)
    return out


def generator(params: Dict[str, torch.Tensor], names, X: torch.Tensor) -> torch.Tensor:
    """Gen1 (names = GEN1, X [D, n, d_t] -> [D, n, d_v]) or Gen2 (GEN2, X [D - 1, n, d_v] -> [D - 1, n, e]); zero layers give zero rows."""
    return U.generator(gen_params(params, names), X)


def generator_backward(params: Dict[str, torch.Tensor], names, X: torch.Tensor, dOut: torch.Tensor, dtype=torch.float64):
    """tests.umudpt_reference.generator_backward of one generator -> (output, dX, {this module's key: grad} of its 18 tensors)."""
    back = {theirs: mine for mine, theirs in zip(names, _U_NAMES)}
    out, dX, g = U.generator_backward(gen_params(params, names), X, dOut, dtype)

    def rename(k):
        for theirs, mine in back.items():
            if k.startswith(theirs + "."):
                return mine + k[len(theirs):]
        raise KeyError(k)
    return out, dX, {rename(k): v for k, v in g.items()}


def prompt_tables(params: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.cat([params[CTX].unsqueeze(0), params[DEEP]], dim=0)  # uumudpt.py:172


def forward(cfg, sd, params, class_embedding, eot, images, taps=None) -> torch.Tensor:
    """CustomCLIP.forward (uumudpt.py:219-233) -> logits [B, C].  taps["G"], taps["T"]: the generators' outputs (kept in the graph)."""
    G = generator(params, GEN1, prompt_tables(params))
    T = generator(params, GEN2, params[VDEEP])
    if taps is not None:
        taps["G"], taps["T"] = G, T
    vis = torch.cat([G[:1] + params[VCTX].unsqueeze(0), G[1:] + params[VDEEP]], dim=0)  # clip/model.py:638-643
    img = O.vision_tower(cfg, sd, images, vis[0], vis[1:], taps)
    txt = O.text_tower(cfg, sd, U.text_prompts(params[CTX], class_embedding), eot, params[DEEP] + T, taps)  # uumudpt.py:224
    return O.cosine_logits(sd, img, txt)


def forward_backward(cfg, sd, params, class_embedding, eot, images, labels):
    """F.cross_entropy (uumudpt.py:298-299) and the gradient of all 40 tensors -> (loss, logits, {key: grad}, dG, dT)."""
    taps = {}
    return O.loss_and_grads(lambda leaves: forward(cfg, sd, leaves, class_embedding, eot, images, taps), params, labels, taps=taps, keep=("G", "T"))


class UumudptCase(U.UmudptCase):
    """One tests/golden/uumudpt_*.npz fixture with its 40 tensors rebuilt from the seeded recipe (cfg.n_ctx / cfg.depth: TRAINER.UUMUDPT.N_CTX /
    DEEP_PROMPT_DEPTH; ctx_init: uumudpt.py:97-104)."""
    seeded_params, trainable_keys = staticmethod(seeded_params), staticmethod(trainable_keys)

    def __init__(self, name: str):
        super().__init__(name)
        self.sample_above = int(self.z["sample_above"])
        self.missing_keys = [str(v) for v in self.z["clip_missing_keys"]]  # what CLIP.load_state_dict reported for the frozen state dict
