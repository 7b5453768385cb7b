"""Test-local restatement of the UMuDPT path (trainers/umudpt.py:79-230) in plain torch CPU, and the loader of the umudpt_* fixtures.

The towers are MuDPT's (``ResidualAttentionBlock_UMuDPT``, clip/model.py:304-351, is ``ResidualAttentionBlock_MuDPT`` line for line), so the
towers are ``oracle.mudpt_oracle``'s; only the front end that makes the prompt tables differs
(``UMuDPTPromptLearner.forward``, umudpt.py:161-178): X = cat(ctx[None], deep_prompts) [depth, n_ctx, d_t] goes through ln_pre, ONE pre-LN
transformer block whose attention runs over the n_ctx rows of one layer (the permute(1, 0, 2) makes the layers the batch), ln_post and
visual_proj; G[0] are the vision tower's input prompt rows, G[1:] its deep prompts (``VisionTransformer_UMuDPT``, clip/model.py:556-597),
and the text tower takes ctx / deep_prompts as they are.  :func:`generator` works in the dtype of its operands (the kernel tests call it in
float64).  Pinned by the fixtures of tests/golden/gen_golden_umudpt.py, which ran the reference's own modules (tests/test_umudpt_cpu.py).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import mudpt_oracle as O
from tests.helpers import GOLDEN, FixtureCase  # noqa: F401

FIXTURES = ["umudpt_tiny", "umudpt_tiny_d1", "umudpt_tiny_d5", "umudpt_vitb16_b2", "umudpt_vitb16_b2_s100"]
P = "umudpt_prompt_learner."
CTX, DEEP = P + "ctx", P + "deep_prompts"
SAMPLE_ABOVE, SAMPLE_ROWS = 65536, 16  # a ViT-B gradient above SAMPLE_ABOVE elements is stored as SAMPLE_ROWS seeded rows plus its rms


def trainable_keys(cfg: O.Config) -> List[Tuple[str, Tuple[int, ...]]]:
    """The reference's 20 trainables -- every parameter whose name contains "prompt_learner" (umudpt.py:252-255) -- in named_parameters()
    order, with their shapes.  cfg.n_ctx / cfg.depth are TRAINER.UMUDPT.N_CTX / DEEP_PROMPT_DEPTH."""
    n, D, d, dv = cfg.n_ctx, cfg.depth, cfg.t_width, cfg.v_width
    shapes = [("ctx", (n, d)), ("deep_prompts", (D - 1, n, d)), ("ln_pre.weight", (d,)), ("ln_pre.bias", (d,)),
              ("self_attn.attn.in_proj_weight", (3 * d, d)), ("self_attn.attn.in_proj_bias", (3 * d,)),
              ("self_attn.attn.out_proj.weight", (d, d)), ("self_attn.attn.out_proj.bias", (d,)),
              ("self_attn.ln_1.weight", (d,)), ("self_attn.ln_1.bias", (d,)),
              ("self_attn.mlp.c_fc.weight", (4 * d, d)), ("self_attn.mlp.c_fc.bias", (4 * d,)),
              ("self_attn.mlp.c_proj.weight", (d, 4 * d)), ("self_attn.mlp.c_proj.bias", (d,)),
              ("self_attn.ln_2.weight", (d,)), ("self_attn.ln_2.bias", (d,)), ("ln_post.weight", (d,)), ("ln_post.bias", (d,)),
              ("visual_proj.weight", (dv, d)), ("visual_proj.bias", (dv,))]
    return [(P + k, s) for k, s in shapes]


def seeded_params(cfg: O.Config, seed: int, ctx: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The fixtures' values of the 20 tensors from ONE generator, drawn in key order, non-degenerate on purpose: every LayerNorm gamma is
    1 + 0.1 N(0, 1), every beta 0.05 N(0, 1) and every bias 0.02 N(0, 1) (the module defaults 1 / 0 would hide a wrong dgamma or dbeta);
    weights at their init scale -- in_proj xavier-uniform (nn.MultiheadAttention), the Linears U(+-1/sqrt(fan_in)) -- and the prompts
    0.02 N(0, 1).  ``ctx`` (the reference's CTX_INIT rows) replaces the drawn ctx."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shp in trainable_keys(cfg):
        r = torch.randn(shp, generator=g)
        if k in (CTX, DEEP):
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


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def generator(params: Dict[str, torch.Tensor], X: torch.Tensor) -> torch.Tensor:
    """G [depth, n_ctx, d_v] = visual_proj(ln_post(Block(ln_pre(X)))) for X [depth, n_ctx, d_t] (umudpt.py:170-176, LightTransformer :56-76):
    d_t / 64 heads, no mask, nn.MultiheadAttention scaling, sequences = the layers.  Runs in the dtype of its operands."""
    p = lambda k: params[P + k]  # noqa: E731
    S = "self_attn."
    d = X.shape[-1]
    x = _ln(X, p("ln_pre.weight"), p("ln_pre.bias"))
    h = _ln(x, p(S + "ln_1.weight"), p(S + "ln_1.bias"))
    qkv = h @ p(S + "attn.in_proj_weight").t() + p(S + "attn.in_proj_bias")
    x = x + O.attention(qkv, d // 64, None) @ p(S + "attn.out_proj.weight").t() + p(S + "attn.out_proj.bias")
    h = _ln(x, p(S + "ln_2.weight"), p(S + "ln_2.bias"))
    u = h @ p(S + "mlp.c_fc.weight").t() + p(S + "mlp.c_fc.bias")
    x = x + (u * torch.sigmoid(1.702 * u)) @ p(S + "mlp.c_proj.weight").t() + p(S + "mlp.c_proj.bias")
    return _ln(x, p("ln_post.weight"), p("ln_post.bias")) @ p("visual_proj.weight").t() + p("visual_proj.bias")


def generator_backward(params: Dict[str, torch.Tensor], X: torch.Tensor, dG: torch.Tensor, dtype=torch.float64):
    """Autograd of :func:`generator` in ``dtype`` -> (G, dX, {key: grad} of the 18 generator tensors)."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items() if k not in (CTX, DEEP)}
    Xl = X.detach().to(dtype).clone().requires_grad_(True)
    G = generator(leaves, Xl)
    G.backward(dG.to(dtype))
    return G.detach(), Xl.grad.detach(), {k: v.grad.detach() for k, v in leaves.items()}


def prompt_tables(params: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.cat([params[CTX].unsqueeze(0), params[DEEP]], dim=0)  # umudpt.py:170


def text_prompts(ctx: torch.Tensor, class_embedding: torch.Tensor) -> torch.Tensor:
    """construct_prompts (umudpt.py:141-168): ctx at rows 1..n_ctx of every class prompt."""
    C = class_embedding.shape[0]
    return torch.cat([class_embedding[:, :1], ctx.unsqueeze(0).expand(C, -1, -1), class_embedding[:, 1 + ctx.shape[0]:]], dim=1)


def forward(cfg, sd, params, class_embedding, eot, images, taps=None) -> torch.Tensor:
    """CustomCLIP.forward (umudpt.py:217-230) -> logits [B, C]: G[0] are the vision tower's input rows and G[1:] its deep rows
    (clip/model.py:574-597), the text tower takes ctx and deep_prompts as they are (umudpt.py:190-204).  taps["G"]: the generator's output
    (kept in the graph)."""
    G = generator(params, prompt_tables(params))
    if taps is not None:
        taps["G"] = G
    img = O.vision_tower(cfg, sd, images, G[0], G[1:], taps)
    txt = O.text_tower(cfg, sd, text_prompts(params[CTX], class_embedding), eot, params[DEEP], taps)
    return O.cosine_logits(sd, img, txt)


def forward_backward(cfg, sd, params, class_embedding, eot, images, labels):
    """F.cross_entropy (umudpt.py:292-294) and the gradient of all 20 tensors -> (loss, logits, {key: grad}, dG)."""
    taps = {}
    return O.loss_and_grads(lambda leaves: forward(cfg, sd, leaves, class_embedding, eot, images, taps), params, labels, taps=taps, keep=("G",))


def sample_rows(key: str, rows: int, seed: int) -> List[int]:
    """The SAMPLE_ROWS rows of a sampled gradient: a seeded draw per tensor, sorted."""
    g = torch.Generator().manual_seed(seed * 1000003 + sum(key.encode()))
    return sorted(int(v) for v in torch.randperm(rows, generator=g)[:SAMPLE_ROWS])


class UmudptCase(FixtureCase):
    """One tests/golden/umudpt_*.npz fixture with its 20 tensors rebuilt from the seeded recipe (cfg.n_ctx / cfg.depth: TRAINER.UMUDPT.N_CTX /
    DEEP_PROMPT_DEPTH).  tests.uumudpt_reference's loader swaps in its own two recipe functions."""
    seeded_params, trainable_keys = staticmethod(seeded_params), staticmethod(trainable_keys)

    def __init__(self, name: str):
        super().__init__(name)
        self.ctx_init = self.frozen["token_embedding.weight"][self.ctx_token_ids]  # the reference's CTX_INIT rows (umudpt.py:96-103)
        self.params = self.seeded_params(self.cfg, self.seeds[1], self.ctx_init)
        self.keys = [k for k, _ in self.trainable_keys(self.cfg)]
        self.load_grads()
        self.init_checksums = {k: [float(v) for v in self.z["init_checksum." + k]] for k in self.keys}
