"""Test-local restatement of the UMuDPT path (trainers/umudpt.py:79-230) in plain torch CPU, and the loader of the umudpt_* fixtures.

The towers are MuDPT's (``ResidualAttentionBlock_UMuDPT``, clip/model.py:304-351, is ``ResidualAttentionBlock_MuDPT`` line for line), so the
blocks are the unchanged ``oracle.mudpt_oracle.block``; only the front end that makes the prompt tables differs
(``UMuDPTPromptLearner.forward``, umudpt.py:161-178): X = cat(ctx[None], deep_prompts) [depth, n_ctx, d_t] goes through ln_pre, ONE pre-LN
transformer block whose attention runs over the n_ctx rows of one layer (the permute(1, 0, 2) makes the layers the batch), ln_post and
visual_proj; G[0] are the vision tower's input prompt rows, G[1:] its deep prompts (``VisionTransformer_UMuDPT``, clip/model.py:556-597),
and the text tower takes ctx / deep_prompts as they are.  :func:`generator` works in the dtype of its operands (the kernel tests call it in
float64).  Pinned by the fixtures of tests/golden/gen_golden_umudpt.py, which ran the reference's own modules (tests/test_umudpt_cpu.py).
"""
from __future__ import annotations

import ast
import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mudpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
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


def vision_tower(cfg: O.Config, sd, G: torch.Tensor, images, taps: Optional[Dict] = None) -> torch.Tensor:
    """VisionTransformer_UMuDPT.forward (clip/model.py:574-597): G[0] appended after the positional embedding, blocks 1 <= i replace the
    last n_ctx rows by G[i] while i < depth -> image features [B, e]."""
    B, n = images.shape[0], cfg.n_ctx
    w = sd["visual.conv1.weight"].reshape(cfg.v_width, -1)
    x = O.patchify(images.float(), cfg.patch) @ w.t()
    x = torch.cat([sd["visual.class_embedding"].expand(B, 1, -1), x], dim=1) + sd["visual.positional_embedding"]
    x = torch.cat([x, G[0].unsqueeze(0).expand(B, -1, -1)], dim=1)
    x = O.layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
    L = x.shape[1]
    for i in range(cfg.v_layers):
        if 1 <= i < G.shape[0]:
            x = torch.cat([x[:, :L - n], G[i].unsqueeze(0).expand(B, -1, -1)], dim=1)
        if taps is not None:
            taps[f"vis.x_in.{i}"] = x
        x = O.block(x, sd, f"visual.transformer.resblocks.{i}.", cfg.v_heads, None)
    return O.layer_norm(x[:, 0], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"]


def text_tower(cfg: O.Config, sd, params, class_embedding, eot, taps: Optional[Dict] = None) -> torch.Tensor:
    """construct_prompts + TextEncoder.forward (umudpt.py:141-168,190-204): ctx at rows 1..n_ctx, blocks 1 <= i < depth replace them by
    deep_prompts[i - 1] -> text features [C, e]."""
    n, C = cfg.n_ctx, class_embedding.shape[0]
    prompts = torch.cat([class_embedding[:, :1], params[CTX].unsqueeze(0).expand(C, -1, -1), class_embedding[:, 1 + n:]], dim=1)
    x = prompts + sd["positional_embedding"]
    mask = O.causal_mask(x.shape[1])
    deep = params[DEEP]
    for i in range(cfg.t_layers):
        if i >= 1 and i - 1 < deep.shape[0]:
            x = torch.cat([x[:, :1], deep[i - 1].unsqueeze(0).expand(C, -1, -1), x[:, 1 + n:]], dim=1)
        if taps is not None:
            taps[f"txt.x_in.{i}"] = x
        x = O.block(x, sd, f"transformer.resblocks.{i}.", cfg.t_heads, mask)
    x = O.layer_norm(x, sd["ln_final.weight"], sd["ln_final.bias"])
    return x[torch.arange(C), eot] @ sd["text_projection"]


def forward(cfg, sd, params, class_embedding, eot, images, taps=None) -> torch.Tensor:
    """CustomCLIP.forward (umudpt.py:217-230) -> logits [B, C].  taps["G"]: the generator's output (kept in the graph)."""
    G = generator(params, prompt_tables(params))
    if taps is not None:
        taps["G"] = G
    img = vision_tower(cfg, sd, G, images, taps)
    txt = text_tower(cfg, sd, params, class_embedding, eot, taps)
    img = img / img.norm(dim=-1, keepdim=True)
    txt = txt / txt.norm(dim=-1, keepdim=True)
    return sd["logit_scale"].exp() * img @ txt.t()


def forward_backward(cfg, sd, params, class_embedding, eot, images, labels):
    """F.cross_entropy (umudpt.py:292-294) and the gradient of all 20 tensors -> (loss, logits, {key: grad}, dG)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    taps = {}
    logits = forward(cfg, sd, leaves, class_embedding, eot, images, taps)
    taps["G"].retain_grad()
    loss = F.cross_entropy(logits, labels.long())
    loss.backward()
    grads = {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return loss.detach(), logits.detach(), grads, taps["G"].grad.detach()


def sample_rows(key: str, rows: int, seed: int) -> List[int]:
    """The SAMPLE_ROWS rows of a sampled gradient: a seeded draw per tensor, sorted."""
    g = torch.Generator().manual_seed(seed * 1000003 + sum(key.encode()))
    return sorted(int(v) for v in torch.randperm(rows, generator=g)[:SAMPLE_ROWS])


class UmudptCase:
    """One tests/golden/umudpt_*.npz fixture with its frozen weights and its 20 tensors rebuilt from the seeded recipe."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.name, self.z = name, z
        self.cfg = O.Config(**ast.literal_eval(str(z["config"])))  # n_ctx / depth: TRAINER.UMUDPT.N_CTX / DEEP_PROMPT_DEPTH
        fs, ts, is_ = (int(v) for v in z["seeds"])
        self.seeds = (fs, ts, is_)
        self.frozen = O.make_frozen_state(self.cfg, fs)
        self.frozen["logit_scale"] = torch.tensor(float(z["logit_scale"]))
        self.classnames = [str(v) for v in z["classnames"]]
        self.tokens = torch.from_numpy(z["tokenized_prompts"]).long()
        self.eot = self.tokens.argmax(dim=-1)
        self.class_embedding = self.frozen["token_embedding.weight"][self.tokens]
        self.ctx_token_ids = [int(v) for v in z["ctx_token_ids"]]
        self.ctx_init = self.frozen["token_embedding.weight"][self.ctx_token_ids]  # the reference's CTX_INIT rows (umudpt.py:96-103)
        self.params = seeded_params(self.cfg, ts, self.ctx_init)
        self.keys = [k for k, _ in trainable_keys(self.cfg)]
        self.labels = torch.from_numpy(z["labels"])
        g = torch.Generator().manual_seed(is_)
        self.images = torch.randn(len(self.labels), 3, self.cfg.image_size, self.cfg.image_size, generator=g)
        self.logits = torch.from_numpy(z["logits"])
        self.loss = float(z["loss"])
        # full gradients, or (rows, values [16, cols], rms of the whole tensor) for the sampled ones
        self.grads = {k: torch.from_numpy(z["grad." + k]) for k in self.keys if "grad." + k in z.files}
        self.grad_samples = {k: ([int(r) for r in z["grad_rows." + k + ".idx"]], torch.from_numpy(z["grad_rows." + k]), float(z["grad_rms." + k]))
                             for k in self.keys if "grad_rows." + k in z.files}
        self.init_checksums = {k: [float(v) for v in z["init_checksum." + k]] for k in self.keys}
        self.taps = {k[4:]: (torch.from_numpy(z[k]), [int(r) for r in z[k + ".rows"]]) for k in z.files if k.startswith("tap.") and not k.endswith(".rows")}
