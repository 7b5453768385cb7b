"""Synthetic stand-ins for what needs the network in the reference: a random-initialised CLIP state dict
(no ViT-B-16.pt offline; clip/clip.py:31-41 are download URLs) and class prompts without the BPE vocabulary.

Used by bench.py and the Dassl-free harness only; real runs pass a checkpoint's state dict instead."""
from __future__ import annotations

import math
from typing import Dict

import torch

from .model import ModelShape

# first Caltech-101 class names (datasets/caltech101.py:8-14 renaming applied), the benchmark's 11 classes
BENCH_CLASSNAMES = ["face", "leopard", "motorbike", "accordion", "airplane", "anchor", "ant", "barrel", "bass", "beaver",
                    "binocular"]
# clip.tokenize("a photo of a <name>.") for the names above (clip/clip.py:199-239): SOT 49406, "a photo of a"
# = 320 1125 539 320, name, "." = 269, EOT 49407.  Values recorded from the reference tokenizer (tests/golden).
_BENCH_NAME_TOKENS = [[1710], [15931], [33341], [48760], [16451], [13201], [773], [11703], [5992], [22874], [29172, 10940]]
CTX_INIT_TOKENS = [320, 1125, 539, 320]  # "a photo of a"
VOCAB = 49408


def bench_tokenized_prompts(ctx_len: int = 77) -> torch.Tensor:
    tok = torch.zeros(len(_BENCH_NAME_TOKENS), ctx_len, dtype=torch.int32)
    for i, name in enumerate(_BENCH_NAME_TOKENS):
        ids = [49406] + CTX_INIT_TOKENS + name + [269, 49407]
        tok[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return tok


X_TOKEN = 343  # "X", the placeholder context word of CoOp's prompts (trainers/coop.py:72); recorded in tests/golden/coop_*.npz


def bench_coop_prompts(n_ctx: int, ctx_len: int = 77):
    """clip.tokenize("X X .. X <name>.") for the benchmark names (trainers/coop.py:72,82-84) and len(_tokenizer.encode(name)) (:80), without
    the BPE vocabulary: the CoOp plugin's stand-in on synthetic data."""
    tok = torch.zeros(len(_BENCH_NAME_TOKENS), ctx_len, dtype=torch.int32)
    for i, name in enumerate(_BENCH_NAME_TOKENS):
        ids = [49406] + [X_TOKEN] * n_ctx + name + [269, 49407]
        tok[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return tok, [len(n) for n in _BENCH_NAME_TOKENS]


def synthetic_tokenized_prompts(n_cls: int, n_ctx: int = 4, ctx_len: int = 77, seed: int = 7) -> torch.Tensor:
    """Prompts shaped like "<ctx words> <name tokens> ." for synthetic class lists (e.g. 1000 ImageNet-sized).  Name lengths
    follow a long-tailed mix like BPE-tokenised ImageNet names: 70 % 1-3 tokens, 25 % 4-6, 5 % 7-12 (the longest name sets
    the number of positions the causal text tower has to run, see mudpt_set_class_prompts)."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.zeros(n_cls, ctx_len, dtype=torch.int32)
    for c in range(n_cls):
        u = float(torch.rand((), generator=g))
        lo, hi = (1, 3) if u < 0.70 else ((4, 6) if u < 0.95 else (7, 12))
        k = lo + int(torch.randint(0, hi - lo + 1, (1,), generator=g))
        ids = [49406] + (CTX_INIT_TOKENS * n_ctx)[:n_ctx] + [int(v) for v in torch.randint(1000, 48000, (k,), generator=g)] + [269, 49407]
        tok[c, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return tok


# the ResNet backbones of clip.load (clip/clip.py:32-36) the library runs -- frozen (zsclip.FrozenCLIP) and under CoOp / CoCoOp (model.CustomCLIP) --
# as ModelShape(**RESNET_SHAPES[name]); RN50x4 (width 80) is not built
RESNET_SHAPES = {
    "RN50": dict(image_size=224, patch=32, v_width=64, v_layers=16, v_heads=32, v_stages=(3, 4, 6, 3), embed_dim=1024),
    "RN101": dict(image_size=224, patch=32, v_width=64, v_layers=33, v_heads=32, v_stages=(3, 4, 23, 3), embed_dim=512),
    "RN50x16": dict(image_size=384, patch=32, v_width=96, v_layers=40, v_heads=48, v_stages=(6, 8, 18, 8), embed_dim=768, t_width=768, t_heads=12),
    "RN50x64": dict(image_size=448, patch=32, v_width=128, v_layers=64, v_heads=64, v_stages=(3, 15, 36, 10), embed_dim=1024, t_width=1024, t_heads=16),
}


def resnet_state_table(shape: ModelShape):
    """(key, tensor shape, init) of the "visual.*" entries of a CLIP ResNet state dict (clip/model.py:17-161) in the reference's module order.
    Convolutions are N(0, 1 / fan_in): activations stay O(1) to O(10) through all stages (2 / fan_in reaches 1e5 at RN50, past fp16); BatchNorm is the identity it is before training
    (weight and running_var ones, bias and running_mean zeros); the attention pool as clip/model.py:786-791."""
    w, C = shape.v_width, 32 * shape.v_width
    rows = []

    def conv_bn(conv, bn, cin, cout, k):
        rows.append((conv + ".weight", (cout, cin, k, k), (cin * k * k) ** -0.5))
        rows.extend([(bn + ".weight", (cout,), "ones"), (bn + ".bias", (cout,), "zeros"), (bn + ".running_mean", (cout,), "zeros"),
                     (bn + ".running_var", (cout,), "ones")])
    conv_bn("visual.conv1", "visual.bn1", 3, w // 2, 3)
    conv_bn("visual.conv2", "visual.bn2", w // 2, w // 2, 3)
    conv_bn("visual.conv3", "visual.bn3", w // 2, w, 3)
    inplanes = w
    for s, blocks in enumerate(shape.v_stages):
        planes = w << s
        for i in range(blocks):
            p = f"visual.layer{s + 1}.{i}."
            conv_bn(p + "conv1", p + "bn1", inplanes, planes, 1)
            conv_bn(p + "conv2", p + "bn2", planes, planes, 3)
            conv_bn(p + "conv3", p + "bn3", planes, 4 * planes, 1)
            if i == 0:  # stride > 1 or inplanes != 4 planes (clip/model.py:41): the first block of every stage
                conv_bn(p + "downsample.0", p + "downsample.1", inplanes, 4 * planes, 1)
            inplanes = 4 * planes
    rows.append(("visual.attnpool.positional_embedding", ((shape.image_size // 32) ** 2 + 1, C), C ** -0.5))
    for n, out in (("k_proj", C), ("q_proj", C), ("v_proj", C), ("c_proj", shape.embed_dim)):
        rows += [(f"visual.attnpool.{n}.weight", (out, C), C ** -0.5), (f"visual.attnpool.{n}.bias", (out,), 0.02)]
    return rows


def clip_state_table(shape: ModelShape):
    """(key, tensor shape, init) of every entry of a CLIP state dict (clip/model.py:667-808), ViT or -- ``shape.resnet`` -- ResNet image
    tower: init is a std for N(0, std^2) entries, "ones" / "zeros" for LayerNorm / BatchNorm terms and attention biases."""
    dv, dt, e = shape.v_width, shape.t_width, shape.embed_dim
    P = (shape.image_size // shape.patch) ** 2
    rows = resnet_state_table(shape) if shape.resnet else [
        ("visual.conv1.weight", (dv, 3, shape.patch, shape.patch), (3 * shape.patch ** 2) ** -0.5),
        ("visual.class_embedding", (dv,), dv ** -0.5),
        ("visual.positional_embedding", (P + 1, dv), dv ** -0.5),
        ("visual.ln_pre.weight", (dv,), "ones"), ("visual.ln_pre.bias", (dv,), "zeros"),
        ("visual.ln_post.weight", (dv,), "ones"), ("visual.ln_post.bias", (dv,), "zeros"),
        ("visual.proj", (dv, e), dv ** -0.5),
    ]
    rows += [
        ("token_embedding.weight", (VOCAB, dt), 0.02),
        ("positional_embedding", (shape.ctx_len, dt), 0.01),
        ("ln_final.weight", (dt,), "ones"), ("ln_final.bias", (dt,), "zeros"),
        ("text_projection", (dt, e), dt ** -0.5),
    ]
    for prefix, d, layers in (("visual.transformer", dv, 0 if shape.resnet else shape.v_layers), ("transformer", dt, shape.t_layers)):
        for i in range(layers):
            p = f"{prefix}.resblocks.{i}."
            rows += [(p + "ln_1.weight", (d,), "ones"), (p + "ln_1.bias", (d,), "zeros"),
                     (p + "ln_2.weight", (d,), "ones"), (p + "ln_2.bias", (d,), "zeros"),
                     (p + "attn.in_proj_weight", (3 * d, d), d ** -0.5), (p + "attn.in_proj_bias", (3 * d,), "zeros"),
                     (p + "attn.out_proj.weight", (d, d), d ** -0.5 * (2 * layers) ** -0.5), (p + "attn.out_proj.bias", (d,), "zeros"),
                     (p + "mlp.c_fc.weight", (4 * d, d), (2 * d) ** -0.5), (p + "mlp.c_fc.bias", (4 * d,), 0.02),
                     (p + "mlp.c_proj.weight", (d, 4 * d), d ** -0.5 * (2 * layers) ** -0.5), (p + "mlp.c_proj.bias", (d,), 0.02)]
    return rows


def random_clip_state_shapes(shape: ModelShape) -> Dict[str, torch.Tensor]:
    """Uninitialised tensors of a CLIP state dict's shapes (under ``torch.device("meta")``: shapes only), for shape inference."""
    sd = {k: torch.empty(s) for k, s, _ in clip_state_table(shape)}
    sd["logit_scale"] = torch.empty(())
    return sd


def random_clip_state(shape: ModelShape, seed: int = 0, fp16_weights: bool = True) -> Dict[str, torch.Tensor]:
    """Random CLIP weights with the distributions of CLIP.initialize_parameters (clip/model.py:781-808) and the
    vision tower's width^-1/2 scale (clip/model.py:506-508,524); random, not zeros (zeros inflate clocks)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s, init in clip_state_table(shape):
        if init == "ones":
            sd[k] = torch.ones(s)
        elif init == "zeros":
            sd[k] = torch.zeros(s)
        else:
            t = torch.randn(*s, generator=g) * init
            sd[k] = t.half().float() if fp16_weights else t
    sd["logit_scale"] = torch.tensor(math.log(1 / 0.07))
    return sd


def synthetic_uint8_images(n: int, n_classes: int, seed: int = 0, lo: int = 32, hi: int = 64):
    """n seeded HWC uint8 "photographs" with heights and widths drawn from [lo, hi] and uniform labels: what a decoded few-shot training set
    looks like to DeviceImageStore.from_arrays (mudpt_amd/augment.py), without files.  Smooth colour ramps under noise, so that a resample
    has structure to get wrong."""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(lo, hi + 1, (n, 2), generator=g)
    labels = torch.randint(0, n_classes, (n,), generator=g)
    images = []
    for h, w in sizes.tolist():
        ramp = torch.arange(h)[:, None, None] * torch.tensor([3, 1, 2]) + torch.arange(w)[None, :, None] * torch.tensor([1, 2, 3])
        images.append(((ramp + torch.randint(0, 64, (h, w, 3), generator=g)) % 256).to(torch.uint8))
    return images, labels
