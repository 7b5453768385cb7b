"""Test-local restatement of CLIP's ResNet image tower (clip/model.py:17-161, eval mode) in float64, batch-first NHWC, and the loader of the
rn_* fixtures.

``image_features`` folds every BatchNorm into the convolution in front of it (scale = gamma / sqrt(var + 1e-5); w' = w scale, b' = beta - mean
scale), runs the stem, the four stages of bottleneck blocks and the attention pool, and returns the raw features [B, embed_dim].  Without
``round_to`` nothing is rounded: tests/test_resnet_cpu.py holds that form to the features and logits the reference's own modules gave
(tests/golden/gen_golden_resnet.py).  With ``round_to`` = torch.float16 / torch.bfloat16 it rounds at exactly the sites the library rounds at
(mudpt_amd/csrc/resnet.hip's header):

  1. the folded convolution weights and the attention pool's Linear weights, to T (the folded bias to fp32);
  2. every GEMM operand activation, to T: the pixels, every post-ReLU tensor, the pooled tensors, the pooled tokens;
  3. the residual is read in T; the sum and the ReLU are exact here (fp32 there), then rounded once;
  4. q / k / v and the attention are exact here (fp32 there); the attention output is rounded to T for c_proj;
  5. the features are not rounded (fp32 there).

float64 stands for the library's fp32 accumulation, so ``emulated_rel`` -- that form against the reference's fp32 features, stored in every
fixture -- is the error of the number formats alone; the GPU test allows 3 x it.

``make_rn_state`` draws the tower's weights from a seed (the fixtures store seeds, not weights); the text side is ``oracle.mudpt_oracle``'s.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import FixtureCase

FIXTURES = ["rn_tiny", "rn_tiny2", "rn50_b2"]
BN_EPS = 1e-5


def conv_table(stages, width):
    """(conv prefix, bn prefix, cin, cout, k) of every convolution of the tower in module order: the stem, then per block conv1, conv2, conv3
    and, in the first block of a stage (stride > 1 or inplanes != 4 planes), downsample."""
    rows = [("visual.conv1", "visual.bn1", 3, width // 2, 3), ("visual.conv2", "visual.bn2", width // 2, width // 2, 3),
            ("visual.conv3", "visual.bn3", width // 2, width, 3)]
    inplanes = width
    for s, blocks in enumerate(stages):
        planes = width << s
        for i in range(blocks):
            p = f"visual.layer{s + 1}.{i}."
            rows += [(p + "conv1", p + "bn1", inplanes, planes, 1), (p + "conv2", p + "bn2", planes, planes, 3), (p + "conv3", p + "bn3", planes, 4 * planes, 1)]
            if i == 0:
                rows.append((p + "downsample.0", p + "downsample.1", inplanes, 4 * planes, 1))
            inplanes = 4 * planes
    return rows


def make_rn_state(shape, seed: int):
    """The "visual.*" tensors of a ResNet tower (``shape``: anything with v_stages, v_width, image_size, embed_dim) from plain
    torch.Generator draws, fp16-representable as checkpoints store them.  Convolutions N(0, 1 / fan_in): a convolution keeps the
    second moment of its input.  Measured in float64 on the three fixture shapes: N(0, 2 / fan_in) grows RN50's activations to 1e5, past fp16,
    and nn.Conv2d's default variance 1 / (3 fan_in) shrinks the image's share of the features below fp16's rounding error (two images then
    differ by 3e-5 to 5e-4 of |F|: no test of the tower); with 1 / fan_in two images differ by 3e-3 (RN50) to 1.3e-2 (tiny), 7 to 28 times
    ``emulated_rel``.  BatchNorm affine and running statistics away from (1, 0, 0, 1): gamma in [0.75, 1.25], beta and running_mean
    0.1 N(0, 1), running_var in [0.5, 1.5]; the attention pool N(0, 1 / C) with biases 0.02 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    r16 = lambda t: t.half().float()  # noqa: E731
    sd = {}
    for conv, bn, cin, cout, k in conv_table(shape.v_stages, shape.v_width):
        sd[conv + ".weight"] = r16(torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5)
        sd[bn + ".weight"] = r16(0.75 + 0.5 * torch.rand(cout, generator=g))
        sd[bn + ".bias"] = r16(0.1 * torch.randn(cout, generator=g))
        sd[bn + ".running_mean"] = r16(0.1 * torch.randn(cout, generator=g))
        sd[bn + ".running_var"] = r16(0.5 + torch.rand(cout, generator=g))
    C = 32 * shape.v_width
    sd["visual.attnpool.positional_embedding"] = r16(torch.randn((shape.image_size // 32) ** 2 + 1, C, generator=g) * C ** -0.5)
    for n, out in (("k_proj", C), ("q_proj", C), ("v_proj", C), ("c_proj", shape.embed_dim)):
        sd[f"visual.attnpool.{n}.weight"] = r16(torch.randn(out, C, generator=g) * C ** -0.5)
        sd[f"visual.attnpool.{n}.bias"] = r16(0.02 * torch.randn(out, generator=g))
    return sd


def fold(sd, conv, bn):
    """float64 (w', b') of a convolution with the eval-mode BatchNorm behind it folded in."""
    scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + BN_EPS)
    return sd[conv + ".weight"].double() * scale[:, None, None, None], sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale


def image_features(sd, images, stages, heads, round_to=None):
    """Raw features [B, embed_dim] (float64) of images [B, 3, S, S].  Activations are [B, H, W, C]."""
    q = (lambda t: t.to(round_to).double()) if round_to is not None else (lambda t: t)
    qb = (lambda t: t.float().double()) if round_to is not None else (lambda t: t)
    width = sd["visual.layer1.0.conv1.weight"].shape[0]

    def conv(x, cname, bname, stride=1, residual=None, relu=True):
        w, b = fold(sd, cname, bname)
        y = F.conv2d(x.permute(0, 3, 1, 2), q(w), None, stride, w.shape[-1] // 2).permute(0, 2, 3, 1) + qb(b)
        if residual is not None:
            y = y + residual
        return q(torch.relu(y) if relu else y)

    def pool(x, k):
        B, H, W, C = x.shape
        return q(x[:, :H // k * k, :W // k * k].reshape(B, H // k, k, W // k, k, C).mean(dim=(2, 4)))

    x = q(images.double().permute(0, 2, 3, 1))
    x = conv(x, "visual.conv1", "visual.bn1", stride=2)
    x = conv(x, "visual.conv2", "visual.bn2")
    x = conv(x, "visual.conv3", "visual.bn3")
    x = pool(x, 2)
    for s, blocks in enumerate(stages):
        for i in range(blocks):
            p, stride = f"visual.layer{s + 1}.{i}.", 2 if (s > 0 and i == 0) else 1
            y = conv(x, p + "conv1", p + "bn1")
            y = conv(y, p + "conv2", p + "bn2")
            if stride > 1:
                y = pool(y, stride)
            identity = x
            if p + "downsample.0.weight" in sd:
                identity = conv(pool(x, stride) if stride > 1 else x, p + "downsample.0", p + "downsample.1", relu=False)
            x = conv(y, p + "conv3", p + "bn3", residual=identity)
    B, H, W, C = x.shape
    assert C == 32 * width and C == heads * 64
    t = x.reshape(B, H * W, C)
    t = q(torch.cat([t.mean(dim=1, keepdim=True), t], dim=1) + sd["visual.attnpool.positional_embedding"].double())
    lin = lambda v, n: v @ q(sd[f"visual.attnpool.{n}.weight"].double()).t() + sd[f"visual.attnpool.{n}.bias"].double()  # noqa: E731
    qh = (lin(t[:, :1], "q_proj") * 64 ** -0.5).reshape(B, 1, heads, 64).transpose(1, 2)
    kh, vh = (lin(t, n).reshape(B, H * W + 1, heads, 64).transpose(1, 2) for n in ("k_proj", "v_proj"))
    a = torch.softmax(qh @ kh.transpose(-1, -2), dim=-1) @ vh
    return lin(q(a.transpose(1, 2).reshape(B, C)), "c_proj")


def feature_error(got, ref):
    """max over images of |F - ref| / |ref|, the metric of tests/test_zsclip_gpu.py."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


class RnShape:
    """What the generator knows of a tower before any state dict exists."""

    def __init__(self, stages, width, image_size, embed_dim):
        self.v_stages, self.v_width, self.image_size, self.embed_dim = tuple(int(v) for v in stages), int(width), int(image_size), int(embed_dim)


class RnCase(FixtureCase):
    """One tests/golden/rn_*.npz fixture.  ``cfg`` (oracle.mudpt_oracle.Config) describes the text side; its ViT fields only seed the draws
    of ``frozen`` and are not a tower of this case.  ``state`` is the CLIP state dict the case runs on: the text side of ``frozen`` and the
    ResNet tower of ``make_rn_state`` (seeds: frozen, tower, images)."""

    def __init__(self, name: str):
        super().__init__(name)
        z = self.z
        self.trainer, self.dataset = str(z["trainer"]), str(z["dataset"])
        self.templates = [str(v) for v in z["templates"]]
        self.tokens = torch.from_numpy(z["tokens"])  # int32 [T, C, ctx_len]
        self.text_features = torch.from_numpy(z["text_features"])
        self.image_features = torch.from_numpy(z["image_features"])
        self.stages, self.width = tuple(int(v) for v in z["rn_stages"]), int(z["rn_width"])
        self.heads = self.width * 32 // 64
        self.emulated_rel = {"fp16": float(z["emulated_rel"][0]), "bf16": float(z["emulated_rel"][1])}
        self.emulated_logit = {"fp16": tuple(float(v) for v in z["emulated_logit"][:2]), "bf16": tuple(float(v) for v in z["emulated_logit"][2:])}  # (max, rms)
        self.rn = make_rn_state(RnShape(self.stages, self.width, self.cfg.image_size, self.cfg.embed_dim), self.seeds[1])
        self.state = {k: v for k, v in self.frozen.items() if not k.startswith("visual.")}
        self.state.update(self.rn)

    def shape(self):
        from mudpt_amd.model import ModelShape
        return ModelShape.from_state_dict(self.state, 0, 1)


_CASES = {}


def case(name: str) -> RnCase:
    """The fixture, loaded once per process and shared (its tensors are not to be written)."""
    if name not in _CASES:
        _CASES[name] = RnCase(name)
    return _CASES[name]


def emulated_rel(sd, images, stages, heads, ref):
    """[fp16, bf16]: the float64 restatement with T-rounding at the five sites against the reference's features."""
    return np.array([feature_error(image_features(sd, images, stages, heads, T), ref) for T in (torch.float16, torch.bfloat16)])
