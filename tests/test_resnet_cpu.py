"""No-GPU checks of the ResNet image tower (mudpt_create_frozen_resnet): the float64 restatement the GPU tests compare against is the
reference's tower; the shape inference, the host-side BatchNorm folding and the create-time refusals."""
import ctypes as C
import os

import pytest
import torch

from mudpt_amd import build, capi, synth
from mudpt_amd.model import ModelShape
from oracle import mudpt_oracle as O
from tests import resnet_reference as R
from tests import zsclip_reference as ZR
from tests.helpers import LOGIT_ATOL, LOGIT_RMS, TINY_SLACK


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_float64_restatement_is_the_reference(name):
    """tests/resnet_reference.image_features without rounding against what the reference's own ModifiedResNet / ZeroshotCLIP gave: the logits
    within test_oracle_golden.py's bound for the same comparison, the raw features to 1e-5 of their norm (the reference ran in fp32)."""
    case = R.case(name)
    with torch.no_grad():
        feat = R.image_features(case.rn, case.images, case.stages, case.heads)
        txt = ZR.text_features(case.cfg, case.frozen, case.tokens)
    assert tuple(feat.shape) == tuple(case.image_features.shape)
    err = R.feature_error(feat, case.image_features)
    print(f"{name}: |F - reference| / |reference| = {err:.2e}")
    assert err <= 1e-5
    torch.testing.assert_close(txt, case.text_features, atol=2e-5, rtol=1e-5)
    logits = case.frozen["logit_scale"].exp() * O.unit(feat.float()) @ txt.t()
    torch.testing.assert_close(logits, case.logits, atol=2e-5, rtol=1e-5)
    # the fixture is a test of the tower: two images differ by far more than the bound the GPU test allows (3 x emulated_rel)
    assert R.feature_error(case.image_features[:1], case.image_features[1:2]) >= 2 * 3 * case.emulated_rel["fp16"]
    assert 0 < case.emulated_rel["fp16"] < case.emulated_rel["bf16"] < 1e-2
    # ... and one a correct implementation can pass: what the number formats alone cost at the logits is at most half of check_logits' bounds
    slack = TINY_SLACK if case.cfg.v_layers < 12 else 1.0
    for dtype, (worst, rms) in case.emulated_logit.items():
        assert worst <= 0.5 * slack * LOGIT_ATOL[dtype] and rms <= 0.5 * slack * LOGIT_RMS[dtype], (name, dtype, worst, rms)


def test_shape_inference():
    """ModelShape.from_state_dict takes build_model's ResNet branch (clip/model.py:890-897) without "visual.proj" and leaves the ViT branch alone."""
    for name, stages, width, size, embed in (("rn_tiny", (1, 1, 1, 1), 32, 64, 512), ("rn_tiny2", (2, 1, 2, 1), 64, 96, 1024), ("rn50_b2", (3, 4, 6, 3), 64, 224, 1024)):
        s = R.case(name).shape()
        assert s.resnet and (s.v_stages, s.v_width, s.image_size, s.embed_dim, s.v_heads) == (stages, width, size, embed, width * 32 // 64)
        assert (s.t_width, s.t_layers, s.t_heads, s.ctx_len) == (R.case(name).cfg.t_width, R.case(name).cfg.t_layers, R.case(name).cfg.t_heads, 77)
    vit = ModelShape.from_state_dict(synth.random_clip_state_shapes(ModelShape()), 4, 12)
    assert vit == ModelShape() and not vit.resnet and vit.v_stages == ()
    assert ModelShape.from_config(O.VIT_B16, 4, 12) == ModelShape()
    # RN101 from the keys alone: one-element tensors stand for everything whose size is not read
    rn101 = ModelShape(**synth.RESNET_SHAPES["RN101"])
    keys = {k: torch.empty(s, device="meta") for k, s, _ in synth.clip_state_table(rn101)}
    got = ModelShape.from_state_dict(keys, 0, 1)
    assert got.v_stages == (3, 4, 23, 3) and (got.v_width, got.image_size, got.v_heads, got.embed_dim, got.v_layers) == (64, 224, 32, 512, 33)
    assert sorted(k for k in keys if k.startswith("visual.")) == sorted(R.make_rn_state(rn101, 0))  # synth and the fixtures' recipe name the same tensors
    for name in ("RN50", "RN101", "RN50x16", "RN50x64"):  # the released towers the library runs: head dimension 64, width % 32 == 0
        s = ModelShape(**synth.RESNET_SHAPES[name])
        assert s.resnet and s.v_width % 32 == 0 and 32 * s.v_width // s.v_heads == 64 and s.v_layers == sum(s.v_stages)


@pytest.mark.parametrize("cout,cin,k,ldk", [(5, 8, 3, 128), (16, 32, 1, 64)])
def test_conv_pack_is_the_float64_fold(lib, cout, cin, k, ldk):
    """mudpt_conv_pack against the fold in float64: T values bit-equal to torch rounding the float64 product once, (ky, kx, c) order, the
    ldk tail zero, the bias the float64 value rounded to fp32."""
    g = torch.Generator().manual_seed(cout)
    w = torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5
    gamma, beta, mean, var = 0.75 + 0.5 * torch.rand(cout, generator=g), 0.1 * torch.randn(cout, generator=g), 0.1 * torch.randn(cout, generator=g), 0.5 + torch.rand(cout, generator=g)
    scale = gamma.double() / torch.sqrt(var.double() + 1e-5)
    w64 = (w.double() * scale[:, None, None, None]).permute(0, 2, 3, 1).reshape(cout, k * k * cin)
    b64 = beta.double() - mean.double() * scale
    for code, T in ((capi.F16, torch.float16), (capi.BF16, torch.bfloat16)):
        out = torch.full((cout, ldk), 7.0, dtype=T)
        bias = torch.full((cout,), 7.0)
        assert capi.call("mudpt_conv_pack", dtype=code, w=w, gamma=gamma, beta=beta, mean=mean, var=var, cout=cout, cin=cin, k=k, ldk=ldk, w_out=out, bias_out=bias) == 0
        assert torch.equal(out[:, :k * k * cin].view(torch.int16), w64.to(T).view(torch.int16))
        assert (out[:, k * k * cin:] == 0).all() and k * k * cin <= ldk
        assert torch.equal(bias, b64.float())
    assert capi.call("mudpt_conv_pack", dtype=capi.F16, w=w, gamma=gamma, beta=beta, mean=mean, var=var, cout=cout, cin=cin, k=k, ldk=k * k * cin - 1, w_out=out,
                     bias_out=bias) == 1 and b"ldk" in lib.mudpt_last_error()
    assert capi.call("mudpt_conv_pack", dtype=capi.F16, w=w, cout=cout, cin=cin, k=k, ldk=ldk) == 1 and b"null" in lib.mudpt_last_error()


REFUSALS = [  # (config changes, shape changes, the word of the message)
    ({"image_size": 200}, {}, b"image_size"),
    ({}, {"layers3": 0}, b"layers"),
    ({}, {"width": 80, "heads": 40}, b"RN50x4"),
    ({}, {"width": 48, "heads": 24}, b"width"),
    ({}, {"heads": 0}, b"heads"),
    ({}, {"heads": 7}, b"heads"),
    ({}, {"heads": 16}, b"head dimension"),
    ({"dtype": capi.F32}, {}, b"ResNet towers run in bf16 / fp16; the parity mode is not built for them"),
]


@pytest.mark.parametrize("cfg_kw,rn_kw,word", REFUSALS)
def test_create_refusals_need_no_device(lib, cfg_kw, rn_kw, word):
    """Every refusal of mudpt_create_frozen_resnet is MUDPT_ERR_ARG with a message that names the field, before any GPU call (this process
    has no device)."""
    cfg = dict(image_size=224, patch=0, v_width=0, v_layers=0, v_heads=0, t_width=512, t_layers=12, t_heads=8, ctx_len=77, embed_dim=1024, n_ctx=0, depth=0, n_cls=11,
               max_batch=4, dtype=capi.F16, variant=0)
    rn = dict(layers1=3, layers2=4, layers3=6, layers4=3, width=64, heads=32)
    cfg.update(cfg_kw)
    rn.update(rn_kw)
    h = C.c_void_p()
    assert lib.mudpt_create_frozen_resnet(C.byref(capi.Config(**cfg)), C.byref(capi.ResnetShape(**rn)), C.byref(h)) == 1
    assert word in lib.mudpt_last_error(), lib.mudpt_last_error()
    assert not h.value


def test_create_refuses_null_pointers(lib):
    h = C.c_void_p()
    cfg, rn = capi.Config(224, 0, 0, 0, 0, 512, 12, 8, 77, 1024, 0, 0, 11, 4, capi.F16, 0), capi.ResnetShape(3, 4, 6, 3, 64, 32)
    for args in ((None, C.byref(rn), C.byref(h)), (C.byref(cfg), None, C.byref(h)), (C.byref(cfg), C.byref(rn), None)):
        assert lib.mudpt_create_frozen_resnet(*args) == 1 and b"null" in lib.mudpt_last_error()


def test_custom_clip_refuses_a_resnet_shape():
    from mudpt_amd.model import CustomCLIP
    with pytest.raises(AssertionError, match="ResNet backbones run on the frozen handle only \\(ZeroshotCLIP, ZeroshotCLIP2, feature extraction\\)"):
        CustomCLIP(ModelShape(**synth.RESNET_SHAPES["RN50"]), {}, torch.zeros(2, 77, dtype=torch.int32))
