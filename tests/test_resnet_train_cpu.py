"""No-GPU checks of CoOp / CoCoOp on CLIP's ResNet image tower (mudpt_create_resnet): the refusals of the library and of CustomCLIP, and
the fixtures of tests/golden/gen_golden_resnet_train.py against the float64 restatement the GPU tests' bounds rest on."""
import ctypes as C
import os

import pytest
import torch

from mudpt_amd import build, capi, synth
from mudpt_amd.model import ModelShape
from tests import resnet_train_reference as RT
from tests.helpers import LOGIT_ATOL, LOGIT_RMS, TINY_SLACK
from tests.test_resnet_cpu import REFUSALS


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


def create(lib, cfg_kw=None, rn_kw=None):
    cfg = dict(image_size=224, patch=0, v_width=0, v_layers=0, v_heads=0, t_width=512, t_layers=12, t_heads=8, ctx_len=77, embed_dim=1024, n_ctx=16, depth=0, n_cls=11,
               max_batch=4, dtype=capi.F16, variant=capi.VARIANT_COOP)
    rn = dict(layers1=3, layers2=4, layers3=6, layers4=3, width=64, heads=32)
    cfg.update(cfg_kw or {})
    rn.update(rn_kw or {})
    h = C.c_void_p()
    rc = lib.mudpt_create_resnet(C.byref(capi.Config(**cfg)), C.byref(capi.ResnetShape(**rn)), C.byref(h))
    return rc, lib.mudpt_last_error(), h


@pytest.mark.parametrize("cfg_kw,rn_kw,word", REFUSALS)
@pytest.mark.parametrize("variant", [capi.VARIANT_COOP, capi.VARIANT_COOP_CSC, capi.VARIANT_COCOOP])
def test_create_resnet_refuses_what_the_frozen_handle_refuses(lib, variant, cfg_kw, rn_kw, word):
    """tests/test_resnet_cpu.py's table, word for word, on the trainable entry point: MUDPT_ERR_ARG before any GPU call (this process has no
    device)."""
    rc, msg, h = create(lib, dict(cfg_kw, variant=variant), rn_kw)
    assert rc == 1 and word in msg and msg.startswith(b"create_resnet:"), msg
    assert not h.value


@pytest.mark.parametrize("variant,name", [(capi.VARIANT_MUDPT, b"MuDPT"), (capi.VARIANT_VPT, b"VPT"), (capi.VARIANT_MPT, b"MPT"), (capi.VARIANT_UMUDPT, b"UMuDPT"),
                                          (capi.VARIANT_UUMUDPT, b"UUMuDPT")])
def test_create_resnet_refuses_the_variants_whose_prompts_live_inside_a_vit(lib, variant, name):
    rc, msg, h = create(lib, dict(variant=variant, n_ctx=4, depth=9))
    assert rc == 1 and name in msg and b"its prompts live inside a ViT" in msg, msg
    assert not h.value
    rc, msg, h = create(lib, dict(variant=99))
    assert rc == 1 and b"unknown variant 99" in msg and not h.value


def test_create_resnet_refuses_null_pointers(lib):
    h = C.c_void_p()
    cfg, rn = capi.Config(224, 0, 0, 0, 0, 512, 12, 8, 77, 1024, 16, 0, 11, 4, capi.F16, capi.VARIANT_COOP), capi.ResnetShape(3, 4, 6, 3, 64, 32)
    for args in ((None, C.byref(rn), C.byref(h)), (C.byref(cfg), None, C.byref(h)), (C.byref(cfg), C.byref(rn), None)):
        assert lib.mudpt_create_resnet(*args) == 1 and b"null" in lib.mudpt_last_error()


@pytest.mark.parametrize("variant", ["mudpt", "vpt", "mpt", "umudpt", "uumudpt"])
def test_custom_clip_refuses_a_resnet_shape_for_every_other_variant(variant):
    from mudpt_amd.model import CustomCLIP
    with pytest.raises(AssertionError, match="ResNet backbones run on the frozen handle only \\(ZeroshotCLIP, ZeroshotCLIP2, feature extraction\\)"):
        CustomCLIP(ModelShape(**synth.RESNET_SHAPES["RN50"]), {}, torch.zeros(2, 77, dtype=torch.int32), variant=variant)


@pytest.mark.parametrize("name", RT.FIXTURES)
def test_float64_restatement_reproduces_the_reference_logits(name):
    """The tower of tests/resnet_reference.py in float64 and the trainer's forward behind it (the oracle's fp32 text tower) against the
    logits the reference's own CustomCLIP gave in fp32 (test_resnet_cpu.py's tolerance for the same comparison); the raw features to 1e-5
    of their norm."""
    from tests import resnet_reference as R
    c = RT.case(name)
    with torch.no_grad():
        feat = R.image_features(c.rn, c.images, c.stages, c.heads)
        logits = RT.logits_from_features(c, feat)
    assert R.feature_error(feat, c.image_features) <= 1e-5
    err = (logits - c.logits.double()).abs().max().item()
    print(f"{name}: |restated - reference| logits max {err:.2e}")
    torch.testing.assert_close(logits.float(), c.logits, atol=2e-5, rtol=1e-5)
    assert c.cfg.embed_dim != c.cfg.t_width or name.startswith("rn50")  # the tiny fixtures exist for embed_dim != t_width
    if c.cocoop:
        assert tuple(c.params["prompt_learner.meta_net.linear1.weight"].shape) == (c.cfg.embed_dim // 16, c.cfg.embed_dim)


@pytest.mark.parametrize("name", RT.FIXTURES)
def test_emulated_tower_term_leaves_half_of_the_logit_bound(name):
    """What the tower's number formats alone cost at the logits is at most half of helpers.check_logits' bound for the fixture, so the GPU
    test's bound is one a correct implementation can meet; the gradient terms are small against check_fixture_grads' bounds too."""
    c = RT.case(name)
    slack = TINY_SLACK if c.cfg.v_layers < 12 else 1.0
    for dtype, (worst, rms) in c.emulated_logit.items():
        print(f"{name} {dtype}: emulated tower term on the logits max {worst:.2e} rms {rms:.2e}")
        assert 0 < worst <= 0.5 * slack * LOGIT_ATOL[dtype] and 0 < rms <= 0.5 * slack * LOGIT_RMS[dtype], (name, dtype, worst, rms)
    for k in c.keys:
        for dtype, (worst, rms) in c.emulated_grad[k].items():
            assert 0 < rms <= worst, (name, k, dtype)
