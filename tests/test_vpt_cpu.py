"""VPT / MPT (trainers/vpt.py, trainers/mpt.py) without a GPU: the test-local restatement against the fixtures of the reference's own
modules, the config defaults, the plugin registry and the C ABI's refusals of mudpt_create / mudpt_create_ex (all before any GPU call)."""
import ctypes as C

import pytest
import torch

from tests import vpt_reference as R


@pytest.fixture(scope="module", params=R.FIXTURES)
def case(request):
    return R.VptCase(request.param)


def test_fixture_recipe_and_trainables(case):
    img = case.images.double()
    assert abs(img.sum().item() - float(case.z["images_checksum"][0])) <= 1e-9 * img.abs().sum().item()
    assert set(case.grads) == set(case.keys) and len(case.keys) > 0
    for k in case.keys:
        assert case.grads[k].shape == case.params[k].shape


def test_restatement_reproduces_the_reference(case):
    taps = {}
    with torch.no_grad():
        logits = R.forward(case.cfg, case.frozen, case.params, case.trainer, case.shape, case.class_embedding, case.eot, case.images, taps)
    assert (logits - case.logits).abs().max().item() <= 1e-4
    for key, (ref, rows) in case.taps.items():  # sampled block inputs, after the splice
        got = taps[key.replace(".", ".x_in.", 1)][:, rows]
        assert (got - ref).abs().max().item() <= 1e-4 * (1 + ref.abs().max().item()), key
    loss, _, grads = R.forward_backward(case.cfg, case.frozen, case.params, case.trainer, case.shape, case.class_embedding, case.eot,
                                        case.images, case.labels)
    assert abs(loss.item() - case.loss) <= 1e-5
    for k in case.keys:
        ref = case.grads[k]
        assert (grads[k] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-9, k


def test_trainable_keys_follow_the_reference_rules():
    from oracle import mudpt_oracle as O
    vpt = R.trainable_keys(O.VIT_B16, "VPT", (0, 0, 8, 12))
    assert [k for k, _ in vpt] == ["image_encoder.visual_ctx"] + [f"image_encoder.transformer.resblocks.{i}.visual_ctx" for i in range(1, 12)]
    assert all(s == (8, 768) for _, s in vpt)
    mpt = R.trainable_keys(O.VIT_B16, "MPT", (2, 12, 2, 12))
    assert len(mpt) == 24 and mpt[0] == (R.TEXT_CTX, (2, 512)) and mpt[12] == ("image_encoder.visual_ctx", (2, 768))
    assert [k for k, _ in R.trainable_keys(O.VIT_B16, "MPT", (2, 30, 2, 13))] == \
        [R.TEXT_CTX] + [f"text_encoder.transformer.resblocks.{i}.visual_ctx" for i in range(1, 12)]  # depth 13: vanilla ViT (model.py:459)


def test_default_cfg_has_the_vpt_and_mpt_nodes():
    from mudpt_amd import dassl_lite
    t = dassl_lite.default_cfg().TRAINER
    for node in (t.VPT, t.MPT):  # train.py:98-113
        assert (node.DEEP_TEXT_N_CTX, node.DEEP_VISUAL_N_CTX, node.TEXT_PROMPT_DEPTH, node.VISUAL_PROMPT_DEPTH) == (0, 0, 0, 0)
        assert (node.TEXT_CTX_INIT, node.PREC) == ("a photo of a", "fp16")


def test_both_plugins_are_registered():
    from mudpt_amd import trainer, vpt
    names = trainer.TRAINER_REGISTRY.registered_names()
    assert "VPT" in names and "MPT" in names
    assert trainer.TRAINER_REGISTRY.get("VPT") is vpt.VPT and trainer.TRAINER_REGISTRY.get("MPT") is vpt.MPT
    assert vpt.YAML_PROMPTS == {"VPT": (0, 0, 8, 12), "MPT": (2, 12, 2, 12)}  # configs/trainers/{VPT,MPT}/vit_b16_c2_ep5_batch4.yaml


def _cfg(capi, variant):
    return capi.Config(32, 16, 192, 3, 3, 128, 3, 2, 77, 128, 2, 2, 5, 4, capi.BF16, variant)


def test_create_refusals_name_the_cfg_key():
    """Every refusal is an argument check before any GPU call (this box has no GPU: a call that got past the checks would fail with
    MUDPT_ERR_HIP instead of MUDPT_ERR_ARG)."""
    from mudpt_amd import capi
    lib = capi.load()
    h = C.c_void_p()
    for variant in (capi.VARIANT_VPT, capi.VARIANT_MPT):
        assert lib.mudpt_create(C.byref(_cfg(capi, variant)), C.byref(h)) == 1
        assert b"mudpt_create_ex" in lib.mudpt_last_error()
        assert lib.mudpt_create_ex(C.byref(_cfg(capi, variant)), None, C.byref(h)) == 1
        assert b"mudpt_prompt_shape" in lib.mudpt_last_error()
    refusals = [
        (capi.VARIANT_VPT, (0, 0, 0, 0), b"TRAINER.VPT.DEEP_VISUAL_N_CTX"),    # no vision prompt: nothing to train
        (capi.VARIANT_VPT, (0, 0, 8, 13), b"TRAINER.VPT.VISUAL_PROMPT_DEPTH"),  # depth above 12: the vanilla ViT (clip/model.py:459)
        (capi.VARIANT_VPT, (0, 0, 8, 0), b"TRAINER.VPT.VISUAL_PROMPT_DEPTH"),
        (capi.VARIANT_VPT, (2, 2, 8, 12), b"TRAINER.VPT.DEEP_TEXT_N_CTX"),     # text deep prompts under VPT
        (capi.VARIANT_MPT, (0, 12, 2, 12), b"TRAINER.MPT.DEEP_TEXT_N_CTX"),     # MPT without text rows
    ]
    for variant, shape, key in refusals:
        ps = capi.PromptShape(*shape)
        assert lib.mudpt_create_ex(C.byref(_cfg(capi, variant)), C.byref(ps), C.byref(h)) == 1, shape
        assert key in lib.mudpt_last_error(), (shape, lib.mudpt_last_error())
    ps = capi.PromptShape(2, 2, 2, 2)
    assert lib.mudpt_create_ex(C.byref(_cfg(capi, capi.VARIANT_MUDPT)), C.byref(ps), C.byref(h)) == 1  # the shape is for VPT / MPT only
    # valid shapes pass every argument check (then fail only at the first device allocation on a GPU-less box)
    if not torch.cuda.is_available():
        for variant, shape in ((capi.VARIANT_VPT, (0, 0, 8, 12)), (capi.VARIANT_VPT, (0, 1, 4, 1)), (capi.VARIANT_MPT, (2, 0, 0, 0)),
                               (capi.VARIANT_MPT, (2, 30, 2, 13))):
            ps = capi.PromptShape(*shape)
            assert lib.mudpt_create_ex(C.byref(_cfg(capi, variant)), C.byref(ps), C.byref(h)) == 2, (shape, lib.mudpt_last_error())


def test_header_declares_the_new_entries():
    from mudpt_amd import capi
    assert "mudpt_create_ex" in capi.declared_functions() and "mudpt_create_ex" in capi.SIGNATURES
    assert (capi.VARIANT_VPT, capi.VARIANT_MPT) == (4, 5)
    assert [f for f, _ in capi.PromptShape._fields_] == ["t_n_ctx", "t_depth", "v_n_ctx", "v_depth"]
