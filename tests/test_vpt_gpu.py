"""GPU parity of the VPT / MPT paths (trainers/vpt.py, trainers/mpt.py) through the C ABI: the HIP library with ``variant = "vpt" / "mpt"``
against the fixtures of the reference's own modules (tests/golden/gen_golden_vpt.py) and the test-local restatement (tests/vpt_reference.py)."""
import ctypes as C

import pytest
import torch

from oracle import mudpt_oracle as O
from tests import vpt_reference as R
from tests.helpers import (assert_training_forward_is_the_inference_forward, check_grads, check_logits, check_parity_mode_at_scale_100,
                           check_sampled_taps)
from tests.test_model_gpu import LOGIT_ATOL

pytestmark = pytest.mark.gpu
PARITY = [f for f in R.FIXTURES if not f.endswith("_s100")]


def build(case, dtype, max_batch=None, knobs=None, params=None):
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape.from_config(case.cfg, 4, 1)
    m = CustomCLIP(shape, case.frozen, case.tokens, ctx_token_ids=case.ctx_token_ids or None, max_batch=max_batch or len(case.labels),
                   dtype=dtype, variant=case.variant, knobs=knobs, prompt_shape=case.shape)
    assert m.param_names == case.keys
    if case.trainer == "MPT":  # the module's own init of the text ctx is the reference's (trainers/mpt.py:55-62)
        assert torch.equal(m.state_dict()[R.TEXT_CTX].cpu(), case.params[R.TEXT_CTX])
    m.set_params(case.params if params is None else params)
    return m


@pytest.fixture(scope="module", params=PARITY)
def case(request):
    return R.VptCase(request.param)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_logits_loss_grads_taps_match_reference(case, dtype):
    m = build(case, dtype)
    m.eval()
    logits = m(case.images).cpu()
    slack = check_logits(logits, case, dtype, f"{case.name} {dtype}")
    check_sampled_taps(m, case, dtype)  # the spliced rows of the sampled block inputs
    m.train()
    loss, logits2 = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    assert_training_forward_is_the_inference_forward(logits2, logits, dtype)
    assert abs(loss.item() - case.loss) <= slack * LOGIT_ATOL[dtype]
    check_grads(m.grads(), case.grads, dtype, f"{case.name} {dtype}")
    m.close()


@pytest.mark.parametrize("name", ["vpt_vitb16_b2_s100", "mpt_vitb16_b2_s100"])
def test_parity_mode_at_logit_scale_100(name):
    case = R.VptCase(name)
    check_parity_mode_at_scale_100(build(case, "fp32"), case)


@pytest.mark.parametrize("name", ["vpt_tiny", "mpt_tiny", "mpt_tiny_textonly", "vpt_vitb16_b2_s100", "mpt_vitb16_b2_s100"])
def test_parity_mode_training_step(name):
    """One training step on a dtype "fp32" handle: the forward is the inference forward bit for bit, the loss is the fixture's within the
    parity mode's logit bound, every gradient passes check_grads with the bf16 constants against the fixture and the restatement, and
    inside that twice the figures this fixture measured (test_knobs_gpu.PARITY_STEP_MEASURED)."""
    from tests.helpers import check_parity_step_grads
    from tests.test_exact_gpu import LOGIT_ATOL_EXACT
    from tests.test_knobs_gpu import PARITY_STEP_MEASURED
    case = R.VptCase(name)
    m = build(case, "fp32")
    m.eval()
    logits = m(case.images).cpu()
    m.train()
    loss, logits2 = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    assert_training_forward_is_the_inference_forward(logits2, logits, "fp32")
    slack = 1.0 if case.cfg.v_layers >= 12 else 3.0  # test_exact_gpu.py::test_logits_at_scale_100_within_1e_3: the tiny shape in the default parity mode
    print(f"{name} parity mode: |loss - reference| {abs(loss.item() - case.loss):.3e} |logit - reference| max {(logits - case.logits).abs().max().item():.3e}")
    assert abs(loss.item() - case.loss) <= slack * LOGIT_ATOL_EXACT
    got = {k: v.detach().cpu().clone() for k, v in m.grads().items()}
    m.close()
    restated = R.forward_backward(case.cfg, case.frozen, case.params, case.trainer, case.shape, case.class_embedding, case.eot, case.images, case.labels)[2]
    check_grads(got, case.grads, "bf16", f"{name} fp32 vs fixture")
    check_grads(got, restated, "bf16", f"{name} fp32 vs restatement")
    check_parity_step_grads(name, [(k, got[k], restated[k]) for k in case.keys], PARITY_STEP_MEASURED[name])


def test_vpt_text_features_are_computed_once():
    """VPT's text tower has nothing to learn: after the first pass no step and no eval forward launches a text-tower pass or a text-side
    head kernel, and the logits are those of a handle that recomputes them."""
    case = R.VptCase("vpt_tiny")
    m = build(case, "fp16")
    lib = m.lib
    count = lambda: int(m.debug_read("text_launches", 1)[0].item())  # noqa: E731
    m.train()
    m.forward_backward(case.images, case.labels)
    first = count()
    assert first >= 1
    loss2, logits2 = m.forward_backward(case.images, case.labels, return_logits=True)
    m.eval()
    ev = m(case.images)
    m.invalidate_text_cache()
    ev2 = m(case.images)
    torch.cuda.synchronize()
    assert count() == first, (first, count())
    assert torch.equal(ev, ev2)
    # a fresh handle's first step (text tower run) gives the same loss and logits bit for bit
    m2 = build(case, "fp16")
    loss3, logits3 = m2.forward_backward(case.images, case.labels, return_logits=True)
    assert torch.equal(logits2, logits3) and loss2.item() == loss3.item()
    assert torch.equal(m.flat_grads, m2.flat_grads)
    # a frozen weight change invalidates the cached features
    w = case.frozen["ln_final.bias"] + 0.5
    assert lib.mudpt_set_weight(m._h, b"ln_final.bias", C.c_void_p(w.data_ptr()), w.numel()) == 0
    ev3 = m(case.images)
    torch.cuda.synchronize()
    assert count() > first and not torch.equal(ev3, ev)
    m.close()
    m2.close()


@pytest.mark.parametrize("name", ["vpt_tiny", "mpt_tiny", "mpt_vitb16_b2"])
def test_two_identical_steps_give_bit_identical_grads(name):
    case = R.VptCase(name)
    m = build(case, "bf16")
    m.forward_backward(case.images, case.labels)
    g1 = m.flat_grads.clone()
    m.forward_backward(case.images, case.labels)
    assert torch.equal(g1, m.flat_grads)
    assert g1.abs().sum().item() > 0
    m.close()


@pytest.mark.parametrize("name", ["mpt_tiny", "vpt_tiny_shallow", "mpt_tiny_textonly"])
def test_three_sgd_steps_track_the_restatement(name):
    case = R.VptCase(name)
    m = build(case, "fp16")
    ref = {k: v.clone() for k, v in case.params.items()}
    bufs = {}
    lr = 0.05
    for step in range(3):
        m.forward_backward(case.images, case.labels)
        m.sgd_step(lr, momentum=0.9, weight_decay=5e-4)
        _, _, g = R.forward_backward(case.cfg, case.frozen, ref, case.trainer, case.shape, case.class_embedding, case.eot, case.images, case.labels)
        for k in ref:
            ref[k], bufs[k] = O.sgd_step(ref[k], g[k], bufs.get(k), lr, 0.9, 5e-4)
    torch.cuda.synchronize()
    got = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for k, r in ref.items():
        moved = (r - case.params[k]).abs().max().item()
        err = (got[k] - r).abs().max().item()
        print(f"{name} {k}: moved {moved:.3e} err {err:.3e}")
        assert moved > 0 and err <= 0.05 * moved + 1e-6, (k, err, moved)
    m.close()


@pytest.mark.parametrize("name", ["vpt_vitb16_b2", "mpt_tiny"])
def test_eval_logits_do_not_depend_on_the_test_batch(name):
    case = R.VptCase(name)
    imgs = torch.cat([case.images, case.images.flip(0), case.images])
    m = build(case, "bf16", max_batch=imgs.shape[0])
    m.eval()
    whole = m(imgs)
    parts = torch.cat([m(imgs[i:i + 1]) for i in range(imgs.shape[0])])
    assert torch.equal(whole, parts)
    m.close()


@pytest.mark.parametrize("trainer", ["VPT", "MPT"])
def test_plugin_trains_checkpoints_and_evaluates(tmp_path, trainer):
    from mudpt_amd import dassl_lite, vpt  # noqa: F401  (registers VPT / MPT)
    model_name = {"VPT": "VisualPromptLearner", "MPT": "MultiModalPromptLearner"}[trainer]

    def cfg_for(out):
        cfg = dassl_lite.default_cfg()
        cfg.TRAINER.NAME = trainer
        node = getattr(cfg.TRAINER, trainer)
        node.DEEP_TEXT_N_CTX, node.TEXT_PROMPT_DEPTH, node.DEEP_VISUAL_N_CTX, node.VISUAL_PROMPT_DEPTH = vpt.YAML_PROMPTS[trainer]
        cfg.OUTPUT_DIR = str(out)
        cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.LR = 2, 0, 0.02
        cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 8, 8
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 4, 4
        return cfg
    t = dassl_lite.build_trainer(cfg_for(tmp_path))
    assert type(t).__name__ == trainer and t.get_model_names() == [model_name]
    keys = [k for k, _ in R.trainable_keys(O.VIT_B16, trainer, vpt.YAML_PROMPTS[trainer])]
    assert list(t.model.state_dict()) == keys
    batch = t.train_loader_x[0]
    t.batch_idx, t.num_batches = 0, 99
    s = t.forward_backward(batch)
    assert set(s) == {"loss", "acc"} and 0.0 <= s["acc"] <= 100.0
    t.train()
    ck = torch.load(str(tmp_path / model_name / "model.pth.tar-2"), map_location="cpu")
    assert list(ck["state_dict"]) == keys
    logits = t.model_inference(batch["img"].cuda())
    t2 = dassl_lite.build_trainer(cfg_for(tmp_path / "fresh"))
    t2.load_model(str(tmp_path), epoch=2)
    assert torch.equal(t2.model.flat_params, t.model.flat_params)
    assert torch.equal(t2.model_inference(batch["img"].cuda()), logits)
    assert 0.0 <= t2.test() <= 100.0


def test_refusals():
    from mudpt_amd import capi
    lib = capi.load()
    for name in ("vpt_tiny", "mpt_tiny"):
        m = build(R.VptCase(name), "fp16")
        assert lib.mudpt_set_class_shard(m._h, 0, 2) == 1 and b"VPT / MPT" in lib.mudpt_last_error()
        f, df, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert lib.mudpt_cp_buffers(m._h, C.byref(f), C.byref(df), C.byref(n)) == 1
        assert lib.mudpt_cp_backward(m._h, capi.CP_TEXT, None) == 1
        assert lib.mudpt_set_class_token_position(m._h, capi.CLASS_TOKEN_END, None) == 1
        m.close()
