"""GPU tests of CoOp / CoCoOp on CLIP's ResNet image tower (``mudpt_create_resnet``) against the fixtures of the reference's own
``trainers.coop.CustomCLIP`` / ``trainers.cocoop.CustomCLIP`` over its ``ModifiedResNet`` (tests/golden/gen_golden_resnet_train.py).

Bounds: the logits under helpers.check_logits, the loss within its slack x LOGIT_ATOL (as the variants' suites hold it), every gradient under
helpers.check_fixture_grads' two bounds (largest error 4 GRAD_RTOL x the tensor's rms, rms error GRAD_RMS x it) plus THREE times the fixture's
emulated tower term for that tensor -- what the tower's number formats alone do to that gradient, computed by the generator on the CPU; three is
the factor tests/test_resnet_gpu.py gives the same emulation.  The measured values are printed beside each bound; DESIGN.md 4.10 holds the
table."""
import pytest
import torch

from mudpt_amd import capi
from tests import resnet_train_reference as RT
from tests.helpers import GRAD_RMS, GRAD_RTOL, LOGIT_ATOL, assert_training_forward_is_the_inference_forward, check_logits

pytestmark = pytest.mark.gpu


def build(case, dtype, max_batch=None, tokens=None, name_lens=None, params=None, state=None):
    from mudpt_amd.model import CustomCLIP
    kw = {} if case.cocoop else dict(class_token_position=case.position, name_lens=case.name_lens if name_lens is None else name_lens)
    m = CustomCLIP(case.shape(), case.state if state is None else state, case.tokens if tokens is None else tokens, max_batch=max_batch or len(case.labels),
                   dtype=dtype, variant=case.variant, **kw)
    assert m.param_names == case.keys
    m.set_params(case.params if params is None else params)
    return m


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", RT.FIXTURES)
def test_logits_loss_grads_match_reference(name, dtype):
    case = RT.case(name)
    m = build(case, dtype)
    m.eval()
    logits = m(case.images).cpu()
    feat = m.image_features().cpu()
    slack = check_logits(logits, case, dtype, f"{name} {dtype}")
    m.train()
    loss, logits2 = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    got = {k: v.detach().float().cpu() for k, v in m.grads().items()}
    m.close()
    assert_training_forward_is_the_inference_forward(logits2, logits, dtype)
    print(f"{name} {dtype}: raw image features, relative {RT.R.feature_error(feat, case.image_features):.3e}; |loss - reference| {abs(loss.item() - case.loss):.3e} "
          f"(bound {slack * LOGIT_ATOL[dtype]:.1e})")
    assert abs(loss.item() - case.loss) <= slack * LOGIT_ATOL[dtype]
    bad = []
    for k in case.keys:
        r = case.grads[k]
        rms = r.pow(2).mean().sqrt().item()
        emu_max, emu_rms = case.emulated_grad[k][dtype]
        err, rel = (got[k] - r).abs().max().item() / rms, (got[k] - r).pow(2).mean().sqrt().item() / rms
        b_max, b_rms = 4 * GRAD_RTOL[dtype] + 3 * emu_max, GRAD_RMS[dtype] + 3 * emu_rms
        print(f"{name} {dtype} {k}: max err / rms {err:.3e} (bound {b_max:.3e} = {4 * GRAD_RTOL[dtype]:.1e} + 3 x {emu_max:.2e}), rms err / rms {rel:.3e} "
              f"(bound {b_rms:.3e} = {GRAD_RMS[dtype]:.1e} + 3 x {emu_rms:.2e})")
        if not (err <= b_max and rel <= b_rms):
            bad.append(k)
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", RT.TINY)
def test_the_tower_is_the_frozen_handles_and_the_flow_behind_it(name, dtype):
    """mudpt_image_features of the trainable handle equals encode_image of a frozen handle on the same weights, bit for bit;
    forward_features(image_features) is forward(images), bit for bit; the training forward is the inference forward."""
    from mudpt_amd.zsclip import FrozenCLIP
    case = RT.case(name)
    B = len(case.labels)
    frozen = FrozenCLIP(case.shape(), case.state, case.tokens.to(torch.int32), max_batch=B, dtype=dtype)
    want = frozen.encode_image(case.images)
    frozen.close()
    m = build(case, dtype)
    m.eval()
    logits = m(case.images)
    feat = m.image_features()
    assert torch.equal(feat, want)
    assert torch.equal(m.forward_features(feat), logits)
    m.train()
    _, train_logits = m.forward_backward(case.images, case.labels, return_logits=True)
    assert_training_forward_is_the_inference_forward(train_logits, logits, dtype)
    with pytest.raises(capi.MudptError, match="training step"):
        m.image_features()
    m.close()


@pytest.mark.parametrize("name", RT.TINY)
def test_sgd_step_moves_the_loss_and_a_batchnorm_upload_refolds(name):
    case = RT.case(name)
    m = build(case, "fp16")
    m.train()
    loss0 = m.forward_backward(case.images, case.labels).item()
    assert m.forward_backward(case.images, case.labels).item() == loss0  # the step is a function of its inputs
    m.sgd_step(lr=0.05, momentum=0.9, weight_decay=0.0)
    loss1 = m.forward_backward(case.images, case.labels).item()
    assert loss1 != loss0 and abs(loss1 - loss0) < 1.0
    # BatchNorm again: the host-side fold runs again at the next step
    m.set_params(case.params)
    key = "visual.layer1.0.bn2.weight"
    m.set_weight(key, 2 * case.state[key])
    loss2 = m.forward_backward(case.images, case.labels).item()
    assert abs(loss2 - loss0) > 1e-4
    m.set_weight(key, case.state[key])
    assert m.forward_backward(case.images, case.labels).item() == loss0
    m.close()


def test_fp32_is_refused_with_the_librarys_sentence():
    case = RT.case("rn_coop_tiny")
    with pytest.raises(AssertionError, match="ResNet towers run in bf16 / fp16; the parity mode is not built for them"):
        build(case, "fp32")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_one_step_at_1000_classes_and_embed_1024(dtype):
    """rn_coop_tiny2_csc's tower (embed_dim 1024) with its five prompts repeated to 1000 classes: the shape the head without an image
    gradient exists for (with dimg the fused head stops at 496 classes).  Finite loss and gradients, the training logits are the inference
    logits, every repetition of a class has that class's logit, and its context gets the gradient its first copy gets."""
    case = RT.case("rn_coop_tiny2_csc")
    rep, B = 200, len(case.labels)
    m = build(case, dtype, tokens=case.tokens.repeat(rep, 1), name_lens=case.name_lens * rep, params={RT.CR.CTX: case.params[RT.CR.CTX].repeat(rep, 1, 1)})
    assert m.n_cls == 1000 and m.shape.embed_dim == 1024
    m.eval()
    logits = m(case.images)
    m.train()
    loss, train_logits = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    g = m.grads()[RT.CR.CTX].detach().cpu()
    m.close()
    assert torch.isfinite(loss).item() and torch.isfinite(g).all() and torch.isfinite(logits).all()
    assert_training_forward_is_the_inference_forward(train_logits, logits, dtype)
    lg = logits.cpu().view(B, rep, 5)
    tol = LOGIT_ATOL[dtype] * 1.5
    assert (lg - lg[:, :1]).abs().max().item() <= tol and (lg[:, 0] - case.logits).abs().max().item() <= 4 * tol
    assert abs(loss.item() - (case.loss + torch.log(torch.tensor(float(rep))).item())) <= 4 * tol  # rep copies of every class: log-sum-exp grows by log(rep)
    assert g.abs().max().item() > 0 and tuple(g.shape) == (1000, case.cfg.n_ctx, case.cfg.t_width)


@pytest.fixture
def rn50_cfg(tmp_path, monkeypatch):
    from mudpt_amd import dassl_lite, tokenizer, trainer
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_TEST_FEATURES", "MUDPT_DEVICE_TEST"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(tokenizer, "_default", None)
    monkeypatch.setattr(trainer, "_warned_fp16_scale", False)

    def make(name, out):
        cfg = dassl_lite.default_cfg()
        cfg.TRAINER.NAME = name
        cfg.MODEL.BACKBONE.NAME, cfg.MODEL.BACKBONE.SYNTHETIC_SEED = "RN50", 3
        cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 4, 4
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 2, 2
        cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.LR = 1, 0, 0.02
        cfg.OUTPUT_DIR = str(out)
        out.mkdir(exist_ok=True)
        return cfg
    return make


@pytest.mark.parametrize("name", ["CoOp", "CoCoOp"])
def test_plugin_trains_checkpoints_and_tests_from_cached_features(name, rn50_cfg, tmp_path, monkeypatch, capsys):
    """RN50 by MODEL.BACKBONE.NAME on synthetic weights, B 2, 11 classes, two iterations: a finite loss summary, a checkpoint round trip that
    reproduces the logits, and a test() pass under MUDPT_TEST_FEATURES whose results equal the image pass."""
    from mudpt_amd import cocoop, coop, dassl_lite  # noqa: F401 -- the plugins register themselves
    t = dassl_lite.build_trainer(rn50_cfg(name, tmp_path / "out"))
    assert t.model.shape.resnet and t.model.shape.v_stages == (3, 4, 6, 3) and t.model.shape.embed_dim == 1024 and t.model.n_cls == 11
    t.batch_idx, t.num_batches = 0, 99
    summaries = [t.forward_backward(batch) for batch in list(t.train_loader_x)[:2]]
    assert len(summaries) == 2 and all(torch.isfinite(torch.tensor(float(s["loss"]))).item() for s in summaries)
    t.train()
    batch = t.train_loader_x[0]
    logits = t.model_inference(batch["img"].cuda())
    assert torch.isfinite(logits).all() and tuple(logits.shape) == (2, 11)
    t2 = dassl_lite.build_trainer(rn50_cfg(name, tmp_path / "fresh"))
    t2.load_model(str(tmp_path / "out"), epoch=1)
    assert torch.equal(t2.model_inference(batch["img"].cuda()), logits)
    t2.model.close()

    def run():
        acc = t.test()
        return acc, dict(t.evaluator.evaluate()), t.evaluator._state.clone()
    on_images = run()
    monkeypatch.setenv("MUDPT_TEST_FEATURES", str(tmp_path / "feat"))
    first = run()  # on the images, and writes the file
    capsys.readouterr()
    with monkeypatch.context() as mp:
        mp.setattr(type(t.model), "forward", lambda self, x: (_ for _ in ()).throw(RuntimeError("the image forward ran")))
        cached = run()
    assert "Cached test features: 4 rows" in capsys.readouterr().out
    for got in (first, cached):
        assert got[0] == on_images[0] and got[1] == on_images[1] and torch.equal(got[2], on_images[2])
    t.model.close()
