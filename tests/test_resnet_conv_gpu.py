"""GPU tests of the ResNet tower on its fused convolution (``mudpt_resnet_conv_path`` 1: every convolution one ``mudpt_conv2d`` launch instead of
im2col + GEMM + bias_act).  The rounding sites are the default path's (resnet.hip's header), so the bounds are the ones tests/test_resnet_gpu.py
and tests/test_resnet_train_gpu.py hold that path to: 3 x ``emulated_rel`` on the raw features, helpers.check_logits on the logits, and the
training suite's own checks of logits, loss and gradients, run here as they stand with the path switched on."""
import os
import subprocess
import sys

import pytest
import torch

from tests import coop_reference as CR
from tests import resnet_reference as R
from tests import resnet_train_reference as RT
from tests import rn_fused_conv_worker as worker
from tests import test_resnet_train_gpu as TG
from tests.helpers import check_logits
from tests.test_resnet_gpu import build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build1(case, dtype, **kw):
    """tests/test_resnet_gpu.build with the fused path chosen at construction."""
    from mudpt_amd.zsclip import FrozenCLIP
    return FrozenCLIP(case.shape(), kw.get("state", case.state), case.tokens, max_batch=len(case.labels), dtype=dtype, rn_fused_conv=True)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_features_and_logits_match_the_reference_and_switching(name, dtype):
    """Path 1 under path 0's bounds; back on path 0 the handle gives the bits of one that never left it, back on path 1 its own first bits.
    |F_path1 - F_path0| / |F| is printed beside emulated_rel: DESIGN.md 4.9 holds the table."""
    case = R.case(name)
    never = build(case, dtype)
    f0 = never.encode_image(case.images)
    assert never.debug_read("conv2d_launches")[0].item() == 0
    never.close()
    m = build1(case, dtype)
    convs = 3 + sum(3 * n + 1 for n in case.stages)  # the stem; conv1 .. conv3 per Bottleneck and one downsample branch per stage
    launches = lambda: int(m.debug_read("conv2d_launches")[0].item())  # noqa: E731
    assert launches() == 0
    f1 = m.encode_image(case.images)
    assert launches() == convs  # every convolution of the tower was one launch of the new kernel
    logits = m(case.images)
    assert torch.equal(m.image_features(), f1) and launches() == 2 * convs
    m.set_resnet_conv_path(0)
    assert torch.equal(m.encode_image(case.images), f0) and launches() == 2 * convs  # the default path launches none
    m.set_resnet_conv_path(1)
    assert torch.equal(m.encode_image(case.images), f1) and launches() == 3 * convs
    with pytest.raises(AssertionError, match="path 2"):
        m.set_resnet_conv_path(2)
    assert torch.equal(m.encode_image(case.images), f1)  # a refused call changes nothing
    m.close()
    rel, bound = R.feature_error(f1, case.image_features), 3 * case.emulated_rel[dtype]
    print(f"{name} {dtype} fused convolutions: raw image features, relative: {rel:.3e} (emulated {case.emulated_rel[dtype]:.3e}, bound {bound:.3e}); "
          f"|F_path1 - F_path0| / |F| {R.feature_error(f1, f0.cpu()):.3e}, path 0 itself {R.feature_error(f0, case.image_features):.3e}")
    assert rel <= bound, (rel, bound)
    check_logits(logits, case, dtype, f"{name} {dtype} fused convolutions")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["rn_tiny", "rn_tiny2"])
def test_batch_invariance_and_the_flow_behind_the_tower(name, dtype):
    """The kernel splits no contraction and every tile form sums in one order: an image's features are the same bits alone and in a batch, and
    forward_features(encode_image(x)) is forward(x) bit for bit."""
    case = R.case(name)
    m = build1(case, dtype)
    whole = m.encode_image(case.images)
    for i in range(len(case.labels)):
        assert torch.equal(m.encode_image(case.images[i:i + 1])[0], whole[i]), i
    logits = m(case.images)
    assert torch.equal(m.forward_features(whole), logits)
    m.close()


def test_refolding_and_the_vit_handles_refusal(monkeypatch):
    """A BatchNorm tensor uploaded again is folded again on path 1 as on path 0; a handle without the tower refuses the switch, at construction too."""
    from mudpt_amd.model import ModelShape
    from mudpt_amd.zsclip import FrozenCLIP
    case = R.case("rn_tiny")
    m = build1(case, "fp16")
    want = m.encode_image(case.images)
    m.set_weight("visual.bn1.weight", 2 * case.state["visual.bn1.weight"])
    assert R.feature_error(m.encode_image(case.images), want.cpu()) > 1e-2
    m.set_weight("visual.bn1.weight", case.state["visual.bn1.weight"])
    assert torch.equal(m.encode_image(case.images), want)
    m.close()
    vit = CR.CoopCase("coop_tiny_end")  # the tiny ViT state tests/test_library_model_gpu.py builds its frozen handle from
    shape = ModelShape.from_config(vit.cfg, 0, 1)
    frozen = FrozenCLIP(shape, vit.frozen, vit.tokens, max_batch=2, dtype="fp16")
    for path in (0, 1):
        with pytest.raises(AssertionError, match="has no ResNet image tower"):
            frozen.set_resnet_conv_path(path)
    frozen.close()
    with pytest.raises(AssertionError, match="has no ResNet image tower"):
        FrozenCLIP(shape, vit.frozen, vit.tokens, max_batch=2, dtype="fp16", rn_fused_conv=True)
    monkeypatch.setenv("MUDPT_RN_FUSED_CONV", "1")  # the variable speaks to ResNet shapes only
    frozen = FrozenCLIP(shape, vit.frozen, vit.tokens, max_batch=2, dtype="fp16")
    frozen.close()


@pytest.fixture
def fused_by_environment(monkeypatch):
    """MUDPT_RN_FUSED_CONV=1 for handles built without the keyword; yields the list of paths such handles were switched to."""
    from mudpt_amd.model import LibraryModel
    monkeypatch.setenv("MUDPT_RN_FUSED_CONV", "1")
    calls, inner = [], LibraryModel.set_resnet_conv_path

    def record(self, path):
        calls.append(int(path))
        return inner(self, path)
    monkeypatch.setattr(LibraryModel, "set_resnet_conv_path", record)
    return calls


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["rn_coop_tiny", "rn_coop_tiny2_csc", "rn_cocoop_tiny", "rn50_coop_b2"])
def test_training_handles_pass_the_training_suites_checks(name, dtype, fused_by_environment):
    """tests/test_resnet_train_gpu.py's check of logits, loss and every gradient against the reference's fixture, as it stands, on a handle
    that the environment put on path 1."""
    TG.test_logits_loss_grads_match_reference(name, dtype)
    assert fused_by_environment == [1]


@pytest.mark.parametrize("name", RT.TINY)
def test_training_tower_is_the_frozen_handles_on_path_1(name, fused_by_environment):
    """The trainable handle's features are a frozen handle's, bit for bit, both on path 1; and the flow behind the tower (the training suite's test)."""
    TG.test_the_tower_is_the_frozen_handles_and_the_flow_behind_it(name, "fp16")
    assert fused_by_environment == [1, 1]  # the frozen handle, then the trainable one


def test_the_plugin_reads_the_environment_in_a_child_process(tmp_path, monkeypatch):
    """CoOp on RN50 by MODEL.BACKBONE.NAME: a child with MUDPT_RN_FUSED_CONV=1 builds a path-1 handle -- its logits are, bit for bit, those of a
    handle built here without the variable and switched explicitly."""
    from mudpt_amd import tokenizer
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_TEST_FEATURES", "MUDPT_DEVICE_TEST", "MUDPT_RN_FUSED_CONV"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(tokenizer, "_default", None)
    out = tmp_path / "child.pt"
    env = dict(os.environ, MUDPT_RN_FUSED_CONV="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rn_fused_conv_worker.py"), str(tmp_path / "child"), str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    child = torch.load(out)
    assert child["paths"] == [1]
    from mudpt_amd.model import LibraryModel
    monkeypatch.setattr(LibraryModel, "set_resnet_conv_path", LibraryModel.set_resnet_conv_path)  # put back what recorded_paths wraps
    calls = worker.recorded_paths()
    t, img = worker.plugin_logits(tmp_path / "parent")
    assert calls == []  # without the variable the plugin stays on the default path
    t.model.set_resnet_conv_path(1)
    logits = t.model_inference(img.cuda()).cpu()
    t.model.close()
    assert torch.isfinite(logits).all() and tuple(logits.shape) == (2, 11)
    assert torch.equal(child["logits"], logits)
