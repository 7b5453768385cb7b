"""The custom-loss step without a device: the new declarations of include/mudpt.h are bound and exported, the host-side refusals of
mudpt_head_grad and of the split step's entry points answer before any launch (the addresses below are never dereferenced), and a trainer
plugin without ``compute_loss`` still makes the ONE library call it made before."""
import ctypes as C

import pytest
import torch
from torch import nn

from mudpt_amd import capi, dassl_lite, trainer

NEW = ("mudpt_head_grad", "mudpt_forward_train", "mudpt_train_features", "mudpt_backward_logits", "mudpt_train_token", "mudpt_train_release")
ADDR = 0x1000  # stands for a device buffer: a refusal comes before anything reads it


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_declared_bound_and_exported(lib):
    for name in NEW:
        assert name in capi.declared_functions() and name in capi.SIGNATURES
        assert getattr(lib, name).argtypes == capi.SIGNATURES[name][1]
    assert [n for n, _ in capi.DECLARATIONS["mudpt_backward_logits"][1]] == ["m", "dlogits_dev", "dimg_dev", "dtxt_dev", "batch", "grad_scale", "stream"]
    assert dict(capi.DECLARATIONS["mudpt_head_grad"][1])["ldg"] is C.c_int64


def head_grad(**kw):
    args = dict(img_n=ADDR, img_inv=ADDR, txt_n=ADDR, txt_inv=ADDR, G=ADDR, ldg=11, Eimg=ADDR, Etxt=ADDR, scale=14.2857, gmul=384.0, B=3, C=11, e=128,
                dimg=ADDR, dtxt=ADDR, path=0)
    args.update(kw)
    return capi.call("mudpt_head_grad", **args)


@pytest.mark.parametrize("change,word", [
    (dict(img_n=None), "img_n"), (dict(img_inv=None), "img_inv"), (dict(txt_n=None), "txt_n"), (dict(txt_inv=None), "txt_inv"),
    (dict(B=0), "B=0"), (dict(C=0), "C=0"), (dict(e=0), "e=0"), (dict(ldg=10), "ldg=10"),
    (dict(dimg=None, dtxt=None), "dimg and dtxt"), (dict(G=None, Eimg=None, Etxt=None), "G, Eimg and Etxt"),
    (dict(path=3), "path"), (dict(path=2, e=72), "fused form does not take e=72"), (dict(path=2, e=1040), "fused form does not take e=1040"),
])
def test_head_grad_refusals_name_the_field(lib, change, word):
    rc = head_grad(**change)
    msg = lib.mudpt_last_error().decode()
    assert rc == 1 and word in msg and msg.startswith("head_grad:"), (rc, msg)


def test_head_grad_refusals_hold_on_the_unfused_path_too(lib):
    for change, word in ((dict(e=72, B=0), "B=0"), (dict(path=1, ldg=3), "ldg=3"), (dict(path=1, dimg=None, dtxt=None), "dimg and dtxt")):
        rc = head_grad(**change)
        assert rc == 1 and word in lib.mudpt_last_error().decode()


def test_split_step_refuses_a_null_model(lib):
    for name, kw in (("mudpt_forward_train", dict(images_dev=ADDR, batch=2, logits_dev=ADDR)),
                     ("mudpt_train_features", dict(batch=2, image_features_dev=ADDR, text_features_dev=ADDR)),
                     ("mudpt_backward_logits", dict(dlogits_dev=ADDR, batch=2, grad_scale=1.0)), ("mudpt_train_token", dict(expect=1)),
                     ("mudpt_train_release", {})):
        rc = capi.call(name, m=None, **kw)
        assert rc == 1 and "null model" in lib.mudpt_last_error().decode(), name


class _StepModel(nn.Module):
    """The surface data_parallel_step uses, recording which entry made the step."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(2))
        self.flat_params, self.flat_grads = self.w.data, torch.zeros(2)
        self.w.grad = self.flat_grads
        self.calls = []

    def forward_backward(self, image, label, grad_scale=1.0, return_logits=False):
        self.calls.append(("forward_backward", tuple(image.shape), grad_scale))
        self.flat_grads.fill_(1.0)
        loss = torch.tensor(0.5)
        return (loss, torch.eye(2)[label]) if return_logits else loss

    def differentiable(self, image, grad_scale=1.0):
        from mudpt_amd.model import ClipOutputs
        self.calls.append(("differentiable", tuple(image.shape), grad_scale))
        model = self

        class Step(torch.autograd.Function):
            @staticmethod
            def forward(ctx, anchor):
                return torch.tensor([[2.0, 0.0], [0.0, 2.0]])

            @staticmethod
            def backward(ctx, g):
                model.flat_grads.add_(g.sum(dim=0))  # a side effect, as the library's: .grad stays the bucket's view
                return None

        return ClipOutputs(Step.apply(torch.zeros((), requires_grad=True)), torch.zeros(2, 4), torch.zeros(2, 4))

    def invalidate_text_cache(self):
        pass


def synthetic_batch():
    """The first two items of dassl_lite's synthetic training set, as its loader collates them."""
    cfg = dassl_lite.default_cfg()
    cfg.INPUT.SIZE = (32, 32)
    dm = dassl_lite.SyntheticDataManager(cfg, ["cat", "dog"])
    batch = dm.train_loader_x[0]
    return {"img": batch["img"][:2], "label": batch["label"][:2]}


def stepped(cls):
    t = object.__new__(cls)
    t.model = _StepModel()
    t.optim = torch.optim.SGD(t.model.parameters(), lr=0.1)
    t.device, t.batch_idx, t.num_batches = torch.device("cpu"), 0, 99
    batch = synthetic_batch()
    return t, batch, t.forward_backward(batch)


def test_plugin_without_compute_loss_takes_the_fused_step():
    assert trainer.PromptTrainer.compute_loss is None

    class Plain(trainer.MuDPT):
        pass

    t, batch, summary = stepped(Plain)
    assert t.model.calls == [("forward_backward", tuple(batch["img"].shape), 1.0)]
    assert summary == {"loss": 0.5} and torch.allclose(t.model.w.detach(), torch.full((2,), 0.9))


def test_plugin_with_compute_loss_goes_through_differentiable():
    class Smoothed(trainer.MuDPT):
        def compute_loss(self, out, label):
            return torch.nn.functional.cross_entropy(out.logits, label, label_smoothing=0.1)

    t, batch, summary = stepped(Smoothed)
    assert t.model.calls == [("differentiable", tuple(batch["img"].shape), 1.0)]
    logits = torch.tensor([[2.0, 0.0], [0.0, 2.0]], requires_grad=True)
    want = torch.nn.functional.cross_entropy(logits, batch["label"], label_smoothing=0.1)
    want.backward()
    assert summary["loss"] == pytest.approx(want.item(), rel=1e-6)
    assert t.model.w.grad is t.model.flat_grads  # the bucket's view, not a tensor of autograd's
    assert torch.allclose(t.model.w.detach(), 1.0 - 0.1 * logits.grad.sum(dim=0), atol=1e-7)


def test_cocoop_plugin_refuses_compute_loss():
    from mudpt_amd import cocoop

    class Custom(cocoop.CoCoOp):
        def compute_loss(self, out, label):
            return out.logits.sum()

    t = object.__new__(Custom)
    t.cfg = dassl_lite.default_cfg()
    with pytest.raises(AssertionError, match="CoCoOp takes no compute_loss"):
        t.build_model()
    object.__new__(cocoop.CoCoOp).check_compute_loss()  # the plugin as registered: nothing to refuse
