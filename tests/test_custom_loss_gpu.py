"""The custom-loss step on the GPU: ``CustomCLIP.differentiable`` (mudpt_forward_train -> torch autograd on the logits and the raw features ->
mudpt_backward_logits) against the fused step, against CPU autograd of the oracle / the variants' restatements under losses the fused step
cannot express, its accumulation into the flat bucket, its state machine and refusals, and the trainer hook.  Tiny fixtures only; every
reference is computed once per module and left unchanged."""
import pytest
import torch
import torch.nn.functional as F

from mudpt_amd import capi
from oracle import mudpt_oracle as O
from tests import coop_reference as CR
from tests import resnet_train_reference as RT
from tests import test_knobs_gpu as TK
from tests import test_model_gpu as TM
from tests import test_resnet_train_gpu as TRT
from tests import umudpt_reference as UR
from tests import uumudpt_reference as UUR
from tests import vpt_reference as VR
from tests.helpers import (GRAD_COS, GRAD_RMS, GRAD_RTOL, LOGIT_ATOL, TINY_SLACK, GoldenCase, assert_training_forward_is_the_inference_forward,
                           check_fixture_grads, check_grad, grad_triple)
from tests.test_exact_gpu import LOGIT_ATOL_EXACT

pytestmark = pytest.mark.gpu
# dtype "fp32" is the parity mode: an fp16-typed backward with the gradient stream in T (lp_grad 1), which helpers.check_parity_step_grads
# and test_knobs_gpu.py grade by the bf16 row; its logits are held to the parity mode's own bound (3 x on the tiny shape, as the suites do)
GRADE = {"fp16": "fp16", "bf16": "bf16", "fp32": "bf16"}
LOSS_SLACK = {"fp16": TINY_SLACK * LOGIT_ATOL["fp16"], "bf16": TINY_SLACK * LOGIT_ATOL["bf16"], "fp32": 3.0 * LOGIT_ATOL_EXACT}
_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def tiny():
    def make():
        c = GoldenCase("mudpt_tiny")
        c.keys = list(O.TRAINABLE_ORDER)
        c.load_grads()
        assert set(c.grads) | set(c.grad_samples) == set(c.keys)
        return c
    return cached("mudpt_tiny", make)


def host_grads(m):
    torch.cuda.synchronize()
    return {k: g.detach().cpu().clone() for k, g in m.grads().items()}


def custom_step(m, images, loss_fn, zero=True):
    """differentiable + loss_fn(out) + backward on a (by default) zeroed bucket -> (loss, ClipOutputs, host gradients)."""
    if zero:
        m.flat_grads.zero_()
    out = m.differentiable(images)
    loss = loss_fn(out)
    loss.backward()
    return loss.item(), out, host_grads(m)


def leaves(params):
    return {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}


def leaf_grads(leaf):
    return {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def held(got, ref, grade, tag, **kw):
    """check_grad of every tensor; exactly zero where the reference is (a tensor no term of the loss reaches)."""
    for k, r in ref.items():
        if got[k].numel() == 0:
            continue
        if r.abs().max().item() == 0:
            assert torch.count_nonzero(got[k]) == 0, (tag, k)
        else:
            check_grad(got[k], r, grade, f"{tag} {k}", **kw)


# ---- 1. cross-entropy through the new path is the fused step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_cross_entropy_equals_the_fused_step(dtype):
    c, grade = tiny(), GRADE[dtype]
    labels = c.labels.cuda()
    a, b = TM.build(c, dtype), TM.build(c, dtype)
    loss_b, logits_b = b.forward_backward(c.images, c.labels, return_logits=True)
    fused, loss_b = host_grads(b), loss_b.item()
    loss_a, out, custom = custom_step(a, c.images, lambda o: F.cross_entropy(o.logits, labels))
    print(f"mudpt_tiny {dtype}: loss fused {loss_b:.6f} custom {loss_a:.6f} (difference {abs(loss_a - loss_b):.3e}, slack {LOSS_SLACK[dtype]:.1e}); "
          f"logits differ by {(out.logits - logits_b).abs().max().item():.3e}")
    assert abs(loss_a - loss_b) <= LOSS_SLACK[dtype] and abs(loss_a - c.loss) <= LOSS_SLACK[dtype]
    worst = [0.0, 0.0, 1.0]
    for k in c.keys:
        emax, erms, cos = grad_triple(custom[k], fused[k])
        worst = [max(worst[0], emax), max(worst[1], erms), min(worst[2], cos)]
        print(f"mudpt_tiny {dtype} {k}: custom vs fused max {emax:.3e} x rms, rms {erms:.3e} x rms, cos {cos:.8f}")
        assert erms <= GRAD_RMS[grade] and cos > GRAD_COS[grade], (k, erms, cos)
    print(f"mudpt_tiny {dtype}: worst tensor, custom vs fused: max {worst[0]:.3e} x rms, rms {worst[1]:.3e} x rms, cos {worst[2]:.8f}")
    check_fixture_grads(custom, c, grade, f"mudpt_tiny {dtype} custom vs fixture")
    check_fixture_grads(fused, c, grade, f"mudpt_tiny {dtype} fused vs fixture")
    a.eval()
    assert_training_forward_is_the_inference_forward(out.logits, a(c.images), dtype)
    for m in (a, b):
        m.close()


# ---- 2. a loss the fused step cannot express ---------------------------------------------------------------------------------------------------
def anchors(c):
    g = torch.Generator().manual_seed(123)
    A = torch.randn(len(c.classnames), c.cfg.embed_dim, generator=g)
    return A, torch.randn(len(c.labels), c.cfg.embed_dim, generator=g)


def feature_loss(logits, img_f, txt_f, labels, A, I, terms):
    parts = {"ce": lambda: F.cross_entropy(logits, labels, label_smoothing=0.1),
             "txt": lambda: 8 * (1 - F.cosine_similarity(txt_f, A, dim=1)).mean(),
             "img": lambda: 8 * (1 - F.cosine_similarity(img_f, I, dim=1)).mean()}
    return sum(parts[t]() for t in terms)


def oracle_feature_grads(terms):
    def make():
        c = tiny()
        A, I = anchors(c)
        leaf, taps = leaves(c.params), {}
        logits = O.forward(c.cfg, c.frozen, leaf, c.class_embedding, c.eot, c.images, taps)
        loss = feature_loss(logits, taps["image_features"], taps["text_features"], c.labels.long(), A, I, terms)
        loss.backward()
        return loss.item(), leaf_grads(leaf)
    return cached(("features", terms), make)


ALL = ("ce", "txt", "img")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_feature_terms_and_label_smoothing_against_the_oracle(dtype):
    c = tiny()
    A, I = (t.cuda() for t in anchors(c))
    labels = c.labels.cuda()
    m = TM.build(c, dtype)
    runs = {}
    for terms in (ALL, ("ce",), ("txt",), ("img",)):
        loss, _, got = custom_step(m, c.images, lambda o: feature_loss(o.logits, o.image_features, o.text_features, labels, A, I, terms))
        ref_loss, ref = oracle_feature_grads(terms)
        print(f"mudpt_tiny {dtype} {'+'.join(terms)}: loss {loss:.6f}, oracle {ref_loss:.6f}")
        if terms == ("ce",):  # a loss of the logits alone, held as the suites hold the cross-entropy; the feature terms are printed
            assert abs(loss - ref_loss) <= TINY_SLACK * LOGIT_ATOL[dtype]
        held(got, ref, dtype, f"mudpt_tiny {dtype} {'+'.join(terms)}", cos=True)
        runs[terms] = got
    total = {k: sum(runs[(t,)][k] for t in ALL) for k in c.keys}
    for k in c.keys:
        emax, erms, cos = grad_triple(total[k], runs[ALL][k])
        print(f"mudpt_tiny {dtype} {k}: sum of the three runs vs the combined run: max {emax:.3e} x rms, rms {erms:.3e} x rms")
    held(total, runs[ALL], dtype, f"mudpt_tiny {dtype} sum of the three runs vs the combined run", cos=True)  # by linearity, within the same bounds
    held(total, oracle_feature_grads(ALL)[1], dtype, f"mudpt_tiny {dtype} sum of the three runs", cos=True)
    m.close()


# ---- 3. accumulation and identity -----------------------------------------------------------------------------------------------------------
def test_backward_accumulates_into_the_same_bucket_views():
    c = tiny()
    labels = c.labels.cuda()
    m = TM.build(c, "fp16")
    ptrs = {k: p.grad.data_ptr() for k, p in m.named_parameters()}
    ce = lambda o: F.cross_entropy(o.logits, labels)  # noqa: E731
    other = lambda o: 3 * o.text_features.pow(2).mean() + F.cross_entropy(o.logits, labels.roll(1))  # noqa: E731
    _, _, g1 = custom_step(m, c.images, ce)
    _, _, g2 = custom_step(m, c.images, other)
    m.flat_grads.zero_()
    custom_step(m, c.images, ce, zero=False)
    _, _, both = custom_step(m, c.images, other, zero=False)
    for k in c.keys:
        assert torch.allclose(both[k], g1[k] + g2[k], rtol=1e-6, atol=0), k
        assert not torch.equal(g1[k], g2[k])
    assert {k: p.grad.data_ptr() for k, p in m.named_parameters()} == ptrs
    flat, base = m.flat_grads.cpu(), m.flat_grads.data_ptr()
    for k, p in m.named_parameters():  # flat_grads is what grads() shows
        off = (p.grad.data_ptr() - base) // 4
        assert 0 <= off <= flat.numel() - p.numel() and torch.equal(flat[off:off + p.numel()].view_as(both[k]), both[k]), k
    # under no_grad: the three tensors, nothing armed
    with torch.no_grad():
        out = m.differentiable(c.images)
    assert not out.logits.requires_grad and out.image_features.shape == (len(c.labels), c.cfg.embed_dim) and out.text_features.shape == (m.n_cls, c.cfg.embed_dim)
    feat = torch.empty_like(out.image_features)
    assert m.lib.mudpt_train_features(m._h, len(c.labels), capi.ptr(feat), None, None) == 3 and b"no mudpt_forward_train is in flight" in m.lib.mudpt_last_error()
    m.close()


# ---- 4. the other variants under a logits-only custom loss ------------------------------------------------------------------------------------------
def logit_loss(logits, labels):
    target = torch.softmax(0.5 * torch.roll(logits.detach(), 1, 1), dim=1)
    return F.cross_entropy(logits, labels, label_smoothing=0.1) + F.kl_div(F.log_softmax(logits, dim=1), target, reduction="batchmean")


def reference_logit_grads(name):
    """CPU autograd of logit_loss through the variant's restatement -> (loss, {key: grad}, taps)."""
    def make():
        c, taps = TK.load(name), {}
        if name.startswith("coop_"):
            leaf = leaves({CR.CTX: c.ctx})
            logits = CR.forward(c.cfg, c.frozen, leaf[CR.CTX], c.class_embedding, c.eot, c.name_lens, c.position, c.images, taps)
            taps["prompts"].retain_grad()
        elif name.startswith(("vpt_", "mpt_")):
            leaf = leaves(c.params)
            logits = VR.forward(c.cfg, c.frozen, leaf, c.trainer, c.shape, c.class_embedding, c.eot, c.images)
        else:
            leaf = leaves(c.params)
            logits = (UR if name.startswith("umudpt_") else UUR).forward(c.cfg, c.frozen, leaf, c.class_embedding, c.eot, c.images)
        loss = logit_loss(logits, c.labels.long())
        loss.backward()
        return loss.item(), leaf_grads(leaf), ({"dprompts": taps["prompts"].grad.detach()} if "prompts" in taps else {})
    return cached(("logits", name), make)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["coop_tiny_end", "coop_tiny_middle_csc", "vpt_tiny", "mpt_tiny", "umudpt_tiny", "uumudpt_tiny"])
def test_variants_under_a_logits_only_loss(name, dtype):
    c = TK.load(name)
    labels = c.labels.cuda()
    m = TK.build(name, dtype)
    loss, _, got = custom_step(m, c.images, lambda o: logit_loss(o.logits, labels))
    if name.startswith("vpt_"):
        # The text side has nothing to learn, and every VPT trainable is the vision tower's, so the bucket cannot show it: the library's own
        # count of text-tower passes and text-side head launches does.  A second step runs no text-side launch at all -- not the text tower
        # (its features are kept), not the head's text half in the backward -- also when the loss reads the text features.
        count = lambda: int(m.debug_read("text_launches", 1)[0].item())  # noqa: E731
        n0 = count()
        out = m.differentiable(c.images)
        n1 = count()
        (logit_loss(out.logits, labels) + out.text_features.pow(2).mean()).backward()
        torch.cuda.synchronize()
        assert n0 > 0 and n1 == n0 and count() == n0, (n0, n1, count())
        assert all(torch.equal(g, got[k] * 2) for k, g in host_grads(m).items())  # the text-feature term added nothing, the step accumulated
    m.close()
    ref_loss, ref, taps = reference_logit_grads(name)
    tag = f"{name} {dtype}"
    print(f"{tag}: loss {loss:.6f}, restatement {ref_loss:.6f}")
    if name.startswith("coop_"):  # tests/test_coop_gpu.py: the CSC rule, or the cancellation bound of the shared context from the restatement's own terms
        from tests import test_coop_gpu as TC
        g, r = got[CR.CTX], ref[CR.CTX]
        rms_g, gmax = r.pow(2).mean().sqrt().item(), r.abs().max().item()
        e, er = (g - r).abs().max().item(), (g - r).pow(2).mean().sqrt().item()
        if c.csc:
            print(f"{tag} CSC d ctx: rms err {er / rms_g:.3e} (bound {TC.GRAD_RMS[dtype]:.1e}) max err / rms {e / rms_g:.3e}")
            assert er <= TC.GRAD_RMS[dtype] * rms_g + 1e-12 and e <= 4 * TC.GRAD_RTOL[dtype] * rms_g + 1e-9
        else:
            bound = TC.DELTA_T[dtype] * TC.kappa(c, taps["dprompts"])
            print(f"{tag} d ctx: rms err {er / rms_g:.3e} (bound {bound:.3e}) max err / max {e / gmax:.3e}")
            assert er <= bound * rms_g + 1e-12 and e <= 4 * bound * gmax + 1e-9
        return
    held(got, ref, dtype, tag)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_resnet_coop_ignores_an_image_feature_gradient(dtype):
    """rn_coop_tiny: the logits-only loss against CPU autograd behind the restated tower's features, under tests/test_resnet_train_gpu.py's
    bounds (the suite's two plus three times the fixture's emulated tower term); a loss that also reads the image features changes no bit."""
    c = RT.case("rn_coop_tiny")
    labels = c.labels.cuda()

    def make():
        leaf = leaves(c.params)
        with torch.no_grad():
            feat = RT.R.image_features(c.rn, c.images, c.stages, c.heads, None)
        loss = logit_loss(RT.logits_from_features(c, feat, leaf), c.labels.long())
        loss.backward()
        return loss.item(), leaf_grads(leaf)
    ref_loss, ref = cached("rn_coop_tiny", make)
    m = TRT.build(c, dtype)
    loss, _, got = custom_step(m, c.images, lambda o: logit_loss(o.logits, labels))
    _, _, with_dimg = custom_step(m, c.images, lambda o: logit_loss(o.logits, labels) + 5 * o.image_features.pow(2).mean())
    m.close()
    assert all(torch.equal(with_dimg[k], got[k]) for k in got), "an image-feature gradient reached the bucket of a ResNet handle"
    for k in c.keys:
        r = ref[k]
        rms = r.pow(2).mean().sqrt().item()
        emu_max, emu_rms = c.emulated_grad[k][dtype]
        err, rel = (got[k] - r).abs().max().item() / rms, (got[k] - r).pow(2).mean().sqrt().item() / rms
        b_max, b_rms = 4 * GRAD_RTOL[dtype] + 3 * emu_max, GRAD_RMS[dtype] + 3 * emu_rms
        print(f"rn_coop_tiny {dtype} {k}: loss {loss:.5f} (restated {ref_loss:.5f}) max err / rms {err:.3e} (bound {b_max:.3e}), rms err / rms {rel:.3e} (bound {b_rms:.3e})")
        assert err <= b_max and rel <= b_rms, k


# ---- 5. state and refusals ------------------------------------------------------------------------------------------------------------------
def test_state_machine_and_refusals():
    c = tiny()
    labels = c.labels.cuda()
    fresh = TM.build(c, "fp16")
    want = TK.step(fresh, c.images, c.labels)
    fresh.close()
    m = TM.build(c, "fp16")
    lib, B = m.lib, len(c.labels)

    def still_steps(tag):
        TK.assert_same_step(TK.step(m, c.images, c.labels), want, tag)

    # a second backward through the same outputs
    out = m.differentiable(c.images)
    loss = F.cross_entropy(out.logits, labels)
    loss.backward(retain_graph=True)
    kept = m.flat_grads.clone()
    with pytest.raises(RuntimeError, match="one forward feeds one backward"):
        loss.backward()
    assert torch.equal(m.flat_grads, kept)
    still_steps("after a second backward")
    # an inference forward in between
    out = m.differentiable(c.images)
    m.eval()
    m(c.images)
    m.train()
    with pytest.raises(RuntimeError, match="one forward feeds one backward"):
        F.cross_entropy(out.logits, labels).backward()
    still_steps("after a backward behind another forward")
    # a second differentiable of the same batch size in between: the first call's outputs may not take the second forward's activations
    out = m.differentiable(c.images)
    newer = m.differentiable(c.images.flip(0))
    m.flat_grads.zero_()
    with pytest.raises(RuntimeError, match="a later forward has overwritten what that one left: one forward feeds one backward"):
        F.cross_entropy(out.logits, labels).backward()
    assert torch.count_nonzero(m.flat_grads) == 0
    F.cross_entropy(newer.logits, labels).backward()  # the forward in flight is still good for its own backward
    assert torch.count_nonzero(m.flat_grads) > 0
    still_steps("after a backward behind a later differentiable")
    # a no_grad differentiable in between arms nothing and ends what was armed
    out = m.differentiable(c.images)
    with torch.no_grad():
        other = m.differentiable(c.images.flip(0))
    with pytest.raises(RuntimeError, match="no mudpt_forward_train is in flight: one forward feeds one backward"):
        (F.cross_entropy(out.logits, labels) + other.logits.mean()).backward()
    still_steps("after a backward behind a no_grad differentiable")
    # a frozen weight set in between (here to the value it had): the setters end the forward in flight
    out = m.differentiable(c.images)
    m.set_weight("logit_scale", c.frozen["logit_scale"])
    with pytest.raises(RuntimeError, match="no mudpt_forward_train is in flight"):
        out.logits.sum().backward()
    still_steps("after a backward behind mudpt_set_weight")
    # a fused step in between
    out = m.differentiable(c.images)
    m.forward_backward(c.images, c.labels)
    with pytest.raises(RuntimeError, match="one forward feeds one backward"):
        out.logits.sum().backward()
    # the C level: another batch, no forward, every gradient null
    x = c.images.cuda().contiguous()
    logits, g = torch.empty(B, m.n_cls, device="cuda"), torch.zeros(B, m.n_cls, device="cuda")
    feat = torch.empty(B, c.cfg.embed_dim, device="cuda")
    assert lib.mudpt_train_features(m._h, B, capi.ptr(feat), None, None) == 3 and b"one forward feeds one backward" in lib.mudpt_last_error()
    assert lib.mudpt_forward_train(m._h, capi.ptr(x), B, capi.ptr(logits), None) == 0
    assert lib.mudpt_backward_logits(m._h, capi.ptr(g), None, None, B - 1, 1.0, None) == 3 and f"ran on {B} images, not {B - 1}".encode() in lib.mudpt_last_error()
    assert lib.mudpt_train_features(m._h, B - 1, capi.ptr(feat), None, None) == 3
    assert lib.mudpt_backward_logits(m._h, None, None, None, B, 1.0, None) == 1 and b"all null" in lib.mudpt_last_error()
    assert lib.mudpt_train_features(m._h, B, capi.ptr(feat), None, None) == 0  # none of the refusals ended the forward in flight
    assert lib.mudpt_backward_logits(m._h, capi.ptr(g), None, None, B, 1.0, None) == 0
    assert lib.mudpt_backward_logits(m._h, capi.ptr(g), None, None, B, 1.0, None) == 3
    torch.cuda.synchronize()
    assert torch.count_nonzero(m.flat_grads) == 0  # a zero logit gradient: a zeroed bucket
    still_steps("after the C-level refusals")
    m.close()


def test_cocoop_frozen_and_sharded_handles_are_refused():
    from tests import test_cocoop_gpu as TCC
    cc = GoldenCase("cocoop_tiny")
    m = TCC.build(cc.cfg, cc.frozen, cc.tokens, cc.params, "fp16", len(cc.labels))
    want = TK.step(m, cc.images, cc.labels)
    with pytest.raises(AssertionError, match="CoCoOp has no custom-loss step: its step is chunked over the images"):
        m.differentiable(cc.images)
    TK.assert_same_step(TK.step(m, cc.images, cc.labels), want, "cocoop_tiny after the refusal")
    m.close()

    from mudpt_amd.model import CustomCLIP, ModelShape
    from mudpt_amd.zsclip import FrozenCLIP
    c = tiny()
    shape = ModelShape.from_config(c.cfg, c.cfg.n_ctx, c.cfg.depth)
    f = FrozenCLIP(shape, c.frozen, c.tokens.int(), max_batch=len(c.labels), dtype="fp16")
    before = f(c.images).clone()
    x, z = c.images.cuda().contiguous(), torch.empty(len(c.labels), f.n_cls, device="cuda")
    assert f.lib.mudpt_forward_train(f._h, capi.ptr(x), len(c.labels), capi.ptr(z), None) == 1
    assert b"a frozen handle (mudpt_create_frozen) has no parameters: nothing to train with a custom loss" in f.lib.mudpt_last_error()
    assert not hasattr(f, "differentiable")  # a FrozenCLIP has no trainable: the Python face is CustomCLIP's alone
    assert torch.equal(f(c.images), before)
    f.close()

    s = CustomCLIP(shape, c.frozen, c.tokens, max_batch=len(c.labels), dtype="fp16", class_shard=(0, 6))
    s.set_params(c.params)
    with pytest.raises(AssertionError, match="class-sharded handle .* has no custom-loss step"):
        s.differentiable(c.images)
    s.close()


# ---- 6. the trainer hook ----------------------------------------------------------------------------------------------------------------------
def test_trainer_hook(tmp_path):
    from mudpt_amd import dassl_lite, trainer

    class SmoothedMuDPT(trainer.MuDPT):
        def compute_loss(self, out, label):
            return F.cross_entropy(out.logits, label, label_smoothing=0.1)

    def make(cls):
        cfg = dassl_lite.default_cfg()
        cfg.OUTPUT_DIR = str(tmp_path)
        cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.LR = 1, 0, 0.02
        cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 8, 4
        cfg.DATALOADER.TEST.BATCH_SIZE = 4
        cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH = 4, 12
        t = cls(cfg)
        t.batch_idx, t.num_batches = 0, 99
        return t

    t = make(SmoothedMuDPT)
    dtype = t.model.dtype_name
    batch = t.train_loader_x[0]
    image, label = t.parse_batch_train(batch)
    _, _, by_hand = custom_step(t.model, image, lambda o: t.compute_loss(o, label.to(o.logits.device)))
    start = t.model.flat_params.clone()
    first = t.forward_backward(batch)
    stepped = host_grads(t.model)
    for k, g in by_hand.items():
        emax, erms, cos = grad_triple(stepped[k], g)
        assert erms <= GRAD_RMS[dtype] and cos > GRAD_COS[dtype], (k, emax, erms, cos)
    second = t.forward_backward(batch)
    assert all(v == v and abs(v) != float("inf") for v in (first["loss"], second["loss"])) and second["loss"] < first["loss"]
    assert not torch.equal(t.model.flat_params, start)
    t.model.close()

    p = make(trainer.MuDPT)
    image, label = p.parse_batch_train(batch)
    p.model.forward_backward(image, label)
    today = host_grads(p.model)
    p.forward_backward(batch)
    now = host_grads(p.model)
    assert all(torch.equal(now[k], today[k]) for k in today), "the plugin without the hook no longer makes today's step"
    p.model.close()
