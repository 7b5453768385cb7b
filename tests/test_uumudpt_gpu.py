"""GPU parity of the UUMuDPT path (trainers/uumudpt.py, clip/model.py:600-664) through the C ABI: the HIP library with ``variant = "uumudpt"``
against the fixtures of the reference's own modules (tests/golden/gen_golden_uumudpt.py) and the test-local restatement
(tests/uumudpt_reference.py).  The cases are those of tests/test_umudpt_gpu.py, with the second direction beside the first.

Gradients are checked in the pieces that can each be bounded without a new number:
  (a) dG and dT -- the gradients of the two generators' outputs as the towers' backwards leave them -- and the four prompt tables' gradients
      (ctx, deep_prompts, visual_ctx, visual_ctx_deep_prompts) against the restatement with GRAD_RTOL / GRAD_RMS of tests/test_model_gpu.py:
      the same quantities as MuDPT's prompt-table gradients, which those constants already bound;
  (b) each generator's 18 gradients against the restatement's float64 generator backward fed the LIBRARY's own dG / dT, with the fp32 bound of
      the kernel tests (tests/test_promptgen_gpu.py: atol 3e-5 sqrt(4 d), rtol 1e-5 for a unit-variance input at generator width d; the
      backward is linear in its input, so atol scales with that input's rms): this isolates the generators from the towers' rounding;
  (c) all 40 against the fixture with GRAD_RTOL / GRAD_RMS, printed per tensor."""
import ctypes as C
import math

import pytest
import torch

from tests import uumudpt_reference as R
from tests.helpers import (assert_training_forward_is_the_inference_forward, check_fixture_grads, check_grad, check_logits,
                           check_parity_mode_at_scale_100, check_sampled_taps)
from tests.test_model_gpu import LOGIT_ATOL, TINY_SLACK

pytestmark = pytest.mark.gpu
PARITY = [f for f in R.FIXTURES if not f.endswith("_s100")]


def build(case, dtype, max_batch=None, knobs=None, params=None):
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape.from_config(case.cfg, case.cfg.n_ctx, case.cfg.depth)
    m = CustomCLIP(shape, case.frozen, case.tokens, ctx_token_ids=case.ctx_token_ids, max_batch=max_batch or len(case.labels), dtype=dtype,
                   variant="uumudpt", knobs=knobs, seed=case.seeds[1])
    assert m.param_names == case.keys and m.ctx_key == R.CTX
    m.set_params(case.params if params is None else params)
    return m


_CASES, _REF = {}, {}


def load(name):
    if name not in _CASES:
        _CASES[name] = R.UumudptCase(name)
    return _CASES[name]


def restated(case):
    """(loss, logits, grads, dG, dT) of the restatement on the fixture's inputs, computed once per fixture and left unchanged."""
    if case.name not in _REF:
        _REF[case.name] = R.forward_backward(case.cfg, case.frozen, case.params, case.class_embedding, case.eot, case.images, case.labels)
    return _REF[case.name]


def generator_bound(got, case, names, X, d_out, width, tag):
    """Piece (b): one generator's 18 gradients against its float64 backward fed the library's own output gradient."""
    scale = d_out.pow(2).mean().sqrt().item()
    atol, rtol = 3e-5 * math.sqrt(4 * width) * scale, 1e-5
    _, _, g64 = R.generator_backward(case.params, names, X, d_out)
    worst = (0.0, "")
    for k, r in g64.items():
        e = (got[k].double() - r).abs()
        worst = max(worst, ((e / (atol + rtol * r.abs())).max().item(), k))
    print(f"{tag} (b): input gradient rms {scale:.3e}; worst generator gradient {worst[1]} at {worst[0]:.3f} of the fp32 bound")
    assert len(g64) == 18 and worst[0] <= 1.0, worst


@pytest.fixture(scope="module", params=PARITY)
def case(request):
    return load(request.param)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_logits_loss_grads_taps_match_reference(case, dtype):
    B = len(case.labels)
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
    got = {k: v.detach().cpu().clone() for k, v in m.grads().items()}
    _, _, ref_grads, ref_dG, ref_dT = restated(case)
    c = case.cfg
    tag = f"{case.name} {dtype}"
    # the generators' outputs are fp32 whatever the towers' operand type
    G = m.debug_read("uumudpt.G", B).view(c.depth, c.n_ctx, c.v_width)
    with torch.no_grad():
        G_ref = R.generator(case.params, R.GEN1, R.prompt_tables(case.params))
        T_ref = R.generator(case.params, R.GEN2, case.params[R.VDEEP])
    assert (G - G_ref).abs().max().item() <= 3e-5 * math.sqrt(4 * c.t_width) + 1e-5 * G_ref.abs().max().item()
    # (a) the gradients the towers leave: their rounding, MuDPT's constants
    dG = m.debug_read("uumudpt.dG", B).view(c.depth, c.n_ctx, c.v_width)
    check_grad(dG, ref_dG, dtype, f"{tag} (a) dG")
    dT = None
    if c.depth > 1:
        T = m.debug_read("uumudpt.T", B).view(c.depth - 1, c.n_ctx, c.embed_dim)
        assert (T - T_ref).abs().max().item() <= 3e-5 * math.sqrt(4 * c.v_width) + 1e-5 * T_ref.abs().max().item()
        dT = m.debug_read("uumudpt.dT", B).view(c.depth - 1, c.n_ctx, c.embed_dim)
        check_grad(dT, ref_dT, dtype, f"{tag} (a) dT")
    for k in (R.CTX, R.DEEP, R.VCTX, R.VDEEP):
        if got[k].numel():
            check_grad(got[k], ref_grads[k], dtype, f"{tag} (a) {k}")
    # (b) each generator's own backward in fp32, fed the library's dG / dT
    generator_bound(got, case, R.GEN1, R.prompt_tables(case.params), dG, c.t_width, f"{tag} Gen1")
    if c.depth > 1:
        generator_bound(got, case, R.GEN2, case.params[R.VDEEP], dT, c.v_width, f"{tag} Gen2")
    else:  # Gen2 idles: its gradients are the zeroed bucket's zeros, as the reference's are
        assert all(torch.count_nonzero(got[k]) == 0 for k, _ in R.generator_keys(R.GEN2, c.v_width, c.embed_dim))
    # (c) all 40 against the fixture (the reference's own autograd)
    check_fixture_grads(got, case, dtype, f"{tag} (c)")
    m.close()


def test_parity_mode_at_logit_scale_100():
    case = load("uumudpt_vitb16_b2_s100")
    check_parity_mode_at_scale_100(build(case, "fp32"), case)


@pytest.mark.parametrize("name", ["uumudpt_tiny", "uumudpt_vitb16_b2_s100"])
def test_parity_mode_training_step(name):
    """One training step on a dtype "fp32" handle, in the pieces of test_logits_loss_grads_taps_match_reference: the forward is the inference
    forward bit for bit and the loss the fixture's within the parity mode's logit bound; (a) what the towers leave and (c) every tensor
    against the fixture with the bf16 constants (the mode runs lp_grad = 1); (b) the generators' own fp32 backward keeps its fp32 bound;
    inside (a) / (c), every tensor against the restatement within twice what this fixture measured (test_knobs_gpu.PARITY_STEP_MEASURED)."""
    from tests.helpers import check_parity_step_grads
    from tests.test_exact_gpu import LOGIT_ATOL_EXACT
    from tests.test_knobs_gpu import PARITY_STEP_MEASURED
    case = load(name)
    B, c = len(case.labels), case.cfg
    m = build(case, "fp32")
    m.eval()
    logits = m(case.images).cpu()
    m.train()
    loss, logits2 = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    assert_training_forward_is_the_inference_forward(logits2, logits, "fp32")
    slack = 1.0 if c.v_layers >= 12 else 3.0  # test_exact_gpu.py::test_logits_at_scale_100_within_1e_3: the tiny shape in the default parity mode
    print(f"{name} parity mode: |loss - reference| {abs(loss.item() - case.loss):.3e} |logit - reference| max {(logits - case.logits).abs().max().item():.3e}")
    assert abs(loss.item() - case.loss) <= slack * LOGIT_ATOL_EXACT
    got = {k: v.detach().cpu().clone() for k, v in m.grads().items()}
    tag = f"{name} fp32"
    _, _, ref_grads, ref_dG, ref_dT = restated(case)
    dG = m.debug_read("uumudpt.dG", B).view(c.depth, c.n_ctx, c.v_width)
    dT = m.debug_read("uumudpt.dT", B).view(c.depth - 1, c.n_ctx, c.embed_dim) if c.depth > 1 else None
    m.close()
    check_grad(dG, ref_dG, "bf16", f"{tag} (a) dG")
    if dT is not None:
        check_grad(dT, ref_dT, "bf16", f"{tag} (a) dT")
    for k in (R.CTX, R.DEEP, R.VCTX, R.VDEEP):
        if got[k].numel():
            check_grad(got[k], ref_grads[k], "bf16", f"{tag} (a) {k}")
    generator_bound(got, case, R.GEN1, R.prompt_tables(case.params), dG, c.t_width, f"{tag} Gen1")  # (b)
    if dT is not None:
        generator_bound(got, case, R.GEN2, case.params[R.VDEEP], dT, c.v_width, f"{tag} Gen2")
    check_fixture_grads(got, case, "bf16", f"{tag} (c)")
    check_parity_step_grads(name, [(k, got[k], ref_grads[k]) for k in case.keys], PARITY_STEP_MEASURED[name])


def test_unconsumed_layers_get_exactly_zero():
    """depth 5 over 3-layer towers: the vision tower never splices G[3], G[4], the text tower never deep_prompts[2:] + T[2:], so those rows of dG
    and dT are exactly zero; either generator's attention stays inside one layer, so its dX of those layers is exactly zero too, and with it
    the gradients of deep_prompts[2:] and visual_ctx_deep_prompts[2:] -- each the sum of a tower's zero and a generator's zero."""
    case = load("uumudpt_tiny_d5")
    for dtype in ("fp16", "fp32"):  # the parity mode's handle too: its backward reads other copies of the forward's buffers
        m = build(case, dtype)
        m.forward_backward(case.images, case.labels)
        c, B = case.cfg, len(case.labels)
        dG = m.debug_read("uumudpt.dG", B).view(c.depth, c.n_ctx, c.v_width)
        dT = m.debug_read("uumudpt.dT", B).view(c.depth - 1, c.n_ctx, c.embed_dim)
        assert torch.count_nonzero(dG[3:]) == 0 and torch.count_nonzero(dG[:3]) > 0, dtype
        assert torch.count_nonzero(dT[2:]) == 0 and torch.count_nonzero(dT[:2]) > 0, dtype
        ref = restated(case)[2]
        for k in (R.DEEP, R.VDEEP):
            g = m.grads()[k].cpu()
            assert torch.count_nonzero(g[2:]) == 0 and torch.count_nonzero(g[:2]) > 0, (k, dtype)
            assert torch.count_nonzero(ref[k][2:]) == 0
        m.close()


def test_depth_one_lists_empty_tensors_and_idles_gen2():
    case = load("uumudpt_tiny_d1")
    m = build(case, "fp16")
    sd = m.state_dict()
    c = case.cfg
    assert len(sd) == 40 and list(sd) == case.keys
    assert tuple(sd[R.DEEP].shape) == (0, 3, c.t_width) and tuple(sd[R.VDEEP].shape) == (0, 3, c.v_width)
    loss = m.forward_backward(case.images, case.labels)
    assert abs(loss.item() - case.loss) <= TINY_SLACK * LOGIT_ATOL["fp16"]
    g = m.grads()
    assert all(torch.count_nonzero(g[k]) == 0 for k, _ in R.generator_keys(R.GEN2, c.v_width, c.embed_dim))
    assert torch.count_nonzero(g[R.VCTX]) > 0 and all(torch.count_nonzero(g[k]) > 0 for k, _ in R.generator_keys(R.GEN1, c.t_width, c.v_width))
    m.close()


def test_init_is_the_references_draw():
    """The module's own initial values (seed = the fixture's) carry the checksums of the reference's freshly constructed modules, each half
    behind its own seed point."""
    case = load("uumudpt_tiny")
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape.from_config(case.cfg, case.cfg.n_ctx, case.cfg.depth)
    m = CustomCLIP(shape, case.frozen, case.tokens, ctx_token_ids=case.ctx_token_ids, max_batch=3, dtype="fp16", variant="uumudpt", seed=case.seeds[1])
    for k, v in m.state_dict().items():
        got = [v.double().sum().item(), v.double().abs().sum().item()]
        assert got == pytest.approx(case.init_checksums[k], rel=1e-12, abs=1e-12), k
    m.close()


@pytest.mark.parametrize("name", ["uumudpt_tiny", "uumudpt_vitb16_b2"])
def test_two_identical_steps_give_bit_identical_grads(name):
    case = load(name)
    m = build(case, "bf16")
    m.forward_backward(case.images, case.labels)
    g1 = m.flat_grads.clone()
    m.forward_backward(case.images, case.labels)
    assert torch.equal(g1.view(torch.int32), m.flat_grads.view(torch.int32))
    assert all(g.abs().sum().item() > 0 for g in m.grads().values())
    m.close()


def test_eval_cache_holds_text_features_G_and_the_deep_sums():
    """An eval forward that reuses the cached text features, G and the vision deep sum equals a recomputed one bit for bit and launches no
    text-tower pass; after an SGD step that moves ONLY visual_ctx_text_proj.bias -- which reaches the logits through T alone -- or ONLY
    visual_proj.bias -- through G alone -- the cache is not reused.  The steps' directions are seeded random ones: a UNIFORM shift of such a
    bias adds one constant to every feature of every prompt row, which the towers' LayerNorms remove."""
    case = load("uumudpt_tiny")
    m = build(case, "fp16")
    count = lambda: int(m.debug_read("text_launches", 1)[0].item())  # noqa: E731
    m.eval()
    a = m(case.images).clone()
    n0 = count()
    b = m(case.images).clone()  # the reuse path
    assert count() == n0 and torch.equal(a, b)
    m.invalidate_text_cache()
    c = m(case.images).clone()  # recomputed
    assert count() > n0 and torch.equal(a, c)
    last, start = a, {k: v.clone() for k, v in case.params.items()}
    for key in (R.V + "_text_proj.bias", R.P + "visual_proj.bias"):  # zero gradients but its own, plain SGD
        m.flat_grads.zero_()
        bias = dict(m.named_parameters())[key]
        direction = torch.randn(bias.numel(), generator=torch.Generator().manual_seed(3))
        bias.grad.copy_(direction)
        before = m.flat_params.clone()
        m.sgd_step(0.05, momentum=0.0, weight_decay=0.0)
        moved = (m.flat_params - before).ne(0)
        start[key] = start[key] - 0.05 * direction
        assert int(moved.sum()) == bias.numel() and torch.allclose(bias.detach().cpu(), start[key], rtol=0, atol=1e-7)
        d = m(case.images).clone()
        assert not torch.equal(last, d), key
        fresh = build(case, "fp16", params={k: v.detach().cpu().clone() for k, v in m.named_parameters()})
        fresh.eval()
        assert torch.equal(fresh(case.images), d)
        fresh.close()
        last = d
    m.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_six_sgd_steps_track_the_restatement(dtype):
    """Six momentum-SGD steps on uumudpt_tiny, the library's step against the restatement plus torch.optim.SGD from the same start: the
    loss sequences agree step by step to the bound of tests/test_model_gpu.py::test_training_trajectory_tracks_the_oracle, and the
    parameters stay together.

    lr is 0.01, not that test's 0.05.  With 40 trained tensors the restatement's OWN trajectory overshoots at 0.05 (losses 1.605, 1.144,
    1.246, 1.230, 1.058, 0.908) and is then no yardstick for the 5e-3 bound: the restatement against itself, with seeded noise of GRAD_RMS's
    size (6e-3 of each gradient's rms, the error the fp16 gradients are allowed) added to its gradients, moves its fourth loss by up to
    6.7e-3 (four seeds, torch CPU).  At 0.01 the trajectory is monotone (1.605, 1.276, 1.108, 0.988, 0.883, 0.819: it trains by 0.79) and the
    same noise moves no loss by more than 2.6e-4, so the bound has room for rounding and none for a wrong gradient."""
    case = load("uumudpt_tiny")
    lr, steps = 0.01, 6
    m = build(case, dtype)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in case.params.items()}
    opt = torch.optim.SGD(list(leaves.values()), lr=lr, momentum=0.9, weight_decay=5e-4)
    ref_losses, got_losses = [], []
    for _ in range(steps):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(R.forward(case.cfg, case.frozen, leaves, case.class_embedding, case.eot, case.images), case.labels.long())
        loss.backward()
        opt.step()
        ref_losses.append(loss.item())
        got_losses.append(m.forward_backward(case.images, case.labels).item())
        m.sgd_step(lr, momentum=0.9, weight_decay=5e-4)
    torch.cuda.synchronize()
    print(f"{dtype} losses: restatement {['%.4f' % v for v in ref_losses]}  library {['%.4f' % v for v in got_losses]}")
    assert ref_losses[-1] < ref_losses[0] - 0.05, "the trajectory must actually train"
    tol = {"fp16": 5e-3, "bf16": 3e-2}[dtype]
    for a, b in zip(ref_losses, got_losses):
        assert abs(a - b) <= tol * max(1.0, abs(a)), (ref_losses, got_losses)
    flat = torch.cat([leaves[k].detach().reshape(-1) for k in case.keys])
    start = torch.cat([case.params[k].reshape(-1) for k in case.keys])
    moved = (flat - start).pow(2).mean().sqrt().item()
    err = (m.flat_params.cpu() - flat).pow(2).mean().sqrt().item()
    print(f"{dtype}: parameters moved {moved:.3e} rms, library - restatement {err:.3e} rms")
    assert err <= {"fp16": 2e-2, "bf16": 1.5e-1}[dtype] * moved
    m.close()


def test_refusals():
    from mudpt_amd import capi
    lib = capi.load()
    m = build(load("uumudpt_tiny"), "fp16")
    assert lib.mudpt_set_class_shard(m._h, 0, 2) == 1 and b"UMuDPT" in lib.mudpt_last_error()
    f, df, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert lib.mudpt_cp_buffers(m._h, C.byref(f), C.byref(df), C.byref(n)) == 1
    assert lib.mudpt_cp_backward(m._h, capi.CP_TEXT, None) == 1
    assert lib.mudpt_set_class_token_position(m._h, capi.CLASS_TOKEN_END, None) == 1
    with pytest.raises(AssertionError, match="unknown tensor"):
        m.debug_read("umudpt.G", 1)  # UMuDPT's name belongs to UMuDPT handles
    m.close()


def test_plugin_trains_checkpoints_and_reloads(tmp_path):
    """What ``python -m mudpt_amd.harness --trainer UUMuDPT --epochs 1 --batch 4`` runs (harness.run is main's body): it trains, writes a
    checkpoint with the 40 reference keys, and the checkpoint reloads into a fresh trainer with equal logits."""
    import dataclasses

    from oracle import mudpt_oracle as O
    from mudpt_amd import harness
    argv = ["--trainer", "UUMuDPT", "--epochs", "1", "--batch", "4", "--train-images", "8"]
    t = harness.run(argv + ["--output-dir", str(tmp_path)])
    assert type(t).__name__ == "UUMuDPT" and t.get_model_names() == ["UnifiedMultimodalDeepPromptTuning"] and 0.0 <= t.result <= 100.0
    keys = [k for k, _ in R.trainable_keys(dataclasses.replace(O.VIT_B16, n_ctx=4, depth=12))]  # the harness's --n-ctx / --depth defaults
    assert list(t.model.state_dict()) == keys and len(keys) == 40
    ck = torch.load(str(tmp_path / "UnifiedMultimodalDeepPromptTuning" / "model.pth.tar-1"), map_location="cpu")
    assert list(ck["state_dict"]) == keys
    held = {id(p) for g in t.optim.param_groups for p in g["params"]}
    assert held == {id(p) for p in t.model.parameters()} and len(held) == 40
    batch = t.test_loader[0]
    logits = t.model_inference(batch["img"].cuda())
    t2 = harness.run(argv + ["--output-dir", str(tmp_path / "fresh"), "--eval-only", "--model-dir", str(tmp_path), "--load-epoch", "1"])
    assert torch.equal(t2.model.flat_params, t.model.flat_params)
    assert torch.equal(t2.model_inference(batch["img"].cuda()), logits)
    assert t2.result == t.result
