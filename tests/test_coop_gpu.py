"""GPU parity of the CoOp path (trainers/coop.py) through the C ABI: the HIP library with ``variant = "coop" / "coop_csc"`` against the
fixtures of the reference's own ``trainers.coop.CustomCLIP`` (tests/golden/gen_golden_coop.py) and the test-local restatement
(tests/coop_reference.py)."""
import ctypes as C

import pytest
import torch

from oracle import mudpt_oracle as O
from tests import coop_reference as R
from tests.helpers import assert_training_forward_is_the_inference_forward, check_logits, check_parity_mode_at_scale_100

pytestmark = pytest.mark.gpu

# Logit bounds of tests/test_cocoop_gpu.py (logit scale 14.29; the s100 fixture is the parity mode's, below).  The tiny shape (embed 128)
# takes that file's tiny-shape error model (test_larger_batch_against_oracle_and_sgd): a relative feature error eps moves the cosine of
# two e-dimensional unit vectors by ~eps / sqrt(e), so sqrt(512 / 128) = 2 x ViT-B/16's bound at equal eps, times its 1.5
# (measured here, fp16: max 1.9e-3, rms 7.8e-4; ViT-B/16 and ViT-B/32 fixtures: max <= 5.2e-4 against 1e-3).
LOGIT_RMS = {"fp16": 5e-4, "bf16": 1.6e-2}
LOGIT_ATOL = {"fp16": 1e-3, "bf16": 3.2e-2}


def slack_of(cfg):
    return 1.0 if cfg.v_layers >= 12 else (512 / cfg.embed_dim) ** 0.5 * 1.5
# Shared context: d ctx = sum_c T_c over the class prompts' context rows -- the cancellation error model of tests/test_cocoop_gpu.py
# (delta_T per term, kappa = ||sqrt(sum T^2)|| / ||sum T|| from the restatement's own terms).  CSC: every class's context gets ONE term,
# nothing cancels: MuDPT's per-tensor bound (tests/test_model_gpu.py GRAD_RTOL / GRAD_RMS).
DELTA_T = {"fp16": 4e-3, "bf16": 4e-2}
GRAD_RTOL = {"fp16": 2e-2, "bf16": 1.5e-1}
GRAD_RMS = {"fp16": 6e-3, "bf16": 6e-2}
PARITY = [f for f in R.FIXTURES if not f.endswith("_s100")]


def shape_of(cfg):
    from mudpt_amd.model import ModelShape
    return ModelShape.from_config(cfg, cfg.n_ctx, 1)


def build(case, dtype, ctx=None, csc=None, tokens=None, name_lens=None, max_batch=None, knobs=None):
    from mudpt_amd.model import CustomCLIP
    csc = case.csc if csc is None else csc
    m = CustomCLIP(shape_of(case.cfg), case.frozen, case.tokens if tokens is None else tokens, max_batch=max_batch or len(case.labels),
                   dtype=dtype, variant="coop_csc" if csc else "coop", knobs=knobs, class_token_position=case.position,
                   name_lens=case.name_lens if name_lens is None else name_lens)
    assert m.param_names == [R.CTX]
    m.set_params({R.CTX: case.ctx if ctx is None else ctx})
    return m


def kappa(case, dprompts):
    """Cancellation factor of the shared context's gradient from the per-class terms T_c = dprompts[c, ctx rows of c]."""
    T = torch.stack([dprompts[c, R.ctx_rows(case.cfg.n_ctx, case.name_lens[c], case.position)] for c in range(len(case.name_lens))]).double()
    return (T.pow(2).sum(0).sqrt().norm() / T.sum(0).norm()).item()


@pytest.fixture(scope="module", params=PARITY)
def case(request):
    return R.CoopCase(request.param)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_logits_loss_grads_match_reference(case, dtype):
    m = build(case, dtype)
    m.eval()
    logits = m(case.images).cpu()
    slack = check_logits(logits, case, dtype, f"{case.name} {dtype}", slack_of(case.cfg), LOGIT_RMS, LOGIT_ATOL)
    m.train()
    loss, logits2 = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    assert_training_forward_is_the_inference_forward(logits2, logits, dtype)
    assert abs(loss.item() - case.loss) <= slack * LOGIT_ATOL[dtype]
    got, ref = m.grads()[R.CTX].detach().cpu(), case.dctx
    rms_g, gmax = ref.pow(2).mean().sqrt().item(), ref.abs().max().item()
    e, er = (got - ref).abs().max().item(), (got - ref).pow(2).mean().sqrt().item()
    if case.csc:
        print(f"{case.name} {dtype} CSC d ctx: rms err {er / rms_g:.3e} (bound {GRAD_RMS[dtype]:.1e}) max err / rms {e / rms_g:.3e}")
        assert er <= GRAD_RMS[dtype] * rms_g + 1e-12 and e <= 4 * GRAD_RTOL[dtype] * rms_g + 1e-9
    else:
        taps = {}
        R.forward_backward(case.cfg, case.frozen, case.ctx, case.class_embedding, case.eot, case.name_lens, case.position, case.images,
                           case.labels, taps)
        bound = DELTA_T[dtype] * kappa(case, taps["dprompts"])
        print(f"{case.name} {dtype} d ctx: rms err {er / rms_g:.3e} (bound {bound:.3e}) max err / max {e / gmax:.3e}")
        assert er <= bound * rms_g + 1e-12 and e <= 4 * bound * gmax + 1e-9
    m.close()


def test_parity_mode_at_logit_scale_100():
    case = R.CoopCase("coop_vitb16_b2_s100")
    check_parity_mode_at_scale_100(build(case, "fp32"), case)


@pytest.mark.parametrize("name", [f for f in R.FIXTURES if f.startswith("coop_tiny_")] + ["coop_vitb16_b2_s100"])
def test_parity_mode_training_step(name):
    """One training step on a dtype "fp32" handle (what PREC "fp32" selects; every class-token position, shared and per-class contexts, and
    ViT-B/16 at logit scale 100).  Its forward is the inference forward bit for bit and its loss is the fixture's within the parity mode's
    logit bound; d ctx passes this suite's own check (the kappa bound, or the CSC rule) with the bf16 constants against both the fixture and
    the restatement, and inside that twice the figures this fixture measured (test_knobs_gpu.PARITY_STEP_MEASURED)."""
    from tests.helpers import check_parity_step_grads
    from tests.test_exact_gpu import LOGIT_ATOL_EXACT
    from tests.test_knobs_gpu import PARITY_STEP_MEASURED
    case = R.CoopCase(name)
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
    got = m.grads()[R.CTX].detach().cpu()
    m.close()
    taps = {}
    restated = R.forward_backward(case.cfg, case.frozen, case.ctx, case.class_embedding, case.eot, case.name_lens, case.position, case.images, case.labels, taps)[2]
    for tag, ref in (("fixture", case.dctx), ("restatement", restated)):
        rms_g, gmax = ref.pow(2).mean().sqrt().item(), ref.abs().max().item()
        e, er = (got - ref).abs().max().item(), (got - ref).pow(2).mean().sqrt().item()
        if case.csc:
            assert er <= GRAD_RMS["bf16"] * rms_g + 1e-12 and e <= 4 * GRAD_RTOL["bf16"] * rms_g + 1e-9, (tag, er / rms_g, e / rms_g)
        else:
            bound = DELTA_T["bf16"] * kappa(case, taps["dprompts"])
            assert er <= bound * rms_g + 1e-12 and e <= 4 * bound * gmax + 1e-9, (tag, er / rms_g, e / gmax, bound)
    check_parity_step_grads(name, [(R.CTX, got, restated)], PARITY_STEP_MEASURED[name])


def test_csc_with_equal_contexts_is_the_shared_context():
    case = R.CoopCase("coop_tiny_middle")
    shared = build(case, "fp16", csc=False)
    csc = build(case, "fp16", csc=True, ctx=case.ctx.unsqueeze(0).expand(len(case.classnames), -1, -1).contiguous())
    for m in (shared, csc):
        m.eval()
    assert torch.equal(shared(case.images), csc(case.images))
    shared.train(), csc.train()
    ls, gs = shared.forward_backward(case.images, case.labels)[None], shared.grads()[R.CTX].clone()
    lc, gc = csc.forward_backward(case.images, case.labels)[None], csc.grads()[R.CTX].clone()
    torch.cuda.synchronize()
    assert torch.equal(ls, lc)
    assert (gc.sum(0) - gs).abs().max().item() <= 1e-5 * gs.abs().max().item()
    shared.close(), csc.close()


@pytest.mark.parametrize("csc", [False, True])
def test_c208_length_buckets_change_nothing(csc):
    """208 mixed-length names, middle: 1 to 4 length buckets (txt_bucket_cost 0) give the same logits and loss bit for bit, the same CSC
    gradients bit for bit, and shared gradients within 2e-5 of their RMS (the context gradient is summed in the caller's class order)."""
    case = R.CoopCase("coop_vitb16_c208_middle_b2")
    g = torch.Generator().manual_seed(5)
    ctx = 0.02 * torch.randn(len(case.classnames), case.cfg.n_ctx, case.cfg.t_width, generator=g) if csc else case.ctx
    outs = []
    for nb in (1, 2, 3, 4):
        m = build(case, "bf16", ctx=ctx, csc=csc, knobs={"txt_buckets": nb, "txt_bucket_cost": 0})
        assert m.text_layout()[1] <= nb and (nb == 1 or m.text_layout()[1] > 1)
        loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
        torch.cuda.synchronize()
        outs.append((loss.item(), logits.cpu(), m.grads()[R.CTX].cpu().clone()))
        m.close()
    for loss, logits, grad in outs[1:]:
        assert loss == outs[0][0] and torch.equal(logits, outs[0][1])
        if csc:
            assert torch.equal(grad, outs[0][2])
        else:
            assert (grad - outs[0][2]).abs().max().item() <= 2e-5 * outs[0][2].pow(2).mean().sqrt().item()


@pytest.mark.parametrize("position", ["middle", "front"])
def test_class_permutation_permutes_logits_and_csc_rows(position):
    case = R.CoopCase("coop_vitb16_c208_middle_b2")
    case.position = position
    Cn = len(case.classnames)
    g = torch.Generator().manual_seed(6)
    ctx = 0.02 * torch.randn(Cn, case.cfg.n_ctx, case.cfg.t_width, generator=g)
    perm = torch.randperm(Cn, generator=g)
    res = []
    for p in (torch.arange(Cn), perm):
        m = build(case, "fp16", ctx=ctx[p].contiguous(), csc=True, tokens=case.tokens[p], name_lens=[case.name_lens[int(i)] for i in p])
        m.eval()
        logits = m(case.images).cpu()
        m.train()
        m.forward_backward(case.images, (p.argsort()[case.labels]))
        torch.cuda.synchronize()
        res.append((logits, m.grads()[R.CTX].cpu().clone()))
        m.close()
    assert torch.equal(res[1][0], res[0][0][:, perm])
    # Gradients: the head's softmax / log-sum-exp add over the classes in their order, so d(text features) moves by fp32 rounding, which
    # the fp16 backward can carry to one fp16 rounding of a token gradient (measured: 2.8e-5 of the largest element); a wrong row would
    # be off by the element itself
    assert (res[1][1] - res[0][1][perm]).abs().max().item() <= 1e-3 * res[0][1].abs().max().item()


def test_eval_text_reuse_is_bit_identical():
    case = R.CoopCase("coop_tiny_front_csc")
    m = build(case, "fp16", max_batch=4)
    m.eval()
    first = m(case.images)
    again = m(case.images)  # parameters unchanged: the text features of the first call are reused (MUDPT_FWD_REUSE_TEXT)
    m.invalidate_text_cache()
    fresh = m(case.images)
    assert torch.equal(first, again) and torch.equal(first, fresh)
    m.close()


@pytest.mark.parametrize("name", ["coop_tiny_front", "coop_tiny_middle_csc"])
def test_three_sgd_steps_track_the_restatement(name):
    case = R.CoopCase(name)
    m = build(case, "fp16")
    p, buf = case.ctx.clone(), None
    for step in range(3):
        loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
        ref_loss, ref_logits, ref = R.forward_backward(case.cfg, case.frozen, p, case.class_embedding, case.eot, case.name_lens, case.position,
                                                       case.images, case.labels)
        assert (logits.cpu() - ref_logits).abs().max().item() <= slack_of(case.cfg) * LOGIT_ATOL["fp16"], step
        assert abs(loss.item() - ref_loss.item()) <= 2e-3, step
        assert (m.grads()[R.CTX].cpu() - ref).pow(2).mean().sqrt().item() <= 2e-2 * ref.pow(2).mean().sqrt().item() + 1e-9, step
        m.sgd_step(0.05)
        p, buf = O.sgd_step(p, ref, buf, 0.05)
    torch.cuda.synchronize()
    # the three updates are sums of gradients each within 2e-2 (rms) of the restatement's: so is what they moved ctx by (measured 1.2e-3
    # of the largest move on the element, at lr 0.05 a move of 0.25)
    err, moved = m.prompt_learner.ctx.detach().cpu() - p, p - case.ctx
    assert err.pow(2).mean().sqrt().item() <= 2e-2 * moved.pow(2).mean().sqrt().item()
    assert err.abs().max().item() <= 2e-2 * moved.abs().max().item()
    m.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_dctx_kernel_is_reproducible_and_exact(dtype):
    """mudpt_coop_dctx on 1000 classes x 16 rows x 512 (the ImageNet shape): repeated calls are bit-identical; the shared sum equals a
    float64 sum to fp32 rounding; CSC rows are the scaled rows; the T stream (lp) path reads the same values."""
    from mudpt_amd import capi
    lib = capi.load()
    Cn, n, d, L = 1000, 16, 512, 40
    g = torch.Generator().manual_seed(9)
    dx = torch.randn(Cn * L, d, generator=g).cuda()
    rows = (torch.arange(Cn).view(Cn, 1) * L + 1 + torch.randperm(L - 2, generator=g)[:n].view(1, n)).to(torch.int32).cuda()
    lp = dx.to(torch.bfloat16 if dtype == 0 else torch.float16)
    for csc in (0, 1):
        outs = []
        for src32, srclp in ((dx, None), (None, lp), (dx, None)):
            out = torch.empty((Cn if csc else 1) * n * d, device="cuda")
            capi.check(lib.mudpt_coop_dctx(dtype, capi.ptr(src32), capi.ptr(srclp), capi.ptr(rows), capi.ptr(out), Cn, n, d, csc, 0.5, None), "coop_dctx")
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[2])
        for out, src in ((outs[0], dx), (outs[1], lp.float())):
            terms = src.cpu().double()[rows.cpu().long()]  # [C, n, d]
            ref = 0.5 * (terms if csc else terms.sum(0))
            assert (out.double().view_as(ref) - ref).abs().max().item() <= (0 if csc else 1e-5 * terms.abs().sum(0).max().item())


def test_coop_step_runs_no_vision_backward():
    """ViT-B/16, 24 images x 11 classes: the profiled step launches no vision-tower LayerNorm / attention backward (MuDPT: dozens)."""
    from mudpt_amd import synth
    from mudpt_amd.model import CustomCLIP, ModelShape
    B = 24
    g = torch.Generator().manual_seed(0)
    images, labels = torch.randn(B, 3, 224, 224, generator=g).cuda(), torch.randint(0, 11, (B,), generator=g).cuda()
    counts = {}
    for variant in ("coop", "mudpt"):
        shape = ModelShape(n_ctx=4, depth=12 if variant == "mudpt" else 1)
        tok = synth.bench_coop_prompts(4)[0] if variant == "coop" else synth.bench_tokenized_prompts()
        m = CustomCLIP(shape, synth.random_clip_state(shape, 0), tok, max_batch=B, dtype="bf16", seed=1, variant=variant)
        m.forward_backward(images, labels)
        m.profile(31)
        m.forward_backward(images, labels)
        cls, _ = m.profile_read_classes()
        m.profile(0)
        counts[variant] = (cls["ln_bwd"][2], cls["attn_bwd"][2], cls["ln_fwd"][2])
        m.close()
    print(counts)
    assert counts["coop"][0] == 0 and counts["coop"][1] == 0 and counts["coop"][2] > 0
    assert counts["mudpt"][0] > 0 and counts["mudpt"][1] > 0


def test_plugin_trains_checkpoints_and_evaluates(tmp_path):
    """trainers/coop.py's surface through dassl_lite: 2 synthetic epochs, the summary has loss and acc, the checkpoint holds ctx only, a
    fresh trainer reloads it and evaluates to the same logits."""
    from mudpt_amd import coop, dassl_lite  # noqa: F401  (registers CoOp)

    def cfg_for(out):
        cfg = dassl_lite.default_cfg()
        cfg.TRAINER.NAME = "CoOp"
        cfg.TRAINER.COOP.N_CTX, cfg.TRAINER.COOP.CSC, cfg.TRAINER.COOP.CLASS_TOKEN_POSITION = 4, True, "middle"
        cfg.OUTPUT_DIR = str(out)
        cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.LR = 2, 0, 0.02
        cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 8, 8
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 4, 4
        return cfg
    t = dassl_lite.build_trainer(cfg_for(tmp_path))
    assert type(t).__name__ == "CoOp" and t.get_model_names() == ["prompt_learner"]
    assert list(t.model.prompt_learner.state_dict()) == ["ctx"] and tuple(t.model.prompt_learner.ctx.shape) == (11, 4, 512)
    batch = t.train_loader_x[0]
    t.batch_idx, t.num_batches = 0, 99
    s = t.forward_backward(batch)
    assert set(s) == {"loss", "acc"} and 0.0 <= s["acc"] <= 100.0 and s["acc"] * 4 / 100 == round(s["acc"] * 4 / 100)
    t.train()
    ck = torch.load(str(tmp_path / "prompt_learner" / "model.pth.tar-2"), map_location="cpu")
    assert list(ck["state_dict"]) == ["ctx"]
    logits = t.model_inference(batch["img"].cuda())
    t2 = dassl_lite.build_trainer(cfg_for(tmp_path / "fresh"))
    t2.load_model(str(tmp_path), epoch=2)
    assert torch.equal(t2.model.prompt_learner.ctx.detach(), t.model.prompt_learner.ctx.detach())
    assert torch.equal(t2.model_inference(batch["img"].cuda()), logits)
    assert 0.0 <= t2.test() <= 100.0


def test_refusals():
    from mudpt_amd import capi
    from mudpt_amd.model import CustomCLIP
    lib = capi.load()
    case = R.CoopCase("coop_tiny_end")
    mud = CustomCLIP(shape_of(case.cfg), case.frozen, case.tokens, max_batch=3, dtype="fp16")  # a MuDPT handle (depth 1)
    assert lib.mudpt_set_class_token_position(mud._h, capi.CLASS_TOKEN_END, None) == 1
    mud.close()
    m = build(case, "fp16")
    assert lib.mudpt_set_class_shard(m._h, 0, 2) == 1 and b"CoOp" in lib.mudpt_last_error()
    f, df, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert lib.mudpt_cp_buffers(m._h, C.byref(f), C.byref(df), C.byref(n)) == 1
    # middle needs name lengths, and every class's context has to fit before its EOT row
    assert lib.mudpt_set_class_token_position(m._h, capi.CLASS_TOKEN_MIDDLE, None) == 1
    too_long = (C.c_int32 * len(case.classnames))(*([70] * len(case.classnames)))
    assert lib.mudpt_set_class_token_position(m._h, capi.CLASS_TOKEN_FRONT, too_long) == 0
    emb = case.class_embedding.contiguous()
    eot = case.eot.to(torch.int32).contiguous()
    assert lib.mudpt_set_class_prompts(m._h, capi.ptr(emb), capi.ptr(eot)) == 1 and b"EOT" in lib.mudpt_last_error()
    m.close()
