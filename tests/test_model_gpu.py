"""End-to-end GPU parity: the HIP path (through the C ABI) against the golden vectors produced by the
reference modules and against the CPU oracle on the same seeded inputs."""
import pytest
import torch

from oracle import mudpt_oracle as O
from tests.helpers import GRAD_COS, GRAD_RMS, GRAD_RTOL, LOGIT_ATOL, LOGIT_RMS, TINY_SLACK, GoldenCase, check_logits  # noqa: F401  (the bounds: the variants' suites import them from here)

pytestmark = pytest.mark.gpu


def build(case: GoldenCase, dtype: str, max_batch=None, knobs=None):
    from mudpt_amd.model import CustomCLIP, ModelShape
    c = case.cfg
    shape = ModelShape.from_config(c, c.n_ctx, c.depth)
    m = CustomCLIP(shape, case.frozen, case.tokens, max_batch=max_batch or len(case.labels), dtype=dtype, knobs=knobs)
    m.set_params(case.params)
    return m


@pytest.fixture(scope="module", params=["mudpt_tiny", "mudpt_vitb16_b4", "mudpt_vitl14_336_b1", "mudpt_vitb16_n2_d9_b2"])  # the last: n_ctx 2, depth 9 -- what the reference's scripts train
def case(request):
    return GoldenCase(request.param)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_logits_match_reference(case, dtype):
    m = build(case, dtype)
    check_logits(m(case.images), case, dtype, dtype)
    m.close()


def test_block_outputs_match_reference_fp16():
    """Residual stream after blocks 0, 1 and the last one of each tower vs the reference's own activations."""
    case = GoldenCase("mudpt_vitb16_b4")
    m = build(case, "fp16")
    m(case.images)
    B, n = len(case.labels), case.cfg.n_ctx
    for tower, pre, layers, nseq in (("vis", "visual.transformer", case.cfg.v_layers, B), ("txt", "transformer", case.cfg.t_layers, 11)):
        width = case.cfg.v_width if tower == "vis" else case.cfg.t_width
        for i in (0, 1, layers - 1):
            ref = torch.from_numpy(case.z[f"tap.{pre}.resblocks.{i}.out"])  # [:, ::8, ::16] sample of [nseq, L, d]
            if i + 1 == layers:
                # The last block's output exists only on the row the model uses (CLS token / EOT token): its tail runs on
                # those rows alone.  The reference sample holds rows 0, 8, 16, ...: every CLS row, and the EOT row of the
                # class prompts whose EOT position is a multiple of 8.
                got = m.debug_read(f"{tower}.x_out", B).view(nseq, width)[:, ::16]
                pos = torch.zeros(nseq, dtype=torch.long) if tower == "vis" else case.eot
                seqs = torch.nonzero(pos % 8 == 0).flatten()
                assert len(seqs) > 0
                want = ref[seqs, pos[seqs] // 8]
                rel = (got[seqs] - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()
                print(f"{tower}.x_out ({len(seqs)} rows): relative rms error {rel:.3e}")
                assert rel < 1.5e-3, (tower, rel)
                continue
            name = f"{tower}.x_in.{i + 1}"
            got = m.debug_read(name, B).view(nseq, -1, width)
            L = got.shape[1]
            rows = torch.arange(0, L, 8)
            got = got[:, ::8, ::16]
            ref = ref[:, :len(rows)]  # the text tower runs on positions 0..max(eot) only (causal: later rows are never used)
            # x_in.{i+1} already carries block i+1's spliced prompt rows: compare the other rows only
            keep = (rows < L - n) if tower == "vis" else ((rows == 0) | (rows > n))
            rel = (got[:, keep] - ref[:, keep]).pow(2).mean().sqrt() / ref[:, keep].pow(2).mean().sqrt()
            print(f"{name}: relative rms error {rel:.3e}")
            assert rel < 1.5e-3, (name, rel)
    m.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_loss_and_grads_match_reference(case, dtype):
    m = build(case, dtype)
    loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    slack = TINY_SLACK if case.cfg.v_layers < 12 else 1.0
    assert abs(loss.item() - case.loss) <= slack * LOGIT_ATOL[dtype]
    assert (logits.cpu() - case.logits).abs().max().item() <= slack * LOGIT_ATOL[dtype]
    _, _, ref = O.forward_backward(case.cfg, case.frozen, case.params, case.class_embedding, case.eot, case.images, case.labels)
    got = {k: v.detach().cpu() for k, v in m.grads().items()}
    for k in O.TRAINABLE_ORDER:
        r, g = ref[k], got[k]
        rms = r.pow(2).mean().sqrt().item()
        err = (g - r).abs().max().item()
        rel_rms = (g - r).pow(2).mean().sqrt().item() / max(rms, 1e-30)
        print(f"{dtype} {k}: rms {rms:.3e} max err {err:.3e} rms err {rel_rms:.3e} x rms")
        assert err <= GRAD_RTOL[dtype] * rms * 4 + 1e-9, (k, err, rms)
        assert rel_rms <= GRAD_RMS[dtype] or rms == 0, (k, rel_rms)
        # direction: cosine similarity of the whole tensor
        cos = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
        assert cos > GRAD_COS[dtype], (k, cos)
        # the fixture itself (reference autograd) agrees with the oracle, checked on CPU in test_oracle_golden
        full = case.grad(k)
        if full is not None:
            assert (g - full).abs().max().item() <= GRAD_RTOL[dtype] * rms * 4 + 1e-9
    m.close()


def test_unused_deep_prompts_get_zero_grad():
    """depth - 1 > layers - 1: surplus deep prompts are never consumed -> zero gradient."""
    case = GoldenCase("mudpt_tiny")
    import dataclasses
    cfg = dataclasses.replace(case.cfg, depth=6)  # 3 layers -> only deep[0], deep[1] are used
    params = O.make_trainable_state(cfg, 5, case.frozen, [int(v) for v in case.z["ctx_token_ids"]])
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape.from_config(cfg, cfg.n_ctx, cfg.depth)
    m = CustomCLIP(shape, case.frozen, case.tokens, max_batch=3, dtype="fp16")
    m.set_params(params)
    loss = m.forward_backward(case.images, case.labels)
    _, logits_ref, ref = O.forward_backward(cfg, case.frozen, params, case.class_embedding, case.eot, case.images, case.labels)
    g = m.grads()["mudpt_prompt_learner.deep_prompts"].cpu()
    assert torch.count_nonzero(g[2:]) == 0 and torch.count_nonzero(ref["mudpt_prompt_learner.deep_prompts"][2:]) == 0
    assert torch.count_nonzero(g[:2]) > 0
    r = ref["image_encoder.visual_ctx_deep_prompts"]
    assert (m.grads()["image_encoder.visual_ctx_deep_prompts"].cpu() - r).abs().max() <= 0.1 * r.pow(2).mean().sqrt() + 1e-9
    m.close()


@pytest.mark.parametrize("nesterov,dampening", [(False, 0.0), (True, 0.0), (False, 0.1)])
def test_sgd_step_matches_torch(nesterov, dampening):
    """The library's fused SGD over two steps against the oracle's torch.optim.SGD restatement (itself held to torch.optim.SGD on CPU,
    tests/test_oracle_golden.py), incl. the nesterov and dampening variants Dassl's build_optimizer can configure."""
    case = GoldenCase("mudpt_tiny")
    m = build(case, "fp16")
    buf = None
    for _ in range(2):
        p0 = m.flat_params.clone()
        m.forward_backward(case.images, case.labels)
        g0 = m.flat_grads.clone()
        m.sgd_step(lr=0.0025, momentum=0.9, weight_decay=5e-4, dampening=dampening, nesterov=nesterov)
        ref, buf = O.sgd_step(p0.cpu(), g0.cpu(), buf, 0.0025, 0.9, 5e-4, dampening, nesterov)
        torch.testing.assert_close(m.flat_params.cpu(), ref, atol=1e-7, rtol=1e-6)
    m.close()


def test_not_ready_fails_loudly():
    from mudpt_amd import capi
    import ctypes as C
    lib = capi.load()
    cfg = capi.Config(32, 16, 192, 3, 3, 128, 3, 2, 77, 128, 2, 2, 11, 2, 1)
    h = C.c_void_p()
    assert lib.mudpt_create(C.byref(cfg), C.byref(h)) == 0
    x = torch.zeros(2, 3, 32, 32, device="cuda")
    out = torch.zeros(2, 11, device="cuda")
    rc = lib.mudpt_forward(h, C.c_void_p(x.data_ptr()), 2, C.c_void_p(out.data_ptr()), None)
    assert rc == 3 and b"frozen weights unset" in lib.mudpt_last_error()
    lib.mudpt_destroy(h)
    bad = capi.Config(32, 16, 192, 3, 3, 128, 3, 2, 77, 128, 2, 0, 11, 2, 1)  # depth 0: trainers/mudpt.py:52 assert
    assert lib.mudpt_create(C.byref(bad), C.byref(h)) == 1 and b"PROMPT_DEPTH" in lib.mudpt_last_error()


def test_eval_reuses_text_features_until_parameters_change():
    """model_inference: the text tower runs once per parameter version in eval mode, same logits."""
    case = GoldenCase("mudpt_tiny")
    m = build(case, "fp16")
    m.eval()
    a = m(case.images).clone()
    assert m._text_version == m.flat_params._version
    b = m(case.images).clone()            # reuse path
    assert torch.equal(a, b)
    with torch.no_grad():
        m.mudpt_prompt_learner.ctx.add_(0.05)   # in-place update bumps the bucket's version -> text tower reruns
    c = m(case.images).clone()
    assert not torch.equal(a, c)
    params = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    with torch.no_grad():
        ref = O.forward(case.cfg, case.frozen, params, case.class_embedding, case.eot, case.images)
    assert (c.cpu() - ref).abs().max().item() < 2e-3
    m.train()
    d = m(case.images)                      # training mode never reuses
    assert torch.equal(c, d)
    m.close()


def test_text_tower_trim_changes_nothing():
    """The text tower runs on positions 0..max(eot) of the 77 (causal mask + EOT readout: later positions are never used).
    Logits, loss and all ten gradients must equal the full-length run up to the summation order inside attention."""
    from mudpt_amd import capi
    case = GoldenCase("mudpt_vitb16_b4")
    lib = capi.load()
    out = {}
    for trim in (1, 0):
        m = build(case, "fp16", knobs={"txt_trim": trim})
        L = m.debug_read("txt.x_in.1", len(case.labels)).numel() // (11 * case.cfg.t_width)
        assert L == (int(case.eot.max()) + 1 if trim else case.cfg.ctx_len)
        loss = m.forward_backward(case.images, case.labels)
        out[trim] = (m(case.images).cpu(), loss.item(), {k: g.detach().cpu().clone() for k, g in m.grads().items()})
        m.close()
    torch.testing.assert_close(out[1][0], out[0][0], atol=2e-5, rtol=0)
    assert abs(out[1][1] - out[0][1]) < 1e-6
    for k, g in out[0][2].items():
        scale = g.pow(2).mean().sqrt().item()
        torch.testing.assert_close(out[1][2][k], g, atol=1e-4 * scale + 1e-12, rtol=0, msg=k)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_last_block_single_query_path_equals_the_general_kernels(dtype):
    """The last block runs single-query attention (one CLS / EOT query per sequence, K / V projections only, dX GEMM over the k, v
    thirds + the selected rows' dq share).  Knob last_single = 0 runs the general kernels on all rows instead: same logits and
    gradients up to T-precision rounding of differently ordered sums."""
    case = GoldenCase("mudpt_vitb16_b4")
    out = {}
    for single in (1, 0):
        m = build(case, dtype, knobs={"last_single": single})
        loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
        torch.cuda.synchronize()
        out[single] = (logits.cpu(), loss.item(), {k: g.detach().cpu().clone() for k, g in m.grads().items()})
        m.close()
    tol = {"fp16": 2e-4, "bf16": 6e-3}[dtype]
    assert (out[1][0] - out[0][0]).abs().max().item() <= tol
    for k, g in out[0][2].items():
        rms = g.pow(2).mean().sqrt().item()
        assert (out[1][2][k] - g).pow(2).mean().sqrt().item() <= {"fp16": 5e-3, "bf16": 6e-2}[dtype] * rms + 1e-12, k


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_training_trajectory_tracks_the_oracle(dtype):
    """Six momentum-SGD steps (forward, cross-entropy, backward, the library's SGD: trainers/mudpt.py:249-251 with Dassl's optimizer
    defaults) on the tiny shape with a learning rate large enough to move the loss, against the CPU oracle taking the same six steps
    from the same start: the loss sequences agree step by step and the parameters stay together (errors do not compound beyond the
    per-step gradient noise)."""
    case = GoldenCase("mudpt_tiny")
    lr, steps = 0.05, 6
    m = build(case, dtype)
    flat = O.flatten(case.params).clone()
    buf, ref_losses, got_losses = None, [], []
    for _ in range(steps):
        loss, _, grads = O.forward_backward(case.cfg, case.frozen, O.unflatten(flat, case.cfg), case.class_embedding, case.eot, case.images, case.labels)
        ref_losses.append(loss.item())
        flat, buf = O.sgd_step(flat, O.flatten(grads), buf, lr)
        got_losses.append(m.forward_backward(case.images, case.labels).item())
        m.sgd_step(lr, momentum=0.9, weight_decay=5e-4)
    torch.cuda.synchronize()
    print(f"{dtype} losses: oracle {['%.4f' % v for v in ref_losses]}  library {['%.4f' % v for v in got_losses]}")
    assert ref_losses[-1] < ref_losses[0] - 0.05, "the trajectory must actually train"
    # lr is 20x the reference's so that six steps move the loss by 1.6: a step amplifies the gradient's rounding noise accordingly
    # (measured: fp16 <= 3.1e-3 on the third step, where the loss falls fastest; bf16 <= 8e-3; fp32 <= 1.8e-3)
    # (the parity mode, dtype "fp32": an fp16-typed step with lp_grad = 1 -- the fp16 row)
    tol = {"fp16": 5e-3, "bf16": 3e-2, "fp32": 5e-3}[dtype]
    for a, b in zip(ref_losses, got_losses):
        assert abs(a - b) <= tol * max(1.0, abs(a)), (ref_losses, got_losses)
    moved = (flat - O.flatten(case.params)).pow(2).mean().sqrt().item()
    err = (m.flat_params.cpu() - flat).pow(2).mean().sqrt().item()
    print(f"{dtype}: parameters moved {moved:.3e} rms, library - oracle {err:.3e} rms")
    # fp32 (the parity mode): capped by the bf16 row, and inside it twice what it measures -- 2.1e-3 of the movement (2.23e-5 against 1.082e-2)
    assert err <= {"fp16": 2e-2, "bf16": 1.5e-1, "fp32": min(1.5e-1, 2 * 2.1e-3)}[dtype] * moved
    m.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_eval_logits_do_not_depend_on_the_test_batch_size(dtype):
    """Inference forwards never split K: the logits of an image are bit-identical whether it arrives in a batch of 4, 2 or 1 --
    a last, partial test batch gives the same numbers as a full one.  (A TRAINING forward of <= 8 ViT-B images may split out_proj / c_proj:
    test_split_k_agrees_with_the_sequential_contraction.)"""
    case = GoldenCase("mudpt_vitb16_b4")
    m = build(case, dtype)
    m.eval()
    full = m(case.images).cpu()
    for n in (2, 1):
        assert torch.equal(m(case.images[:n]).cpu(), full[:n]), n
    m.train()
    _, train_logits = m.forward_backward(case.images, case.labels, return_logits=True)
    assert not torch.equal(train_logits.cpu(), full)  # this shape's training forward does split (156 tiles): the knob is what differs
    m.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_split_k_agrees_with_the_sequential_contraction(dtype):
    """B = 4 ViT-B/16 (M = 804 rows): the vision tower's long-K store GEMMs (backward dfc K 3072, dqkv K 2304; forward c_proj K 3072 while the
    grid is at most 320 tiles of 64 x 64, i.e. up to 8 images) split K over up to four slices whose fp32 partials are summed in slice order
    (gemm.hip split_k_slices: whether and how a shape splits depends on M and on the CU count, so results are bit-reproducible for a fixed
    shape and device only; the text tower never splits).  Knob split_k = 0 contracts sequentially everywhere, fwd_split_k = 0 on the
    forward only: with the latter logits and loss are BIT-identical to the sequential run; with the forward split they agree to the
    rounding of a differently associated fp32 sum; gradients agree far inside the bound both hold against the reference."""
    case = GoldenCase("mudpt_vitb16_b4")
    out = {}
    for key, kn in (("split", {}), ("bwd_only", {"fwd_split_k": 0}), ("none", {"split_k": 0})):
        m = build(case, dtype, knobs=kn)
        loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
        torch.cuda.synchronize()
        out[key] = (logits.cpu(), loss.item(), {k: g.detach().cpu().clone() for k, g in m.grads().items()})
        m.close()
    assert torch.equal(out["bwd_only"][0], out["none"][0]) and out["bwd_only"][1] == out["none"][1]
    assert not torch.equal(out["split"][0], out["none"][0]), "c_proj of this case is expected to split on the forward (156 tiles)"
    # a differently associated fp32 sum flips the T rounding of ~1 % of c_proj's outputs per block: measured 2.8e-4 (fp16) on these logits,
    # a fraction of the mode's whole rounding noise (LOGIT_ATOL)
    assert (out["split"][0] - out["none"][0]).abs().max().item() <= (6e-4 if dtype == "fp16" else 8e-3)
    out = {1: out["split"], 0: out["none"]}
    differs = False
    for k, g in out[0][2].items():
        rms = g.pow(2).mean().sqrt().item()
        d = (out[1][2][k] - g)
        differs |= bool(d.abs().max().item() > 0)
        assert d.pow(2).mean().sqrt().item() <= GRAD_RMS[dtype] * rms + 1e-12, k
        assert d.abs().max().item() <= GRAD_RTOL[dtype] * rms * 4 + 1e-9, k
    assert differs, "the shapes of this case are expected to split (M = 804: 84 workgroups of 128 x 64 on 256 CUs)"
