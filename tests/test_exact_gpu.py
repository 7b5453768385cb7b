"""The parity mode (dtype "fp32" = MUDPT_F32, what PREC = "fp32" selects) through the C ABI, against the reference fixtures at the logit scale
pretrained CLIP checkpoints carry: exp(logit_scale) = 100 (the reference multiplies the cosine by it, trainers/mudpt.py:181-182,
trainers/cocoop.py:180,191; the init value of clip/model.py:777 is 14.29).  north_star's bound -- logits within 1e-3 of the reference's
CPU path -- is then 1e-5 on the cosine.  The mode (chosen by the per-site ablation of tests/precision_ablation.py): text tower
on 22-bit (hi, lo) fp16 pairs + fp32 attention (every one of its rounding sites alone costs 2.5e-3); vision tower on hi + e4m3 remainders
contracted on the fp8 matrix pipe, fp16 attention.  Knobs vis_lo = 1, vis_exact_attn = 1 give round 3's "exact" mode (pairs + fp32
attention in both towers), which the same fixtures hold to 3e-5."""
import ctypes as C
import math
import os

import pytest
import torch

from tests.helpers import GoldenCase, ok
from tests.test_model_gpu import build

pytestmark = pytest.mark.gpu

LOGIT_ATOL_EXACT = 1e-3   # north_star, on the MAXIMUM over the logits, at logit scale 100
EXACT_KNOBS = {"vis_lo": 1, "vis_exact_attn": 1}  # round 3's exact mode: fp16 pairs + fp32 attention forward in the vision tower too
LOGIT_ATOL_R3_EXACT = 5e-5  # ... measured 1.5e-5 / 2.5e-5 (208 classes) / 1.2e-5 (ViT-L/14@336)
TINY_SLACK = 1.5          # the 3-layer tiny shapes (embed 128): a relative feature error moves the cosine by eps / sqrt(e), tests/test_model_gpu.py
GRAD_RTOL = 2e-2          # the backward is the fp16 mode's: same bound as tests/test_model_gpu.py GRAD_RTOL["fp16"]


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("B,L,H,causal", [(3, 201, 12, False), (11, 9, 8, True), (5, 77, 8, True), (2, 581, 4, False), (2, 64, 2, False),
                                           (3, 65, 1, True), (1, 1, 1, True), (2, 33, 3, False), (700, 9, 8, True)])
def test_exact_attention_forward(B, L, H, causal):
    """attention_exact.hip against a float64 softmax(QK^T / 8 [+ causal mask]) V: output (hi + lo) to fp32 rounding, the log-sum-exp, and the
    fp16 copy of q | k | v it leaves for the backward."""
    from mudpt_amd import capi
    lib = capi.load()
    g = torch.Generator().manual_seed(L * 7 + H)
    d = H * 64
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 1.5).cuda()
    if L >= 33:
        qkv[0, 5, d:d + 64] *= 6.0  # one key far above the rest: the running maximum jumps inside a later tile (rescale path)
        qkv[0, L - 1, d:d + 64] *= 5.0
    Lp = lib.mudpt_attention_padded_len(L)
    hi = torch.zeros(B, L, d, device="cuda", dtype=torch.float16)
    lo = torch.zeros(B, L, d, device="cuda", dtype=torch.float16)   # the remainder as fp16 (lo_mode 1): same row stride in bytes
    lo8 = torch.zeros(B, L, 2 * d, device="cuda", dtype=torch.uint8)  # ... as e4m3 bytes of remainder * 2^12 (lo_mode 2): the first d bytes of each row
    lse = torch.full((B, H, Lp), float("nan"), device="cuda")  # the kernel must write every row, the padded tail included
    lp = torch.zeros(B, L, 3 * d, device="cuda", dtype=torch.float16)
    rc = lib.mudpt_attention_fwd_exact(P(qkv), P(lp), P(hi), P(lo), 1, d, P(lse), B, L, H, int(causal), None)
    assert rc == 0, lib.mudpt_last_error().decode()
    hi8 = torch.zeros_like(hi)
    rc = lib.mudpt_attention_fwd_exact(P(qkv), None, P(hi8), P(lo8), 2, d, P(lse), B, L, H, int(causal), None)
    assert rc == 0, lib.mudpt_last_error().decode()
    torch.cuda.synchronize()
    hi = torch.cat([hi, lo], dim=-1)  # (the checks below index [hi | lo])
    q, k, v = (t.reshape(B, L, H, 64).transpose(1, 2).double().cpu() for t in qkv.split(d, dim=-1))
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    ref = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, d)
    got = hi[..., :d].double().cpu() + hi[..., d:].double().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"exact attention B {B} L {L} H {H} causal {causal}: max err {err:.2e} (max |O| {scale:.2f})")
    assert err <= 8e-6 * max(scale, 1.0)  # fp32 score rounding at |s| ~ 50 (torch fp32 on the CPU: 6e-6 on this input) + the [hi | lo] pair's 2^-22
    ref_lse = torch.logsumexp(s, dim=-1)
    assert (lse[:, :, :L].double().cpu() - ref_lse).abs().max().item() <= 2e-5
    assert (lse[:, :, L:] == 0).all()  # the padded tail the whole-pair backward kernels read (as the fp16 forward kernels leave it)
    assert torch.equal(lp.cpu(), qkv.half().cpu())
    # hi is the fp16 rounding of the value, lo the remainder: |lo| <= half an ulp of hi
    ulp = torch.ldexp(torch.ones(()), torch.frexp(hi[..., :d].float().abs().clamp_min(6.2e-5)).exponent - 11).cpu()
    assert (hi[..., d:].float().abs().cpu() <= 0.5 * ulp * (1 + 1e-3)).all()
    # the e4m3 form: same hi; the bytes are the OCP e4m3 rounding of remainder * 2^12 (|remainder| <= 2^-11 |O|: far below the 448 maximum here)
    assert torch.equal(hi8, hi[..., :d])
    rem = (ref.float() - hi[..., :d].float().cpu())  # ~ the remainder (the kernel's O differs from the float64 one by fp32 rounding)
    got8 = lo8[..., :d].cpu().view(torch.float8_e4m3fn).float() / 4096.0
    assert (lo8[..., d:] == 0).all()  # the padding half of each row is never written
    assert (got8 - hi[..., d:].float().cpu()).abs().max().item() <= 2.0 ** -4 * hi[..., d:].float().abs().max().item() + 2.0 ** -21  # e4m3: 3 mantissa bits
    assert (got8 - rem).abs().max().item() <= 2.0 ** -4 * rem.abs().max().item() + 1e-5


@pytest.mark.parametrize("name", ["mudpt_tiny_s100", "mudpt_vitb16_b4_s100", "mudpt_vitb16_c208_b2_s100", "mudpt_vitl14_336_b1_s100"])
def test_logits_at_scale_100_within_1e_3(name):
    case = GoldenCase(name)
    assert abs(case.frozen["logit_scale"].exp().item() - 100.0) < 1e-3
    slack = TINY_SLACK if case.cfg.v_layers < 12 else 1.0
    # the 3-layer toy shape has 7 vision tokens and embed 128: its fp16 attention averages over nothing and a relative feature error moves
    # the cosine sqrt(512 / 128) = 2x as far as ViT-B/16's (tests/test_model_gpu.py) -- 2e-3 measured, 3e-3 allowed, for the default mode only
    slack_default = 3.0 if case.cfg.v_layers < 12 else 1.0
    m = build(case, "fp32")
    logits = m(case.images).cpu()
    err = (logits - case.logits).abs().max().item()
    rms = (logits - case.logits).pow(2).mean().sqrt().item()
    print(f"{name} parity mode (dtype fp32): |logit - reference| max {err:.3e} rms {rms:.3e}")
    assert err <= slack_default * LOGIT_ATOL_EXACT, err
    loss, lg = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu(), logits)  # the training step's forward is the inference forward
    assert abs(loss.item() - case.loss) <= slack_default * LOGIT_ATOL_EXACT
    # gradients against the REFERENCE's own (the fixture: every tensor in full, the three big projection weights as the [::8, ::8] sample
    # gen_golden.py stores; the oracle is held to the same fixtures on the CPU, tests/test_oracle_golden.py)
    for k, g in m.grads().items():
        full, sample = case.grad(k), case.grad_sample(k)
        r, g = (full, g.detach().cpu()) if full is not None else (sample, g.detach().cpu()[::8, ::8])
        rms_g = r.pow(2).mean().sqrt().item()
        e = (g - r).abs().max().item()
        print(f"  {k}: rms {rms_g:.3e} max err {e:.3e}")
        assert math.isfinite(e) and e <= GRAD_RTOL * rms_g * 4 + 1e-9, (k, e, rms_g)
        assert torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item() > 0.9995, k
    m.close()
    # round 3's exact mode through the knobs: fp16 pairs + fp32 attention forward in both towers
    m = build(case, "fp32", knobs=EXACT_KNOBS)
    e = (m(case.images).cpu() - case.logits).abs().max().item()
    print(f"{name} dtype fp32 + vis_lo 1 + vis_exact_attn 1 (round 3's exact mode): max {e:.3e}")
    assert e <= slack * LOGIT_ATOL_R3_EXACT
    m.close()
    # for the record: the fast modes at this scale (fp16 = split text tower only; bf16 = the benchmark mode) -- sanity-bounded only
    for dtype, bound in (("fp16", 1.2e-2), ("bf16", 0.25)):
        m = build(case, dtype)
        e = (m(case.images).cpu() - case.logits).abs().max().item()
        print(f"{name} {dtype}: max {e:.3e}")
        assert e <= slack * bound
        m.close()


# name -> knobs of one row of DESIGN.md 2's ablation table (the same rows are timed at B 256 by tools/parity_ablation_bench.py) (site masks: 1 in_proj, 2 out_proj, 4 c_fc, 8 c_proj, 16 patch embed)
ABLATION = [
    ("fp16 mode (vision fp16; text: pairs, fp16 attention)", None, 2e-2),
    ("text exact; vision fp16 everywhere", {"vis_lo": 0}, 6e-3),
    ("text exact; vision e4m3 lo at c_fc, c_proj", {"vis_sites": 4 + 8}, 2.5e-3),
    ("text exact; vision e4m3 lo at c_fc, c_proj, patch", {"vis_sites": 4 + 8 + 16}, 2.5e-3),
    ("text exact; vision e4m3 lo at out_proj, c_fc, c_proj, patch", {"vis_sites": 2 + 4 + 8 + 16}, 2e-3),
    ("text exact; vision e4m3 lo at all four GEMMs", {"vis_sites": 15}, 2e-3),
    ("parity mode: + split pixels", {}, 1e-3),
    ("parity mode with fp16 pairs in the vision tower", {"vis_lo": 1}, 1e-3),
    ("parity mode + vision fp32 attention", {"vis_exact_attn": 1}, 3e-4),
    ("round 3 exact: pairs + fp32 attention", EXACT_KNOBS, LOGIT_ATOL_R3_EXACT),
    ("text pairs but fp16 attention; vision as parity mode", {"txt_exact_attn": 0}, 2e-2),
]


@pytest.mark.parametrize("name", ["mudpt_vitb16_b4_s100", "mudpt_vitb16_c208_b2_s100"] + (["mudpt_vitl14_336_b1_s100"] if os.environ.get("MUDPT_TEST_ABLATION_VITL") else []))
def test_precision_ablation_on_the_gpu(name):
    """The GPU side of tests/precision_ablation.py: each row of DESIGN.md 2's table through the knobs, against the reference's logits at
    logit scale 100.  Bounds are loose sanity limits (2-3x the measured maxima); the printed maxima are what DESIGN.md quotes.
    (ViT-L/14@336 -- six rows, 15 s of weight ingestion each -- only with MUDPT_TEST_ABLATION_VITL=1: its default-mode row is
    test_logits_at_scale_100_within_1e_3's.)"""
    case = GoldenCase(name)
    rows = ABLATION if case.cfg.v_layers == 12 else [ABLATION[i] for i in (0, 1, 2, 6, 8, 9)]
    for label, knobs, bound in rows:
        m = build(case, "fp16" if knobs is None else "fp32", knobs=knobs or {})
        d = m(case.images).cpu() - case.logits
        print(f"{name} | {label}: max {d.abs().max().item():.3e} rms {d.pow(2).mean().sqrt().item():.3e}")
        assert d.abs().max().item() <= bound, label
        m.close()


@pytest.mark.parametrize("name", ["mudpt_tiny", "mudpt_vitb16_b4", "mudpt_vitb16_c208_b2", "mudpt_vitl14_336_b1"])
def test_exact_mode_at_init_scale(name):
    """The same modes on the scale-14.29 fixtures (208 class prompts of mixed length: the length buckets; ViT-L/14@336: the tiled L = 581)."""
    case = GoldenCase(name)
    for knobs, bound in (({}, 2e-4), (EXACT_KNOBS, 2e-5)):
        m = build(case, "fp32", knobs=knobs)
        logits = m(case.images).cpu()
        err = (logits - case.logits).abs().max().item()
        print(f"{name} dtype fp32 {knobs}: max {err:.3e}")
        assert err <= bound * (TINY_SLACK if case.cfg.v_layers < 12 else 1.0)
        m.close()


@pytest.mark.parametrize("name", ["cocoop_tiny_s100", "cocoop_vitb16_b2_s100"])
def test_cocoop_logits_at_scale_100_within_1e_3(name):
    from oracle import cocoop_oracle as CO
    from tests.test_cocoop_gpu import build as build_cocoop
    case = GoldenCase(name)
    slack = TINY_SLACK * 1.5 if case.cfg.v_layers < 12 else 1.0  # CoCoOp's image-feature error enters twice (tests/test_cocoop_gpu.py)
    for knobs, bound in ((EXACT_KNOBS, 5e-5 if case.cfg.v_layers == 12 else 2e-3), ({"vis_exact_attn": 1}, 5e-4 if case.cfg.v_layers == 12 else 2e-3)):
        m = build_cocoop(case.cfg, case.frozen, case.tokens, case.params, "fp32", len(case.labels), knobs=knobs)
        m.eval()
        e = (m(case.images).cpu() - case.logits).abs().max().item()
        print(f"{name} dtype fp32 {knobs}: max {e:.3e}")
        assert e <= bound
        m.close()
    m = build_cocoop(case.cfg, case.frozen, case.tokens, case.params, "fp32", len(case.labels))
    m.eval()
    logits = m(case.images).cpu()
    err = (logits - case.logits).abs().max().item()
    print(f"{name} parity mode (dtype fp32): max {err:.3e}")
    assert err <= slack * LOGIT_ATOL_EXACT
    m.train()
    loss, train_logits = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(train_logits.cpu(), logits)  # the training step's forward is the inference forward
    assert abs(loss.item() - case.loss) <= slack * LOGIT_ATOL_EXACT
    # gradients: the bf16 constants as the hard bound (the mode runs lp_grad = 1), inside them twice what this fixture measured against the
    # oracle (tests/test_knobs_gpu.py PARITY_STEP_MEASURED), against the fixture's stored gradients too; the cosine at the fp16 floor
    from tests.helpers import GRAD_COS, check_parity_step_grads
    from tests.test_knobs_gpu import PARITY_STEP_MEASURED
    got = {k: g.detach().cpu().clone() for k, g in m.grads().items()}
    m.close()
    assert all(torch.isfinite(g).all() for g in got.values())
    oracle = CO.forward_backward(case.cfg, case.frozen, case.params, case.class_embedding, case.eot, case.images, case.labels)[2]
    worst = check_parity_step_grads(name, [(k, got[k], oracle[k]) for k in CO.TRAINABLE_ORDER], PARITY_STEP_MEASURED[name])
    check_parity_step_grads(name + " (fixture)", [(k, got[k], case.grad(k)) for k in CO.TRAINABLE_ORDER], PARITY_STEP_MEASURED[name])
    assert worst[2] > GRAD_COS["fp16"], worst


def _split_operand(x32, lo_mode):
    """hi, the low buffer as the library lays it out (same row stride in bytes as hi) and the value hi + decoded(lo) the second pass sees."""
    hi = x32.half()
    rem = x32 - hi.float()
    if lo_mode == 1:
        lo = rem.half()
        return hi, lo, hi.double() + lo.double()
    lo8 = torch.zeros(x32.shape[0], 2 * x32.shape[1], dtype=torch.uint8)
    q = (rem * 4096.0).clamp(-448, 448).to(torch.float8_e4m3fn)
    lo8[:, :x32.shape[1]] = q.view(torch.uint8)
    return hi, lo8, hi.double() + q.float().double() / 4096.0


def _e4m3_weights(lib, W):
    """The library's own host conversion (what mudpt_set_weight applies): e4m3 of W * 2^shift in rows of 2 K bytes + the E8M0 block scale."""
    mx = W.abs().max().item()
    shift = int(math.floor(math.log2(448.0 / mx)))
    Wf = W.float().contiguous()
    raw = torch.zeros(W.numel(), dtype=torch.uint8)
    assert lib.mudpt_e4m3_from_f32(P(Wf), P(raw), W.numel(), shift) == 0
    assert torch.equal(raw, (Wf * 2.0 ** shift).to(torch.float8_e4m3fn).view(torch.uint8).flatten())  # = torch's OCP e4m3fn rounding
    W8 = torch.zeros(W.shape[0], 2 * W.shape[1], dtype=torch.uint8)
    W8[:, :W.shape[1]] = raw.view(W.shape)
    return W8, 127 - shift, raw.view(W.shape).view(torch.float8_e4m3fn).float().double() / 2.0 ** shift


@pytest.mark.parametrize("lo_mode", [1, 2])
@pytest.mark.parametrize("M,N,K,epi", [(804, 768, 768, 5), (99, 512, 2048, 2), (804, 3072, 768, 1), (6000, 3072, 1536, 1), (22000, 2048, 1024, 1),
                                        (51456 // 4, 2304, 768, 0), (13000, 768, 3072, 5), (700, 192, 128, 0),
                                        # K = 640 (ViT-L/14's padded patch rows): 10 + 5 K-steps per tile, an odd count -- the LDS stage of a tile's first
                                        # step alternates from tile to tile; N = 1008: a ragged last column tile; both on the persistent kernel
                                        (30000, 1024, 640, 5), (20000, 1008, 1024, 0)])
def test_split_operand_gemm(lo_mode, M, N, K, epi):
    """A forward GEMM of a split tower: first pass hi . W^T, second pass over the low half -- fp16 remainders against the same W (lo_mode 1)
    or e4m3 remainders against the e4m3 weights on the MX-scaled fp8 matrix instruction (lo_mode 2) -- through the small-tile kernel and
    the persistent kernel (full + half tiles), with the store / fp32-store / residual / QuickGELU epilogues.  The result must equal the
    float64 contraction of the operands AS QUANTISED (the kernels add fp32 accumulation only); with epilogue 1 the QuickGELU output comes
    back as a split operand itself in the same form."""
    from mudpt_amd import capi
    lib = capi.load()
    g = torch.Generator().manual_seed(M + N + K + lo_mode)
    A32 = torch.randn(M, K, generator=g) * 1.5
    A32[0, :8] = torch.tensor([300.0, -250.0, 1e-4, 0.0, 3e-3, 65.0, -7.7, 100.0])  # large values (e4m3 remainders near the 448 limit), tiny ones
    W = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    bias = torch.randn(N, generator=g)
    hi, lo, a_eff = _split_operand(A32, lo_mode)
    W8, s8, w8_eff = _e4m3_weights(lib, W) if lo_mode == 2 else (None, 127, None)
    hi_d, lo_d, W_d, bias_d = hi.cuda(), lo.cuda(), W.cuda(), bias.cuda()
    W8_d = W8.cuda() if W8 is not None else None
    aux = torch.randn(M, N, generator=g).cuda() if epi == 2 else None
    out_f32 = epi in (2, 5)
    out0 = torch.zeros(M, N, device="cuda", dtype=torch.float32 if out_f32 else torch.float16)
    out1 = torch.zeros(M, N, device="cuda", dtype=torch.float16) if epi == 1 else None
    out1_lo = (torch.zeros(M, N, device="cuda", dtype=torch.float16) if lo_mode == 1 else torch.zeros(M, 2 * N, device="cuda", dtype=torch.uint8)) if epi == 1 else None
    ok(lib, capi.call("mudpt_gemm_split", dtype=1, epilogue=epi, M=M, N=N, K=K, A=hi_d, A_lo=lo_d, lo_mode=lo_mode, lda=K, B=W_d, B8=W8_d, b8_scale=s8, ldb=K, bias=bias_d,
                      out0=out0, ldo0=N, out1=out1, out1_lo=out1_lo, out1_lo_mode=lo_mode, ldo1=N, aux=aux, ldaux=N))
    # what the two passes contract: hi . W + lo . (W or its e4m3 copy)
    Wd = W.double()
    ref = hi.double() @ Wd.t() + (a_eff - hi.double()) @ (w8_eff if lo_mode == 2 else Wd).t() + bias.double()
    if epi == 2:
        ref = ref + aux.double().cpu()
    mag = (hi.double().abs() @ Wd.abs().t()).max().item()
    got = out0.double().cpu()
    err = (got - ref).abs().max().item()
    print(f"split GEMM lo_mode {lo_mode} {M}x{N}x{K} epi {epi}: max err {err:.2e} (sum |a b| up to {mag:.1f})")
    if out_f32:
        assert err <= 1e-6 * mag + 1e-6  # fp32 accumulation over K products in the kernels' order
    else:
        assert err <= 2.0 ** -11 * ref.abs().max().item() + 1e-6
    # and the second pass is really there: against the full-precision operand the split result is far closer than hi alone
    full = A32.double() @ Wd.t() + bias.double() + (aux.double().cpu() if epi == 2 else 0)
    if out_f32:
        e_split, e_hi = (got - full).abs().max().item(), (hi.double() @ Wd.t() + bias.double() + (aux.double().cpu() if epi == 2 else 0) - full).abs().max().item()
        assert e_split <= (0.02 if lo_mode == 1 else 0.25) * e_hi + 1e-6 * mag, (e_split, e_hi)
    if epi == 1:
        gelu = ref * torch.sigmoid(1.702 * ref)
        g_hi = out1.double().cpu()
        g_lo = out1_lo.double().cpu() if lo_mode == 1 else out1_lo[:, :N].cpu().view(torch.float8_e4m3fn).float().double() / 4096.0
        if lo_mode == 2:
            assert (out1_lo[:, N:] == 0).all()
        tol = 1e-5 if lo_mode == 1 else 2.0 ** -15  # the pair carries 22 bits (+ the hardware exp / rcp of QuickGELU, 1 ulp each); hi + e4m3 remainder 11 + 4
        e = ((g_hi + g_lo - gelu).abs() / gelu.abs().clamp_min(1.0)).max().item()
        print(f"   QuickGELU output as a split operand: max relative err {e:.2e}")
        assert e <= tol
        assert (out1.float() - (out1.float() + g_lo.float().cuda())).abs().max().item() <= 2.0 ** -11 * out1.float().abs().max().item()


@pytest.mark.parametrize("lo_mode", [1, 2])
def test_layernorm_writes_split_operands(lo_mode):
    from mudpt_amd import capi
    lib = capi.load()
    g = torch.Generator().manual_seed(5 + lo_mode)
    rows, d = 1000, 768
    x = (torch.randn(rows, d, generator=g) * 3 + 0.5).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.05 * torch.randn(d, generator=g)).cuda()
    out = torch.zeros(rows, d, device="cuda", dtype=torch.float16)
    lo = torch.zeros(rows, d, device="cuda", dtype=torch.float16) if lo_mode == 1 else torch.zeros(rows, 2 * d, device="cuda", dtype=torch.uint8)
    ok(lib, capi.call("mudpt_layernorm_fwd_split", dtype=1, x=x, ldx=d, gamma=gamma, beta=beta, out=out, out_lo=lo, lo_mode=lo_mode, ldo=d, rows=rows, d=d))
    y = torch.nn.functional.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5).cpu()
    lo_v = lo.double().cpu() if lo_mode == 1 else lo[:, :d].cpu().view(torch.float8_e4m3fn).float().double() / 4096.0
    err = (out.double().cpu() + lo_v - y).abs().max().item()
    print(f"LayerNorm split output, lo_mode {lo_mode}: max |hi + lo - y| = {err:.2e}")
    assert (out.double().cpu() - y).abs().max().item() <= 2.0 ** -11 * y.abs().max().item()
    assert err <= (2e-6 if lo_mode == 1 else 2.0 ** -15) * y.abs().max().item()
