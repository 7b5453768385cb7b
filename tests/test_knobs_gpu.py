"""The wiring of the kernels in model.cpp, one level above the single-kernel suites: every knob of mudpt_model_set on a whole step, the
identities the code states between its kernel forms, what a step leaves behind in a handle, the caller's stream and a second handle.

  1. every non-default setting of MODEL_KNOBS (tests/helpers.py) against the oracle, with the checks of
     tests/test_model_gpu.py::test_loss_and_grads_match_reference;
  2. bit for bit (torch.equal): backward-only knobs leave logits and loss alone; block 0's attention window changes nothing; the GEMM kernel
     choice changes nothing once split K (a differently associated sum) is off;
  3. a step after another step, an eval forward and new parameters equals that step on a fresh handle, with knobs flipped in between too;
  4. a step on a side stream whose inputs become valid only on that stream, and two handles stepping in turns.

One handle per (fixture, dtype) lives for the whole module (weights are uploaded from the host: seconds for ViT-B/16, more for ViT-L/14); a case
moves knobs with CustomCLIP.set_knob and sets them back (helpers.KNOB_DEFAULTS).  A run under a setting is computed once and shared by the
tests that need it; the oracle's gradients once per fixture."""
import contextlib
import dataclasses
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch

from oracle import mudpt_oracle as O
from tests import coop_reference as CR
from tests import helpers as H
from tests import test_cocoop_gpu as TCC
from tests import test_coop_gpu as TC
from tests import test_exact_gpu as TE
from tests import test_manyclass_gpu as TMC
from tests import test_model_gpu as TM
from tests import test_umudpt_gpu as TU
from tests import test_uumudpt_gpu as TUU
from tests import test_vpt_gpu as TV
from tests import vpt_reference as VR
from tests.helpers import GRAD_COS, GRAD_RMS, GRAD_RTOL, KNOB_DEFAULTS, LOGIT_ATOL, TINY_SLACK, GoldenCase

pytestmark = pytest.mark.gpu
DTYPES = ("fp16", "bf16")
Step = namedtuple("Step", "logits loss grads")  # of one forward_backward: host copies

_CASES, _HANDLES, _RUNS, _ORACLE = {}, {}, {}, {}
# The attention window works in blocks of 16 query rows (attention.hip in_win), so an extent that is one row short shows only where the last
# prompt row OPENS a block -- in no committed fixture.  Two seeded shapes (the oracle's recipes, as tests/test_edge_gpu.py builds its own)
# put it there: n_ctx 12 on the tiny vision tower (rows 5 .. 16 of 17), n_ctx 16 on the text tower (rows 1 .. 16)
SEEDED_SHAPES = {"seeded_tiny_n12": 12, "seeded_tiny_n16": 16}


def load(name):
    """The fixture `name` with .images, .labels and .params (the trainables by state-dict key), whatever its trainer variant; built once."""
    if name not in _CASES:
        if name == "oracle_vitb16_c1000_b2":
            from tests.golden import gen_oracle_c1000 as G
            cfg, frozen, tok, params, images, labels = G.inputs()
            c = SimpleNamespace(cfg=cfg, frozen=frozen, tokens=tok, params=params, images=images, labels=labels)
        elif name in SEEDED_SHAPES:
            cfg = dataclasses.replace(O.TINY, n_ctx=SEEDED_SHAPES[name], depth=2)
            g = torch.Generator().manual_seed(73)
            c = SimpleNamespace(cfg=cfg, frozen=O.make_frozen_state(cfg, 71), tokens=O.synthetic_tokens(cfg, 5).long(), params=O.make_trainable_state(cfg, 72),
                                images=torch.randn(3, 3, cfg.image_size, cfg.image_size, generator=g), labels=torch.randint(0, 5, (3,), generator=g))
        elif name.startswith("coop_"):
            c = CR.CoopCase(name)
            c.params = {CR.CTX: c.ctx}
        elif name.startswith(("vpt_", "mpt_")):
            c = VR.VptCase(name)
        elif name.startswith("umudpt_"):
            c = TU.load(name)
        elif name.startswith("uumudpt_"):
            c = TUU.load(name)
        else:
            c = GoldenCase(name)
        _CASES[name] = c
    return _CASES[name]


def build(name, dtype, max_batch=None, knobs=None):
    """A new handle on the fixture through its variant's own build helper, with the fixture's parameters set."""
    c = load(name)
    mb = max_batch or len(c.labels)
    if name == "oracle_vitb16_c1000_b2" or name in SEEDED_SHAPES:
        return TMC.build(c.cfg, c.frozen, c.tokens, c.params, dtype, mb, knobs=knobs)
    if name.startswith("coop_"):
        return TC.build(c, dtype, max_batch=mb, knobs=knobs)
    if name.startswith("cocoop_"):
        return TCC.build(c.cfg, c.frozen, c.tokens, c.params, dtype, mb, knobs=knobs)
    mod = TV if name.startswith(("vpt_", "mpt_")) else TU if name.startswith("umudpt_") else TUU if name.startswith("uumudpt_") else TM
    return mod.build(c, dtype, max_batch=mb, knobs=knobs)


def handle(name, dtype):
    """The module's handle on (fixture, dtype): max_batch = the fixture's batch, default knobs, the fixture's parameters."""
    if (name, dtype) not in _HANDLES:
        _HANDLES[name, dtype] = build(name, dtype)
    return _HANDLES[name, dtype]


@pytest.fixture(scope="module", autouse=True)
def _module_handles():
    yield
    for m in _HANDLES.values():
        m.close()
    for cache in (_HANDLES, _RUNS, _ORACLE, _CASES, _FRESH):
        cache.clear()


@contextlib.contextmanager
def knobs_set(m, dtype, sets):
    """Apply (name, value) calls in order; afterwards every knob this module moves is back at the dtype's default."""
    try:
        for k, v in sets:
            m.set_knob(k, v)
        yield m
    finally:
        for k, v in KNOB_DEFAULTS[dtype].items():
            m.set_knob(k, v)


def step(m, images, labels):
    loss, logits = m.forward_backward(images, labels, return_logits=True)
    return Step(logits.cpu(), loss.item(), {k: g.detach().cpu().clone() for k, g in m.grads().items()})


def run(name, dtype, sets=(), construct=False):
    """The fixture's own step on the module's handle under the setting `sets` (construct: on a handle built with it), computed once."""
    key = (name, dtype, tuple(sets))
    if key not in _RUNS:
        c = load(name)
        if construct:
            m = build(name, dtype, knobs=dict(sets))
            _RUNS[key] = step(m, c.images, c.labels)
            m.close()
        else:
            m = handle(name, dtype)
            m.set_params(c.params)
            with knobs_set(m, dtype, sets):
                _RUNS[key] = step(m, c.images, c.labels)
    return _RUNS[key]


def oracle_grads(name):
    if name not in _ORACLE:
        c = load(name)
        _ORACLE[name] = O.forward_backward(c.cfg, c.frozen, c.params, c.class_embedding, c.eot, c.images, c.labels)[2]
    return _ORACLE[name]


def assert_same_step(got, want, tag):
    """Logits, loss and every gradient tensor bit for bit."""
    bad = [] if torch.equal(got.logits, want.logits) else [("logits", (got.logits - want.logits).abs().max().item())]
    if got.loss != want.loss:
        bad.append(("loss", abs(got.loss - want.loss)))
    assert got.grads.keys() == want.grads.keys()
    for k, g in want.grads.items():
        if not torch.equal(got.grads[k], g):
            bad.append((k, (got.grads[k] - g).abs().max().item() / max(g.pow(2).mean().sqrt().item(), 1e-30)))
    assert not bad, f"{tag}: not bit-identical (logits / loss: max difference; gradients: max difference / rms): {bad}"
    assert all(torch.isfinite(g).all() for g in want.grads.values()) and sum(g.abs().sum().item() for g in want.grads.values()) > 0


def fixture_ids(v):
    return v.id if isinstance(v, H.KnobSetting) else str(v)


# ---- 1. every non-default setting against the oracle ------------------------------------------------------------------------------------
ORACLE_CASES = ([(name, s) for name in ("mudpt_tiny", "mudpt_vitb16_b4") for s in H.knob_settings() if s.dtype != "fp32"]
                # L = 581 > 224: the two attention-form knobs meet the resident / staged forms
                + [("mudpt_vitl14_336_b1", s) for s in H.knob_settings(H.ATTN_FORM_KNOBS)]
                # the parity mode's own knobs at the logit scale its bound is stated at
                + [(name, s) for name in ("mudpt_tiny_s100", "mudpt_vitb16_b4_s100") for s in H.knob_settings(dtype="fp32")])


# What the settings that lower an fp16 handle's grade measure on an MI355X against the oracle (O.forward_backward on the CPU, as in
# test_loss_and_grads_match_reference; logits and loss against the fixture's), the worse of mudpt_tiny and mudpt_vitb16_b4:
# (max |logit error|, worst tensor's max gradient error / its rms, worst tensor's rms gradient error / its rms).  The default fp16 handle
# measures (8.4e-4, 1.8e-2, 2.1e-3) there; the smallest cosine over all of them is 0.999995, so the fp16 floor stays.  The test bounds each
# by TWICE its row, and by the bf16 constants where those are smaller.
LOWERED_MEASURED = {
    "lp_grad": (8.5e-4, 2.4e-2, 3.1e-3),    # header: "30 % more gradient error" -- ViT-B/16: max 1.8e-2 -> 2.4e-2, rms 2.0e-3 -> 3.1e-3; logits untouched (backward only)
    "lp_upd": (1.3e-3, 2.5e-2, 2.5e-3),     # header: "2e-4 of logit error" -- 6.0e-4 -> 7.1e-4 on ViT-B/16, 8.4e-4 -> 1.23e-3 on the tiny shape
    "gelu_q8": (8.5e-4, 1.8e-2, 2.1e-3),    # header: "2.4e-3 on a factor" -- below the fp16 backward's own noise: figures as the default's
    "txt_split": (1.6e-3, 2.5e-2, 2.8e-3),  # test_model_gpu.py: "with plain 11-bit operands ... single logits reached 1.5e-3": 1.57e-3 on ViT-B/16
    "txt_lo": (1.6e-3, 2.5e-2, 2.8e-3),     # the same setting between two steps: the same figures to the last digit
    "txt_sites": (1.2e-3, 2.2e-2, 2.5e-3),  # in_proj and c_fc split, out_proj and c_proj not: between the two
}


# What the parity mode's own knobs measure on an MI355X against the oracle at logit scale 100, the worse of mudpt_tiny_s100 and
# mudpt_vitb16_b4_s100: setting -> (worst tensor's max gradient error / its rms, worst tensor's rms gradient error / its rms, smallest
# cosine).  The default parity handle measures the "default" row; all of them are expected near LOWERED_MEASURED["lp_grad"] (the backward
# is the fp16 mode's with lp_grad = 1, whatever the forward's operands).  The test bounds each by TWICE its row inside the bf16 constants.
PARITY_KNOBS_MEASURED = {  # (the ViT-B/16 fixture is the worse one in every row; logits: 3.8e-4, 3.0e-4, 7.8e-5, 1.2e-5, 3.4e-3 there)
    "vis_lo1-fp32": (2.44e-2, 3.03e-3, 0.999995),
    "vis_sites12-fp32": (2.83e-2, 3.43e-3, 0.999994),
    "vis_exact_attn1-fp32": (2.87e-2, 3.51e-3, 0.999994),
    "vis_exact_attn1-vis_lo1-fp32": (2.86e-2, 3.50e-3, 0.999994),
    "txt_exact_attn0-fp32": (3.45e-2, 3.28e-3, 0.999995),
}


def parity_logit_bound(c, setting):
    """The bound test_exact_gpu.py's ablation holds the row with these knobs to (ViT-B/16 at logit scale 100); on the 3-layer tiny shape
    times the slack test_logits_at_scale_100_within_1e_3 gives it: 3 while the vision attention runs in fp16 (7 tokens: it averages over
    nothing), TINY_SLACK once vis_exact_attn = 1."""
    bound = next(b for _, knobs, b in TE.ABLATION if knobs == dict(setting.sets))
    if c.cfg.v_layers >= 12:
        return bound
    return bound * (TE.TINY_SLACK if dict(setting.sets).get("vis_exact_attn") else 3.0)


def check_parity_setting(name, setting):
    """test_setting_matches_the_oracle on a dtype "fp32" handle: logits and loss against the fixture inside the ablation's bound for the
    row; every gradient tensor against the oracle with the bf16 constants as the hard bound (the mode runs lp_grad = 1) and, inside them,
    twice PARITY_KNOBS_MEASURED's row; the fp16 cosine floor.  (ViT-L/14@336, where vis_exact_attn = 1 feeds the staged or resident backward
    at L = 581, is left to the ablation's logits: one handle's weight ingestion alone takes 15 s.)"""
    c = load(name)
    got = run(name, "fp32", setting.sets)
    logit_tol = parity_logit_bound(c, setting)
    dl = (got.logits - c.logits).abs().max().item()
    print(f"{name} {setting.id}: |loss - reference| {abs(got.loss - c.loss):.3e} |logit - reference| max {dl:.3e} (bound {logit_tol:.2e})")
    assert abs(got.loss - c.loss) <= logit_tol and dl <= logit_tol
    grad_max, grad_rms, cos_floor = 4 * GRAD_RTOL["bf16"], GRAD_RMS["bf16"], GRAD_COS["fp16"]
    measured = PARITY_KNOBS_MEASURED[setting.id]
    grad_max, grad_rms = min(grad_max, 2 * measured[0]), min(grad_rms, 2 * measured[1])
    ref, worst = oracle_grads(name), [0.0, 0.0, 1.0]
    for k in O.TRAINABLE_ORDER:
        r, g = ref[k], got.grads[k]
        rms = r.pow(2).mean().sqrt().item()
        err = (g - r).abs().max().item()
        rel_rms = (g - r).pow(2).mean().sqrt().item() / max(rms, 1e-30)
        cos = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
        worst = [max(worst[0], err / max(rms, 1e-30)), max(worst[1], rel_rms), min(worst[2], cos)]
        print(f"  {k}: rms {rms:.3e} max err {err / max(rms, 1e-30):.3e} x rms (bound {grad_max:.2e}) rms err {rel_rms:.3e} x rms (bound {grad_rms:.2e}) cos {cos:.6f}")
        assert err <= grad_max * rms + 1e-9, (k, err, rms)
        assert rel_rms <= grad_rms or rms == 0, (k, rel_rms)
        assert cos > cos_floor, (k, cos)
    print(f"{name} {setting.id}: worst tensor max {worst[0]:.2e} rms {worst[1]:.2e} cos {worst[2]:.6f}")


# What one training step of a parity-mode handle (dtype "fp32") measures on an MI355X against the variant's restatement, the worst tensor:
# fixture -> (max gradient error / rms, rms gradient error / rms, smallest cosine).  The variants' suites (test_parity_mode_training_step in
# test_coop_gpu.py, test_vpt_gpu.py, test_umudpt_gpu.py, test_uumudpt_gpu.py; the CoCoOp half of test_exact_gpu.py) hold each fixture to TWICE
# its row inside the bf16 constants (helpers.check_parity_step_grads).  Expected near LOWERED_MEASURED["lp_grad"]: the same backward.
# The ViT-B/16 rows at logit scale 100 with a larger RMS error are sums of nearly cancelling per-class terms (CoOp's shared context, MPT's
# text prompts, CoCoOp: the kappa of tests/test_cocoop_gpu.py; the softmax is more peaked at scale 100), the same relative error on every
# tensor of the fixture; UUMuDPT's larger maximum is the tail of 1.7 M-element generator weights at an RMS error of 2.8e-3.  No row points at
# a wrong copy: that gives O(1).  (A cosine that prints as 1.000000 is recorded as 0.999999.)
PARITY_STEP_MEASURED = {
    "coop_tiny_end": (1.03e-2, 2.11e-3, 0.999998), "coop_tiny_middle": (6.63e-3, 1.49e-3, 0.999999), "coop_tiny_front": (6.34e-3, 1.31e-3, 0.999999),
    "coop_tiny_end_csc": (7.55e-3, 9.14e-4, 0.999999), "coop_tiny_middle_csc": (6.17e-3, 8.97e-4, 0.999999), "coop_tiny_front_csc": (7.70e-3, 9.45e-4, 0.999999),
    "coop_vitb16_b2_s100": (2.82e-2, 5.23e-3, 0.999986),
    "vpt_tiny": (3.85e-3, 8.67e-4, 0.999999), "mpt_tiny": (5.20e-3, 1.30e-3, 0.999999), "mpt_tiny_textonly": (4.03e-3, 9.98e-4, 0.999999),
    "vpt_vitb16_b2_s100": (7.89e-3, 1.05e-3, 0.999999), "mpt_vitb16_b2_s100": (2.74e-2, 5.10e-3, 0.999987),
    "umudpt_tiny": (9.58e-3, 1.43e-3, 0.999999), "umudpt_vitb16_b2_s100": (1.98e-2, 2.88e-3, 0.999996),
    "uumudpt_tiny": (1.83e-2, 1.49e-3, 0.999999), "uumudpt_vitb16_b2_s100": (4.94e-2, 3.12e-3, 0.999995),
    "cocoop_tiny_s100": (1.30e-2, 2.25e-3, 0.999998), "cocoop_vitb16_b2_s100": (5.71e-2, 6.95e-3, 0.999976),
}


@pytest.mark.parametrize("name,setting", ORACLE_CASES, ids=fixture_ids)
def test_setting_matches_the_oracle(name, setting):
    """One step under the setting, then the checks of test_loss_and_grads_match_reference with the dtype's own constants: loss and logits
    against the fixture, every gradient tensor's max error, RMS error and cosine against the oracle, and its max error against the
    reference's stored gradient.  include/mudpt.h: "no knob is needed for correct results" -- nor may one give wrong ones.

    Settings that do not change the arithmetic grade (kernel forms, the window, gemm_variant, a bf16 stream or GELU factor moved UP to fp32 / T)
    keep the handle's dtype's constants.  Settings that lower an fp16 handle's grade (KnobSetting.lowers: lp_grad 1, lp_upd 1, gelu_q8 1, no or
    fewer split operands in the text tower) have the bf16 constants as their hard bound: bf16 mode runs with all of them on at a 16 x
    coarser T, and a wiring error gives O(1) errors either way.  Inside it, each is held to twice what it measures against the oracle
    (LOWERED_MEASURED, with the header's figure for the trade beside it).  Every figure is printed against the oracle for the record."""
    if setting.dtype == "fp32":
        return check_parity_setting(name, setting)
    c, dtype = load(name), setting.dtype
    got = run(name, dtype, setting.sets, setting.construct)
    grade = "bf16" if setting.lowers else dtype
    slack = TINY_SLACK if c.cfg.v_layers < 12 else 1.0
    logit_tol, grad_max, grad_rms, cos_floor = slack * LOGIT_ATOL[grade], 4 * GRAD_RTOL[grade], GRAD_RMS[grade], GRAD_COS[grade]
    if setting.lowers:
        measured = LOWERED_MEASURED[setting.sets[0][0]]
        logit_tol, grad_max, grad_rms = min(logit_tol, 2 * measured[0]), min(grad_max, 2 * measured[1]), min(grad_rms, 2 * measured[2])
        cos_floor = GRAD_COS["fp16"]
    dl = (got.logits - c.logits).abs().max().item()
    print(f"{name} {setting.id} (grade {grade}): |loss - reference| {abs(got.loss - c.loss):.3e} |logit - reference| max {dl:.3e} (bound {logit_tol:.2e})")
    assert abs(got.loss - c.loss) <= logit_tol
    assert dl <= logit_tol
    ref = oracle_grads(name)
    for k in O.TRAINABLE_ORDER:
        r, g = ref[k], got.grads[k]
        rms = r.pow(2).mean().sqrt().item()
        err = (g - r).abs().max().item()
        rel_rms = (g - r).pow(2).mean().sqrt().item() / max(rms, 1e-30)
        cos = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
        print(f"  {k}: rms {rms:.3e} max err {err / max(rms, 1e-30):.3e} x rms (bound {grad_max:.2e}) rms err {rel_rms:.3e} x rms (bound {grad_rms:.2e}) cos {cos:.6f}")
        assert err <= grad_max * rms + 1e-9, (k, err, rms)
        assert rel_rms <= grad_rms or rms == 0, (k, rel_rms)
        assert cos > cos_floor, (k, cos)
        full = c.grad(k)
        if full is not None:
            assert (g - full).abs().max().item() <= grad_max * rms + 1e-9, k


# ---- 2. the identities the code states, bit for bit ---------------------------------------------------------------------------------------
BACKWARD_ONLY = ("attn_window", "attn_two_kernels", "attn_fused_w1", "gelu_q8", "lp_grad")  # lp_grad: with lp_upd pinned (MODEL_KNOBS' bf16 row)


# the same five on a parity-mode handle, each moved off that mode's default
PARITY_BACKWARD_ONLY = [H.KnobSetting("fp32", ((k, 1 - KNOB_DEFAULTS["fp32"][k]),)) for k in BACKWARD_ONLY]


@pytest.mark.parametrize("name,setting", [(n, s) for n in ("mudpt_tiny", "mudpt_vitb16_b4") for s in H.knob_settings(BACKWARD_ONLY) + PARITY_BACKWARD_ONLY], ids=fixture_ids)
def test_backward_only_knob_leaves_the_forward_alone(name, setting):
    """The attention backward's forms and window, the 8-bit QuickGELU' codes (c_fc's second output; QuickGELU(u) itself is written as before)
    and the gradient stream's type are read by the backward alone: logits and loss of the step equal the default's bit for bit.  The two
    that change the backward's arithmetic do move the gradients -- a knob the step ignores would pass everything else here."""
    base, got = run(name, setting.dtype), run(name, setting.dtype, setting.sets)
    assert torch.equal(got.logits, base.logits) and got.loss == base.loss, (got.logits - base.logits).abs().max().item()
    if setting.dtype == "fp32" and setting.sets[0][0] == "gelu_q8":
        # both towers of the parity mode run split operands, and a tower with split operands keeps u in T whatever the knob says (model.cpp:
        # "gelu_q8 && t.split == LO_NONE"): the whole step is the default's
        assert_same_step(got, base, f"{name} fp32 gelu_q8 1 vs 0")
    elif setting.sets[0][0] in ("gelu_q8", "lp_grad"):
        assert any(not torch.equal(got.grads[k], g) for k, g in base.grads.items())


WINDOW_FIXTURES = ["mudpt_tiny", "mudpt_vitb16_b4",  # L = 201: BWD_TWO
                   "mudpt_vitl14_336_b1",            # L = 581: BWD_STAGED
                   "mudpt_vitb16_c208_b2",           # several text length buckets: the window's extent per bucket
                   "coop_tiny_middle", "coop_tiny_front_csc", "coop_vitb16_c208_middle_b2",  # context rows around / behind the class name: head_span > n
                   "seeded_tiny_n12", "seeded_tiny_n16"]  # the last prompt row opens a 16-row block: vision tower, text tower


WINDOW_CASES = [(n, dt) for n in WINDOW_FIXTURES for dt in DTYPES] + [(n, "fp32") for n in ("mudpt_tiny", "coop_tiny_middle", "seeded_tiny_n16")]


@pytest.mark.parametrize("name,dtype", WINDOW_CASES)
def test_attention_window_changes_nothing(name, dtype):
    """kernels.h: the windowed attention backward computes "the same sums in the same order as without the window" on its rows and writes no
    other row of dqkv; block_bwd reads the prompt rows alone.  With attn_two_kernels = 1 the windowed and the full call run the same form
    (attn_form), so attn_window 0 and 1 give the same step bit for bit -- unless the window's extent (model arithmetic: head_span, the
    bucket's length) misses a row the model reads.  The kernels round the window out to blocks of 16 rows, which hides a short extent in
    every committed fixture (their last prompt row lies inside a block): SEEDED_SHAPES are where it shows."""
    two = (("attn_two_kernels", 1),)
    c, m = load(name), handle(name, dtype)
    try:  # the windowed step behind ANOTHER step: a row the window leaves unwritten then holds that step's value, not this one's
        dirty(m, c, len(c.labels), len(c.labels))
        m.set_params(c.params)
        with knobs_set(m, dtype, two):
            windowed = step(m, c.images, c.labels)
    finally:
        m.set_params(c.params)
    assert_same_step(windowed, run(name, dtype, two + (("attn_window", 0),)), f"{name} {dtype} window vs all rows")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["mudpt_vitb16_b4",           # M = 804: the 64 x 64 forms at both K depths against 128-wide tiles
                                  "oracle_vitb16_c1000_b2"])  # the text tower's persistent kernel (bf16: with the 8-bit GELU codes) against simple tiles
def test_gemm_kernel_choice_changes_nothing(name, dtype):
    """gemm.hip: every GEMM kernel contracts K in the same order and produces bit-identical rows.  With split_k = 0 (a split sum is
    associated differently) a whole step under gemm_variant 12 (no 128-deep K-tiles), 1 (simple tiles instead of the persistent kernel) and
    10 (64 x 64 tiles, 128-deep where K allows) equals the default dispatch's bit for bit."""
    base = run(name, dtype, (("split_k", 0),))
    for v in (12, 1, 10):
        assert_same_step(run(name, dtype, (("split_k", 0), ("gemm_variant", v))), base, f"{name} {dtype} gemm_variant {v} vs 0")


# ---- 3. a step leaves nothing behind --------------------------------------------------------------------------------------------------------
def other_inputs(c, n, n_cls, seed):
    """Parameters, n images (scaled by 2) and labels unlike the fixture's, from `seed`."""
    g = torch.Generator().manual_seed(seed)
    params = {k: v + 0.02 * torch.randn(v.shape, generator=g) for k, v in c.params.items()}
    return params, 2.0 * torch.randn(n, *c.images.shape[1:], generator=g), torch.randint(0, n_cls, (n,), generator=g)


def dirty(m, c, n_first, n_eval):
    """Leave another step's and an eval forward's values in every buffer of the handle: a training step on n_first images with other
    parameters (finite results asserted), then an eval forward on a third batch, which reuses the step's text features where the variant
    allows (MUDPT_FWD_REUSE_TEXT)."""
    params, images, labels = other_inputs(c, n_first, m.n_cls, 0xA)
    m.set_params(params)
    first = step(m, images, labels)
    assert torch.isfinite(first.logits).all() and all(torch.isfinite(g).all() for g in first.grads.values())
    assert sum(g.abs().sum().item() for g in first.grads.values()) > 0
    m.eval()
    assert torch.isfinite(m(torch.randn(n_eval, *c.images.shape[1:], generator=torch.Generator().manual_seed(0xC)))).all()
    m.train()
    return first


LEFTOVER_FIXTURES = ["mudpt_tiny", "mudpt_vitb16_b4", "coop_tiny_end", "coop_tiny_middle_csc", "cocoop_tiny", "vpt_tiny", "mpt_tiny", "umudpt_tiny", "uumudpt_tiny"]
_FRESH = {}


@pytest.mark.parametrize("first", ["same_size", "larger"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", LEFTOVER_FIXTURES)
def test_step_leaves_nothing_behind(name, dtype, first):
    """block_bwd: "the other rows of t.dx / t.dx_lp are left stale and nothing reads them"; the last block's scatters, the split-K scratch,
    the T-precision streams and the 8-bit GELU codes likewise survive a step.  Repeating one step cannot see a stale read (stale = fresh), so:
    parameters, images (x 2) and labels of another seed -> a training step -> an eval forward on a third batch -> the fixture's parameters ->
    the fixture's step on its first B - 1 images.  That last step equals the same step on a freshly built handle bit for bit, whether the
    first batch had the same size (stale rows overlap completely) or was larger (B: stale rows behind the live ones)."""
    c = load(name)
    B = len(c.labels)
    n2 = B - 1
    assert n2 >= 1
    images, labels = c.images[:n2], c.labels[:n2]
    if (name, dtype) not in _FRESH:
        fresh = build(name, dtype)
        _FRESH[name, dtype] = step(fresh, images, labels)
        fresh.close()
    m = handle(name, dtype)
    try:
        dirty(m, c, n2 if first == "same_size" else B, n2)
        m.set_params(c.params)
        got = step(m, images, labels)
    finally:
        m.set_params(c.params)
    assert_same_step(got, _FRESH[name, dtype], f"{name} {dtype} after a {first} step")


PARITY_LEFTOVER_FIXTURES = ["mudpt_tiny", "coop_tiny_end", "cocoop_tiny", "vpt_tiny", "mpt_tiny", "umudpt_tiny", "uumudpt_tiny"]


@pytest.mark.parametrize("name", PARITY_LEFTOVER_FIXTURES)
def test_parity_handle_leaves_nothing_behind(name):
    """test_step_leaves_nothing_behind on a dtype "fp32" handle, one fixture per variant, with vis_exact_attn flipped 0 -> 1 -> 0 between the
    steps: another seed's step and eval forward under the default, the same under vis_exact_attn = 1 (the vision tower's backward then reads
    the fp16 qkv copy and the lse that attention_exact.hip wrote, not the fp16 kernel's), the knob back at 0, the fixture's parameters, the
    fixture's step on its first B - 1 images.  That step equals the same step on a freshly built fp32 handle bit for bit: a stale qkv_lp or
    lse of the other kernel, or of the larger batch, shows here."""
    c, dtype = load(name), "fp32"
    B = len(c.labels)
    images, labels = c.images[:B - 1], c.labels[:B - 1]
    fresh = build(name, dtype)
    want = step(fresh, images, labels)
    fresh.close()
    m = handle(name, dtype)
    try:
        dirty(m, c, B, B - 1)
        with knobs_set(m, dtype, (("vis_exact_attn", 1),)):
            dirty(m, c, B, B - 1)
        m.set_params(c.params)
        got = step(m, images, labels)
    finally:
        m.set_params(c.params)
    assert_same_step(got, want, f"{name} fp32 after steps under vis_exact_attn 0, 1")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knob", ["attn_window", "lp_grad", "gelu_q8"])
def test_knob_flipped_between_two_steps(knob, dtype):
    """mudpt_model_set between two steps ("gelu_q8: between steps only"): the step after the flip equals the same step on a fresh handle
    built with that setting -- nothing the first step stored in the other form (fp32 / T stream copies, u / 8-bit codes, unwritten dqkv rows)
    reaches it."""
    name = "mudpt_tiny"
    c, value = load(name), 1 - KNOB_DEFAULTS[dtype].get(knob, 1)
    fresh = build(name, dtype, knobs={knob: value})
    want = step(fresh, c.images, c.labels)
    fresh.close()
    m = handle(name, dtype)
    try:
        dirty(m, c, len(c.labels), len(c.labels))
        m.set_params(c.params)
        with knobs_set(m, dtype, ((knob, value),)):
            got = step(m, c.images, c.labels)
    finally:
        m.set_params(c.params)
    assert_same_step(got, want, f"{name} {dtype} {knob} {value} after a default step")
    assert any(not torch.equal(got.grads[k], g) for k, g in run(name, dtype).grads.items()) or knob == "attn_window"


# ---- 4. the caller's stream, and a second handle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["mudpt_tiny", "cocoop_tiny"])  # CoCoOp: its own step, the text tower in chunks behind the vision tower
def test_step_on_a_side_stream(name, dtype):
    """The library forks the text tower onto a stream of its own and joins it with events recorded on the CALLER's stream (model.cpp ev_fork /
    ev_join, ev_fork_b / ev_join_b).  On a side stream that is first kept busy for tens of milliseconds (a chain of 4096^3 matmuls into
    buffers allocated beforehand), the parameters are written and the images copied into a buffer that held other values -- device to
    device, so nothing waits on the host -- and the step runs.  A launch ordered against any other stream reads the old parameters, the old
    images or the previous step's buffers, every time: after side.synchronize() logits, loss and gradients equal the default-stream step
    bit for bit.  The same sequence runs once before with the other inputs: it loads every kernel and fills the stream's allocator pool
    (either may synchronise the device), and leaves another step's values in every buffer.  The premise is asserted: the chain was still
    running when the host had enqueued the whole step.  Four side streams in turn: the runtime maps streams onto a few hardware queues, and
    a launch on a stream that shares the caller's queue is ordered behind the caller's work by the queue itself, which hides the error
    (measured: a launch moved to the null stream went unseen on one stream in four)."""
    c, m = load(name), handle(name, dtype)
    want = run(name, dtype)
    dev = torch.device("cuda")
    other_params, other_images, other_labels = other_inputs(c, len(c.labels), m.n_cls, 0xA)
    inputs = [({k: v.to(dev) for k, v in p.items()}, x.to(dev), y.to(dev)) for p, x, y in ((other_params, other_images, other_labels), (c.params, c.images, c.labels))]
    buf = torch.zeros_like(inputs[0][1])
    a = torch.randn(4096, 4096, device=dev) / 64.0
    x, y = a.clone(), torch.empty_like(a)
    chain_done = torch.cuda.Event()
    torch.cuda.synchronize()
    results = []
    try:
        for side in [torch.cuda.Stream() for _ in range(4)]:
            for params, images, labels in inputs:
                with torch.cuda.stream(side):
                    for _ in range(12):
                        torch.mm(x, a, out=y)
                        torch.mm(y, a, out=x)
                    chain_done.record(side)
                    m.set_params(params)
                    buf.copy_(images)
                    loss, logits = m.forward_backward(buf, labels, return_logits=True)
                    got = (logits.clone(), loss.clone(), {k: g.detach().clone() for k, g in m.grads().items()})
                    still_busy = not chain_done.query()
                side.synchronize()
            assert still_busy, "the side stream had drained before the step was enqueued: the test's premise does not hold on this machine"
            results.append(Step(got[0].cpu(), got[1].item(), {k: g.cpu() for k, g in got[2].items()}))
        assert torch.isfinite(x).all()
    finally:
        torch.cuda.synchronize()
        m.set_params(c.params)
    for i, got in enumerate(results):
        assert_same_step(got, want, f"{name} {dtype} on side stream {i}")


def test_two_handles_step_in_turns():
    """include/mudpt.h: "nothing is process-global: two models in one process do not interfere".  A: tiny, fp16, default knobs.  B: tiny, bf16,
    another max_batch, {attn_two_kernels 1, gemm_variant 1, lp_grad 0}.  Steps A, B, A, B without a device synchronise in between give each
    handle what it gives stepping alone; A alone is measured before B exists, so B's knobs (or dtype) showing in A would move it."""
    name = "mudpt_tiny"
    c = load(name)
    knobs_b = {"attn_two_kernels": 1, "gemm_variant": 1, "lp_grad": 0}
    batches = [(c.images, c.labels), (c.images.flip(0)[:2] * 0.5, c.labels.flip(0)[:2])]
    A = build(name, "fp16")
    alone_a = [step(A, *b) for b in batches]
    assert_same_step(alone_a[0], run(name, "fp16"), "handle A alone vs the module's handle")
    B = build(name, "bf16", max_batch=5, knobs=knobs_b)
    alone_b = [step(B, *b) for b in batches]
    with_knobs = run(name, "bf16", tuple(knobs_b.items()))
    assert_same_step(alone_b[0], with_knobs, "handle B alone vs the module's bf16 handle under B's knobs")
    assert any(not torch.equal(with_knobs.grads[k], g) for k, g in run(name, "bf16").grads.items())  # B's knobs do change B
    dev = torch.device("cuda")
    batches = [(x.to(dev), y.to(dev)) for x, y in batches]
    torch.cuda.synchronize()
    got = {"A": [], "B": []}
    for i in range(2):
        for key, m in (("A", A), ("B", B)):
            loss, logits = m.forward_backward(*batches[i], return_logits=True)
            got[key].append((logits.clone(), loss.clone(), {k: g.detach().clone() for k, g in m.grads().items()}))
    torch.cuda.synchronize()
    for key, alone in (("A", alone_a), ("B", alone_b)):
        for i in range(2):
            lg, ls, gr = got[key][i]
            assert_same_step(Step(lg.cpu(), ls.item(), {k: g.cpu() for k, g in gr.items()}), alone[i], f"handle {key}, step {i}, in turns vs alone")
    A.close()
    B.close()
