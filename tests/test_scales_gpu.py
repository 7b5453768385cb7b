"""The two scale factors of a training step, on every trainer variant.

mudpt_forward_backward runs its backward on per-sample gradients times loss_scale and multiplies by unscale = grad_scale / (B loss_scale) at
every reduction that leaves a tower (model.cpp head_train lists the sites); every data-parallel run passes grad_scale = 1 / world, and
trainer.data_parallel_step halves the loss scale on overflow and doubles it again later.  One tiny fixture per variant reaches every site:
the length buckets (208 classes), CoOp's shared and per-class contexts, VPT with and without deep prompts, MPT with and without vision
prompts, both prompt generators, CoCoOp in more than one chunk, and the class-parallel phases ("mudpt_tiny/cp": forward_backward_cp on an
unsharded handle).

  1. bf16 handles: power-of-two loss scales give the same step bit for bit;
  2. every dtype: logits and loss do not see either factor;
  3. a power-of-two grad_scale multiplies every gradient tensor exactly;
  4. grad_scale 1/3 and loss_scale 96 against each variant's own reference with its own check;
  5. set_loss_scale between two steps leaves nothing of the old scale behind;
  6. fp16-typed handles over every scale the trainer can visit, against the oracle (the table of DESIGN.md 2).

One handle per (fixture, dtype) lives for the whole module; a run under (loss_scale, grad_scale) is computed once and shared."""
import pytest
import torch

from oracle import cocoop_oracle as CO
from oracle import mudpt_oracle as O
from tests import coop_reference as CR
from tests import test_cocoop_gpu as TCC
from tests import test_coop_gpu as TC
from tests import test_exact_gpu as TE
from tests import test_knobs_gpu as TK
from tests import test_umudpt_gpu as TU
from tests import test_uumudpt_gpu as TUU
from tests.helpers import GRAD_COS, GRAD_RMS, GRAD_RTOL, check_fixture_grads, check_grad, check_grads
from tests.test_knobs_gpu import Step, assert_same_step

pytestmark = pytest.mark.gpu
DTYPES = ("bf16", "fp16", "fp32")
CP = "mudpt_tiny/cp"  # the class-parallel phases on an unsharded handle of mudpt_tiny
FIXTURES = ["mudpt_tiny", "mudpt_vitb16_c208_b2", "coop_tiny_middle", "coop_tiny_front_csc", "vpt_tiny", "vpt_tiny_shallow", "mpt_tiny", "mpt_tiny_textonly",
            "umudpt_tiny", "uumudpt_tiny", "cocoop_tiny", CP]
DEFAULT_SCALE = 128.0
POW2_LOSS_SCALES = (1.0, 128.0, 4096.0)
POW2_GRAD_SCALES = (0.5, 0.125)
ODD = ((DEFAULT_SCALE, 1.0 / 3.0), (96.0, 1.0))  # (loss_scale, grad_scale): world size 3; a loss scale that is no power of two

_HANDLES, _RUNS, _KAPPA = {}, {}, {}


def fixture_of(name):
    return name.partition("/")[0]


def build(name, dtype):
    """A new handle on the fixture; CoCoOp with one image per text-tower pass, so that its two reductions run once per chunk."""
    c = TK.load(fixture_of(name))
    if name.startswith("cocoop_"):
        assert len(c.labels) >= 2
        return TK.build(name, dtype, knobs={"cocoop_chunk": 1})
    return TK.build(fixture_of(name), dtype)


def handle(name, dtype):
    if (name, dtype) not in _HANDLES:
        _HANDLES[name, dtype] = build(name, dtype)
    return _HANDLES[name, dtype]


@pytest.fixture(scope="module", autouse=True)
def _module_handles():
    yield
    for m in _HANDLES.values():
        m.close()
    for cache in (_HANDLES, _RUNS, _KAPPA):
        cache.clear()


def step(m, name, grad_scale=1.0):
    c = TK.load(fixture_of(name))
    fb = m.forward_backward_cp if name == CP else m.forward_backward
    loss, logits = fb(c.images, c.labels, grad_scale=grad_scale, return_logits=True)
    return Step(logits.cpu(), loss.item(), {k: g.detach().cpu().clone() for k, g in m.grads().items()})


def run(name, dtype, loss_scale=DEFAULT_SCALE, grad_scale=1.0):
    """The fixture's step on the module's handle under the two factors, computed once; the handle is left at the default scale."""
    key = (name, dtype, loss_scale, grad_scale)
    if key not in _RUNS:
        m = handle(name, dtype)
        m.set_loss_scale(loss_scale)
        try:
            _RUNS[key] = step(m, name, grad_scale)
        finally:
            m.set_loss_scale(DEFAULT_SCALE)
    return _RUNS[key]


# ---- 1. bf16: a power-of-two loss scale commutes with the whole backward --------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_power_of_two_loss_scales_change_nothing(name):
    """Logits, loss and every gradient tensor at loss_scale 1 and 4096 equal the default's (128) bit for bit.  Derived, with or without
    lp_grad: bf16 has fp32's exponent range, so a power-of-two factor commutes with every rounding of a linear backward (even scale 1 leaves
    the token gradients inside that range); loss_scale * B and fl(1 / (B s)) = fl(1 / B) / s are exact; QuickGELU' and the gelu_q8 codes
    come from the forward's u, not from a gradient.  A site that forgets unscale, hard-codes 128 or reads a stale cp_unscale is off by a
    factor of 128 or 32 here."""
    base = run(name, "bf16")
    for s in POW2_LOSS_SCALES:
        assert_same_step(run(name, "bf16", s), base, f"{name} bf16 loss_scale {s:g} vs {DEFAULT_SCALE:g}")


# ---- 2. neither factor reaches the forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_logits_and_loss_ignore_both_factors(name, dtype):
    """The loss is the plain mean over the batch and the logits are the forward's: bit-identical under every loss scale and every grad_scale
    of this module (an fp16 backward may flush or overflow at the extreme scales; the forward may not notice)."""
    base = run(name, dtype)
    for ls, gs in [(s, 1.0) for s in POW2_LOSS_SCALES] + [(DEFAULT_SCALE, g) for g in POW2_GRAD_SCALES] + list(ODD):
        got = run(name, dtype, ls, gs)
        assert torch.equal(got.logits, base.logits) and got.loss == base.loss, (name, dtype, ls, gs, (got.logits - base.logits).abs().max().item(), got.loss - base.loss)


# ---- 3. grad_scale enters through unscale alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_power_of_two_grad_scale_multiplies_every_gradient_exactly(name, dtype):
    """grad_scale 1/2 and 1/8 (world sizes 2 and 8): every gradient tensor equals grad_scale times the grad_scale = 1 result bit for bit --
    the factor enters only through unscale = grad_scale / (B loss_scale), a power-of-two multiple of the default's, and everything behind the
    reductions is fp32 and linear.  A site that applies it twice, or not at all, is off by the factor."""
    base = run(name, dtype)
    for gs in POW2_GRAD_SCALES:
        got = run(name, dtype, DEFAULT_SCALE, gs)
        want = Step(base.logits, base.loss, {k: g * gs for k, g in base.grads.items()})
        assert_same_step(got, want, f"{name} {dtype} grad_scale {gs:g}")


# ---- 4. factors that are no powers of two, against each variant's reference ----------------------------------------------------------------------
def _coop_kappa(c):
    if c.name not in _KAPPA:
        taps = {}
        CR.forward_backward(c.cfg, c.frozen, c.ctx, c.class_embedding, c.eot, c.name_lens, c.position, c.images, c.labels, taps)
        _KAPPA[c.name] = TC.kappa(c, taps["dprompts"])
    return _KAPPA[c.name]


def _cocoop_kappa(name, c):
    if name not in _KAPPA:
        taps = {}
        CO.forward_backward(c.cfg, c.frozen, c.params, c.class_embedding, c.eot, c.images, c.labels, taps)
        _KAPPA[name] = TCC.cancellation_factors(c.cfg, taps["dprompts"])
    return _KAPPA[name]


def mudpt_figures(grads, ref, factor=1.0):
    """Per tensor (max error / rms, rms error / rms, cosine) against factor * the oracle's gradient."""
    out = {}
    for k in O.TRAINABLE_ORDER:
        r, g = ref[k] * factor, grads[k]
        rms = max(r.pow(2).mean().sqrt().item(), 1e-30)
        out[k] = ((g - r).abs().max().item() / rms, (g - r).pow(2).mean().sqrt().item() / rms,
                  torch.nn.functional.cosine_similarity(g.flatten().double(), r.flatten().double(), dim=0).item())
    return out


def worst(figures):
    return max(f[0] for f in figures.values()), max(f[1] for f in figures.values()), min(f[2] for f in figures.values())


def check_against_reference(name, grade, grads, factor, tag):
    """The variant suite's own gradient check with the constants of `grade`, against its reference times `factor`."""
    fx = fixture_of(name)
    c = TK.load(fx)
    if fx.startswith("mudpt_"):  # test_model_gpu.py::test_loss_and_grads_match_reference
        if fx == "mudpt_vitb16_c208_b2":  # against the fixture (the reference's own autograd; the three big weights as their [::8, ::8] samples): no 208-class oracle pass on the CPU
            stored = {k: c.grad(k) if c.grad(k) is not None else c.grad_sample(k) for k in O.TRAINABLE_ORDER}
            grads, ref = {k: grads[k] if c.grad(k) is not None else grads[k][::8, ::8] for k in O.TRAINABLE_ORDER}, stored
        else:
            ref = TK.oracle_grads(fx)
        for k, (emax, erms, cos) in mudpt_figures(grads, ref, factor).items():
            print(f"{tag} {k}: max err {emax:.3e} x rms, rms err {erms:.3e} x rms, cos {cos:.6f}")
            assert emax <= 4 * GRAD_RTOL[grade] + 1e-9 and erms <= GRAD_RMS[grade] and cos > GRAD_COS[grade], (tag, k, emax, erms, cos)
    elif fx.startswith("coop_"):  # test_coop_gpu.py::test_logits_loss_grads_match_reference
        got, ref = grads[CR.CTX], c.dctx * factor
        rms_g, gmax = ref.pow(2).mean().sqrt().item(), ref.abs().max().item()
        e, er = (got - ref).abs().max().item(), (got - ref).pow(2).mean().sqrt().item()
        print(f"{tag} d ctx: rms err {er / rms_g:.3e} max err / rms {e / rms_g:.3e}")
        if c.csc:
            assert er <= TC.GRAD_RMS[grade] * rms_g + 1e-12 and e <= 4 * TC.GRAD_RTOL[grade] * rms_g + 1e-9, (tag, er / rms_g, e / rms_g)
        else:
            bound = TC.DELTA_T[grade] * _coop_kappa(c)
            assert er <= bound * rms_g + 1e-12 and e <= 4 * bound * gmax + 1e-9, (tag, er / rms_g, e / gmax, bound)
    elif fx.startswith(("vpt_", "mpt_")):
        check_grads(grads, {k: r * factor for k, r in c.grads.items()}, grade, tag)
    elif fx.startswith(("umudpt_", "uumudpt_")):  # pieces (a) and (c) of the suites' parity test; (b) does not depend on the towers' type
        mod = TU if fx.startswith("umudpt_") else TUU
        restated = mod.restated(c)[2]
        tables = (TU.R.CTX, TU.R.DEEP) if mod is TU else (TUU.R.CTX, TUU.R.DEEP, TUU.R.VCTX, TUU.R.VDEEP)
        for k in tables:
            if grads[k].numel():
                check_grad(grads[k], restated[k] * factor, grade, f"{tag} (a) {k}")
        check_fixture_grads(grads, c, grade, f"{tag} (c)", factor)
    else:  # test_cocoop_gpu.py::test_logits_loss_grads_match_reference
        kappa = _cocoop_kappa(fx, c)
        for k in CO.TRAINABLE_ORDER:
            r = c.grad(k) * factor
            rms_g, gmax = r.pow(2).mean().sqrt().item(), r.abs().max().item()
            e, er = (grads[k] - r).abs().max().item(), (grads[k] - r).pow(2).mean().sqrt().item()
            bound = TCC.DELTA_T[grade] * kappa.get(k, kappa["meta"])
            print(f"{tag} {k}: rms err {er / rms_g:.3e} (bound {bound:.3e}) max err / max|g| {e / gmax:.3e}")
            assert er <= bound * rms_g + 1e-9 and e <= 4 * bound * gmax + 1e-9, (tag, k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_odd_factors_match_the_reference(name, dtype):
    """grad_scale = 1/3 (three ranks) and loss_scale = 96: the setter takes any positive finite value, and nothing in the step may assume a
    power of two.  Each variant's own check against its own reference (the oracle, the restatement, the fixture) times grad_scale, with the
    handle dtype's constants; a parity-mode handle (an fp16-typed backward with lp_grad = 1) is graded with the bf16 row, as
    test_knobs_gpu.py grades lp_grad = 1 on an fp16 handle."""
    grade = "bf16" if dtype == "fp32" else dtype
    for ls, gs in ODD:
        got = run(name, dtype, ls, gs)
        assert all(torch.isfinite(g).all() for g in got.grads.values())
        check_against_reference(name, grade, got.grads, gs, f"{name} {dtype} loss_scale {ls:g} grad_scale {gs:.4f}")


# ---- 5. set_loss_scale between two steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIXTURES)
def test_set_loss_scale_between_two_steps(name, dtype):
    """A step at 128, set_loss_scale(32), a second step: it equals the first step of a fresh handle built at scale 32 bit for bit -- on a
    bf16 handle also the default-scale step (identity 1).  The class-parallel phases take their unscale from the mudpt_cp_head of the
    step in flight; one kept from the previous step shows as a factor of 4."""
    fresh = build(name, dtype)
    fresh.set_loss_scale(32.0)
    want = step(fresh, name)
    fresh.close()
    m = handle(name, dtype)  # run() leaves it at 128
    step(m, name)
    m.set_loss_scale(32.0)
    try:
        got = step(m, name)
    finally:
        m.set_loss_scale(DEFAULT_SCALE)
    assert_same_step(got, want, f"{name} {dtype} at 32 after a step at 128 vs a fresh handle at 32")
    if dtype == "bf16":
        assert_same_step(got, run(name, dtype), f"{name} bf16 at 32 after a step at 128 vs the default step")


# ---- 6. the scales the trainer can visit, on fp16-typed handles ----------------------------------------------------------------------------------
VISITED = [DEFAULT_SCALE * 2.0 ** k for k in range(-7, 4)]  # 1 (trainer.LOSS_SCALE_MIN) .. 1024
# (max error / rms, rms error / rms, cosine floor) per handle dtype at 16 .. 1024 -- the default, three halvings (a run recovers from each
# only after LOSS_SCALE_GROWTH_INTERVAL clean steps) and three doublings: the handle dtype's own constants.  fp16: tests/helpers.py.  fp32:
# the bound and the cosine floor test_exact_gpu.py::test_logits_at_scale_100_within_1e_3 holds its gradients to, and the bf16 row's RMS
# bound (the mode runs lp_grad = 1).  Below 16 the step is still taken, so it must still be a usable gradient: the bf16 row.
NEAR = {"fp16": (4 * GRAD_RTOL["fp16"], GRAD_RMS["fp16"], GRAD_COS["fp16"]), "fp32": (4 * TE.GRAD_RTOL, GRAD_RMS["bf16"], 0.9995)}
FAR = (4 * GRAD_RTOL["bf16"], GRAD_RMS["bf16"], GRAD_COS["bf16"])
# What an MI355X measures, worst tensor against the oracle: scale -> (max error / rms, rms error / rms, cosine); the table of DESIGN.md 2
# (the worse of mudpt_tiny and mudpt_vitb16_b4).  Below 4 the fp16 copies of the token gradients start to lose bits to the subnormal range;
# scale 1 still gives a gradient inside the bf16 row, so trainer.LOSS_SCALE_MIN = 1 stands.
VISITED_MEASURED = {
    "fp16": {1: (4.42e-2, 6.24e-3, 0.999981), 2: (2.21e-2, 3.31e-3, 0.999995), 4: (1.69e-2, 2.17e-3, 0.999998), 8: (1.69e-2, 2.15e-3, 0.999998),
             16: (1.97e-2, 2.19e-3, 0.999998), 32: (1.78e-2, 2.10e-3, 0.999998), 64: (1.67e-2, 2.10e-3, 0.999998), 128: (1.79e-2, 2.10e-3, 0.999998),
             256: (1.76e-2, 2.10e-3, 0.999998), 512: (1.74e-2, 2.10e-3, 0.999998), 1024: (1.74e-2, 2.10e-3, 0.999998)},
    "fp32": {1: (5.00e-2, 6.93e-3, 0.999976), 2: (3.46e-2, 3.54e-3, 0.999994), 4: (3.17e-2, 3.04e-3, 0.999995), 8: (2.65e-2, 2.90e-3, 0.999996),
             16: (2.82e-2, 3.04e-3, 0.999995), 32: (2.92e-2, 2.96e-3, 0.999996), 64: (3.22e-2, 3.19e-3, 0.999995), 128: (3.22e-2, 3.17e-3, 0.999995),
             256: (2.94e-2, 3.16e-3, 0.999995), 512: (2.78e-2, 3.18e-3, 0.999995), 1024: (2.84e-2, 3.19e-3, 0.999995)},
}


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("name", ["mudpt_tiny", "mudpt_vitb16_b4"])
def test_loss_scales_the_trainer_can_visit(name, dtype):
    """One step at every scale trainer.data_parallel_step can reach from the default, 128 * 2^k for k = -7 (LOSS_SCALE_MIN) .. +3, against
    the oracle: the worst tensor's max error / rms, rms error / rms and cosine are printed per scale (DESIGN.md 2 holds the table), then
    asserted: NEAR at 16 .. 1024, FAR below.  A scale the trainer can reach that fails FAR means it steps on flushed gradients."""
    ref, rows, bad = TK.oracle_grads(name), [], []
    for s in VISITED:
        got = run(name, dtype, s)
        emax, erms, cos = worst(mudpt_figures(got.grads, ref))
        finite = all(torch.isfinite(g).all().item() for g in got.grads.values())
        rows.append(f"| {s:g} | {emax:.2e} | {erms:.2e} | {cos:.6f} |")
        bmax, brms, bcos = NEAR[dtype] if s >= 16 else FAR
        if not (finite and emax <= bmax + 1e-9 and erms <= brms and cos > bcos):
            bad.append((s, emax, erms, cos, finite))
    # the setter reaches the backward: at scale 1 the fp16 token gradients round differently (a setter the step ignored would pass every identity)
    assert any(not torch.equal(run(name, dtype, 1.0).grads[k], g) for k, g in run(name, dtype).grads.items())
    print(f"{name} {dtype}\n| loss scale | max err / rms | rms err / rms | cosine |\n|---|---|---|---|\n" + "\n".join(rows))
    assert not bad, (name, dtype, bad)
