"""The LayerNorm checks of test_layernorm_gpu.py can fail, shown without a GPU: the checker that the GPU test runs over the HIP kernels'
results (tests/helpers.py: ln_regimes, ln64, ln_bounds, ln_bwd_bounds, ln_check) runs here over fp32 restatements in torch.  The faithful
two-pass restatement has to stay under HALF of every bound in every regime at every width; each wrong variant has to exceed a bound, in the
regime named beside it, at every width (EXCEPTIONS lists the widths where a variant is too close to the definition to tell).  On the plain
regime alone -- the only data the older LayerNorm tests use -- a kernel with eps = 1e-6 or with a one-pass variance passes their 2e-5 check."""
import pytest
import torch

from tests.helpers import (EPS, LN_EPS, LN_REGIMES, LN_ROWS_PER_REGIME, LN_WIDTHS, ln64, ln_bounds, ln_bwd64, ln_bwd_bounds, ln_groups, ln_operands,
                           ln_ratios, ln_regimes, ln_stats32)

TT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def truncate_to(y, dtype):
    """fp32 -> T towards zero instead of to nearest."""
    if dtype == "bf16":
        return (y.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    h = y.to(torch.float16)
    over = h.float().abs() > y.abs()  # rounded away from zero: one step back (the fp16 codes of one sign ascend with the magnitude)
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)


def forward32(x, gamma, beta, variant="faithful"):
    """fp32 restatement of ln_fwd_kernel, or a wrong variant of it: mean, rstd [rows, 1], y fp32 and y in both T."""
    d = x.shape[-1]
    eps = {"eps_1e-6": 1e-6, "eps_0": 0.0}.get(variant, LN_EPS)
    mean = x.sum(-1, keepdim=True) / d
    c = x - mean
    if variant == "one_pass":
        var = (x * x).sum(-1, keepdim=True) / d - mean * mean
    else:
        var = (c * c).sum(-1, keepdim=True) / (d - 1 if variant == "unbiased" else d)
    rstd = 1.0 / (var.sqrt() + eps) if variant == "eps_after_sqrt" else torch.rsqrt(var + eps)
    y = c * rstd * gamma + beta
    cast = truncate_to if variant == "truncate" else (lambda v, dt: v.to(TT[dt]))
    return {"mean": mean, "rstd": rstd, "y": y, "y_bf16": cast(y, "bf16"), "y_fp16": cast(y, "fp16")}


def backward32(x, gamma, dy, dres, mean, rstd, variant="faithful"):
    """fp32 restatement of ln_bwd_kernel (mean, rstd: fp32 [rows, 1]), or a wrong variant: dx fp32 and in both T."""
    d = x.shape[-1]
    n = d - 1 if variant == "bwd_d_minus_1" else d
    xh = (x - mean) * rstd
    g = dy * gamma
    c1, c2 = g.sum(-1, keepdim=True) / n, (g * xh).sum(-1, keepdim=True) / n
    if variant == "bwd_no_mean_g":
        c1 = torch.zeros_like(c1)
    dx = rstd * (g - c1 - xh * c2) + dres
    dgamma, dbeta = torch.zeros(d), torch.zeros(d)
    for r in range(x.shape[0]):  # ln_bwd_affine_kernel: one thread per column, rows in order
        dgamma, dbeta = dgamma + dy[r] * xh[r], dbeta + dy[r]
    return {"dx": dx, "dx_bf16": dx.to(torch.bfloat16), "dx_fp16": dx.to(torch.float16), "dgamma": dgamma, "dbeta": dbeta}


def case(d):
    g = torch.Generator().manual_seed(1000 + d)
    x = ln_regimes(LN_ROWS_PER_REGIME, d, g)
    gamma, beta, dy, dres = ln_operands(x.shape[0], d, g)
    ref = ln64(x, gamma, beta)
    bref = ln_bwd64(ref, gamma, dy, dres)
    return x, gamma, beta, dy, dres, ref, bref


def ratios(d, variant, fp32_share=1.0):
    """{quantity: worst error / bound per regime} of a variant at width d, every quantity the GPU test checks.  fp32_share: the T bounds
    (fp32 bound + rounding to T) with only that share of their fp32 part."""
    x, gamma, beta, dy, dres, ref, bref = case(d)
    groups = ln_groups()
    f = forward32(x, gamma, beta, variant)
    mean32, rstd32 = ln_stats32(ref)
    b = backward32(x, gamma, dy, dres, mean32.unsqueeze(-1), rstd32.unsqueeze(-1), variant)
    fb, bb = ln_bounds(ref, gamma), ln_bwd_bounds(ref, bref, dy)
    out = {"mean": ln_ratios(f["mean"], ref.mean, fb["mean"], groups), "rstd": ln_ratios(f["rstd"], ref.rstd, fb["rstd"], groups),
           "y": ln_ratios(f["y"], ref.y, fb["y"], groups), "dx": ln_ratios(b["dx"], bref.dx, bb["dx"], groups)}
    if variant == "faithful":  # the affine gradients, one ratio each (a column sums over every regime)
        out["dgamma"], out["dbeta"] = (ln_ratios(b[k], getattr(bref, k), bb[k]).reshape(1) for k in ("dgamma", "dbeta"))
    for dt in ("bf16", "fp16"):
        out["y_" + dt] = ln_ratios(f["y_" + dt], ref.y, ln_bounds(ref, gamma, dt)["y"] - (1 - fp32_share) * fb["y"], groups)
        out["dx_" + dt] = ln_ratios(b["dx_" + dt], bref.dx, ln_bwd_bounds(ref, bref, dy, dt)["dx"] - (1 - fp32_share) * bb["dx"], groups)
    return out


@pytest.mark.parametrize("d", LN_WIDTHS)
def test_faithful_restatement_stays_under_half_of_every_bound(d):
    """Half of every fp32 bound.  A T bound is the fp32 bound plus half an ulp of T, which correct rounding attains: there the restatement has
    to stay inside half of the fp32 part plus that rounding term (ratios(..., fp32_share=0.5))."""
    for what, r in ratios(d, "faithful", fp32_share=0.5).items():
        print(f"d = {d} {what}: " + " ".join(f"{n} {v:.3f}" for n, v in zip(LN_REGIMES if len(r) > 1 else ("all",), r.tolist())))
        assert (r <= (1.0 if what[-4:] in ("bf16", "fp16") else 0.5)).all(), (d, what, r.tolist())


# variant -> (the quantity and the regime that catch it at every width, widths excepted)
CAUGHT_BY = {
    "eps_1e-6": ("rstd", "eps_dominates"),          # rstd = 1 / sqrt(1e-6 + 1e-6) instead of 1 / sqrt(1e-6 + 1e-5): 2.3 x
    "eps_0": ("rstd", "zero"),                      # 1 / sqrt(0): infinite, y = 0 * inf
    "unbiased": ("rstd", "plain"),                  # sqrt((d - 1) / d): 1 / (2 d) relative, 5e-4 at d = 1024 against 16 u = 1e-6
    "one_pass": ("rstd", "offset"),                 # E[x^2] = 9e4 carries an ulp of 8e-3; the variance is 2.5e-3
    "eps_after_sqrt": ("rstd", "zero"),             # 1 / (0 + 1e-5) = 1e5 instead of 316
    "truncate": ("y_bf16", "plain"),                # up to 2 EPS |y| where EPS |y| is allowed
    "bwd_no_mean_g": ("dx", "zero"),                # dx = rstd (g - mean(g)) there: the whole term, 316 mean(g), is missing
    # both means off by 1 / (d - 1).  At d = 1024 that is 1e-3 of terms that are a few per cent of the gradient: 1.3 x the bound, on the
    # plain regime only (everywhere else the gradient is rstd-times larger and so is the bound)
    "bwd_d_minus_1": ("dx", "plain"),
}
# (variant, d) where the variant stays inside every bound, with the reason
EXCEPTIONS = {}


@pytest.mark.parametrize("d", LN_WIDTHS)
@pytest.mark.parametrize("variant", sorted(CAUGHT_BY))
def test_wrong_variant_fails_the_checks(variant, d):
    what, regime = CAUGHT_BY[variant]
    r = ratios(d, variant)
    worst = {k: v.max().item() for k, v in r.items()}
    print(f"{variant} d = {d}: worst error / bound {worst}")
    if (variant, d) in EXCEPTIONS:
        assert max(worst.values()) <= 1.0, "no longer an exception: take it off the list"
        return
    assert r[what][LN_REGIMES.index(regime)].item() > 1.0, (variant, d, what, regime, r[what].tolist())
    if variant == "truncate":  # fp16 as well
        assert r["y_fp16"][LN_REGIMES.index(regime)].item() > 1.0


@pytest.mark.parametrize("d", LN_WIDTHS)
@pytest.mark.parametrize("variant", ["eps_1e-6", "one_pass"])
def test_the_old_check_on_plain_data_misses_eps_and_one_pass(variant, d):
    """The gap: test_layernorm_fwd_bwd's fp32 check (atol 2e-5, rtol 1e-5 on randn * 2 + 0.5) accepts both."""
    x, gamma, beta, _, _, ref, _ = case(d)
    rows = slice(0, LN_ROWS_PER_REGIME)
    y = forward32(x[rows], gamma, beta, variant)["y"]
    torch.testing.assert_close(y.double(), ref.y[rows], atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("lo_mode", [1, 2])
@pytest.mark.parametrize("d", LN_WIDTHS)
def test_faithful_split_pair_stays_inside_its_bound(d, lo_mode, dtype):
    """hi = T(y), lo = T(y - hi) or e4m3((y - hi) 2^12) saturating at 448, as common.h's split_rem / pack_lo8: hi + lo within half the fp32
    bound plus the remainder's rounding."""
    x, gamma, beta, _, _, ref, _ = case(d)
    y = forward32(x, gamma, beta)["y"]
    hi = y.to(TT[dtype])
    rem = y - hi.float()
    lo = rem.to(TT[dtype]).double() if lo_mode == 1 else (rem * 4096).clamp(-448, 448).to(torch.float8_e4m3fn).float().double() / 4096
    bound = ln_bounds(ref, gamma, dtype, lo_mode, hi=hi)["y"] - 0.5 * ln_bounds(ref, gamma)["y"]
    r = ln_ratios(hi.double() + lo, ref.y, bound, ln_groups())
    print(f"d = {d} {dtype} lo_mode {lo_mode}: " + " ".join(f"{n} {v:.3f}" for n, v in zip(LN_REGIMES, r.tolist())))
    assert (r <= 1.0).all()
    # and a pair whose low half is dropped fails
    assert (ln_ratios(hi.double(), ref.y, bound, ln_groups()) > 1.0).any()


def test_truncation_helper_truncates():
    y = torch.tensor([1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 1.0 + 3 * 2.0 ** -12, 0.3, -0.3, 2.0])
    for dt in ("bf16", "fp16"):
        t = truncate_to(y, dt).float()
        assert (t.abs() <= y.abs()).all() and ((y - t).abs() < 4 * EPS[dt] * y.abs()).all()
        assert t[5] == 2.0 and (truncate_to(t, dt).float() == t).all()
