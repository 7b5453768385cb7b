"""The LayerNorm kernels (layernorm.hip, promptgen.hip's ln_bwd_affine) against float64 from the definition, on the inputs where a LayerNorm
goes wrong and the older tests have none: seven regimes in one 35-row launch (helpers.ln_regimes: plain, a mean 6000 standard deviations
from zero, variances below and near eps, constant rows, outliers, zeros), widths that fill one lane, a few lanes, part of the last 64-lane
slab at every k and the whole register file, every row stride different from d and from every other one between NaN (operands) and
sentinel (results) guards, every forward and backward form of the launchers, saved statistics on every forward, T results held to correct
rounding, and two runs of every launch bit for bit.  The bounds (helpers.ln_bounds, ln_bwd_bounds) are derived from the fp32 format and
the reference's own conditioning, not from a kernel; tests/test_layernorm_cpu.py shows without a GPU that they reject a wrong eps, an
unbiased or one-pass variance, truncation and two wrong backwards.

Measured on an MI355X: the kernels' worst |error| / bound over every case of this file, by regime (the module prints this table when it
ends; run with -s).  "all": the one-row cases and the column sums, which have no regime.  The fused cases count a row under the regime it
had before the splice.  The T rows are near 1 because their bound is half an ulp of T, which correct rounding attains; their fp32 part is
the `y` / `dx` row.  Nothing exceeded a bound, so no constant was widened and no kernel changed.

    quantity        plain  offset  eps_dominates  var_near_eps  constant  outliers   zero    all
    mean            0.103   0.152          0.121         0.132     0.103     0.004  0.103  0.066
    rstd            0.082   0.021          0.082         0.082     0.082     0.139  0.082  0.096
    y               0.103   0.151          0.098         0.116     0.103     0.007  0.103      -
    y_bf16          0.975   0.526          0.926         0.922     0.913     0.922  0.922  0.911
    y_fp16          0.922   0.213          0.805         0.805     0.650     0.805  0.805  0.672
    pair_bf16_lo1   0.155   0.150          0.101         0.119     0.068     0.153  0.062      -
    pair_bf16_lo2   0.430   0.155          0.279         0.266     0.234     0.355  0.344      -
    pair_fp16_lo1   0.009   0.151          0.098         0.110     0.068     0.007  0.001      -
    pair_fp16_lo2   0.241   0.150          0.145         0.122     0.089     0.158  0.113      -
    dx              0.006   0.024          0.003         0.012     0.002     0.009  0.005  0.003
    dx_bf16         0.985   0.348          0.940         0.883     0.964     0.990  0.978  0.980
    dx_fp16         0.917   0.057          0.738         0.548     0.783     0.954  0.900  0.936
    affine_dx       0.005   0.024          0.003         0.012     0.002     0.004  0.004  0.003
    dgamma              -       -              -             -         -         -      -  0.047
    dbeta               -       -              -             -         -         -      -  0.064
"""
import functools

import pytest
import torch

from mudpt_amd import capi
from tests.helpers import (LN_NO_PADS, LN_PADS, LN_REGIMES, LN_ROWS_PER_REGIME, LN_WIDTHS, SENT, LnRef, ln64, ln_bounds, ln_bwd64, ln_bwd_bounds,
                           ln_check, ln_groups, ln_operands, ln_regimes, ln_stats32, ok)

pytestmark = pytest.mark.gpu

DT = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16)}
ROWS = len(LN_REGIMES) * LN_ROWS_PER_REGIME
LAYOUTS = [(d, False) for d in LN_WIDTHS] + [(260, True), (772, True)]
LAYOUT_IDS = [f"d{d}" + ("-strided" if s else "") for d, s in LAYOUTS]
SPLICE = (2, 3, 7)  # (row0, n, L): rows 2..4 of every 7-row sequence, five sequences in 35 rows
WORST = {}          # (quantity, regime) -> worst error / bound over the module


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield capi.load()
    names = sorted({k[0] for k in WORST})
    print("\nworst error / bound over this module, by regime:\n" + "quantity".ljust(14) + " ".join(n.rjust(14) for n in LN_REGIMES + ("all",)))
    for q in names:
        print(q.ljust(14) + " ".join((f"{WORST[(q, n)]:.3f}" if (q, n) in WORST else "-").rjust(14) for n in LN_REGIMES + ("all",)))


@functools.lru_cache(maxsize=None)
def case(d):
    """x (the regimes), gamma, beta, dy, dres and the float64 forward of one width: computed once, shared, never written."""
    g = torch.Generator().manual_seed(2000 + d)
    x = ln_regimes(LN_ROWS_PER_REGIME, d, g)
    gamma, beta, dy, dres = ln_operands(ROWS, d, g)
    return x, gamma, beta, dy, dres, ln64(x, gamma, beta)


def pads_of(strided):
    return LN_PADS if strided else LN_NO_PADS


# ---- guarded device buffers: one guard row behind every matrix, three guard elements behind every vector ----
def dev_in(t, pad=0):
    """t [rows, d] inside a [rows + 1, d + pad] buffer of NaN."""
    rows, d = t.shape
    buf = torch.full((rows + 1, d + pad), float("nan"), dtype=t.dtype)
    buf[:rows, :d] = t
    return buf.cuda()


def vec_in(v):
    return torch.cat([v, torch.full((3,), float("nan"), dtype=v.dtype)]).cuda()


def dev_out(rows, d, pad=0, dtype=torch.float32):
    return torch.full((rows + 1, d + pad), SENT, dtype=dtype, device="cuda")


def vec_out(n):
    return torch.full((n + 3,), SENT, device="cuda")


def take(buf, rows, d, written=None):
    """The [rows, d] window of a dev_out buffer; everything else -- and the rows outside `written` -- must still hold the sentinel."""
    c = buf.cpu()
    assert (c[:rows, d:] == SENT).all() and (c[rows:] == SENT).all(), "a write outside the result's rows or columns"
    if written is not None:
        rest = torch.ones(rows, dtype=torch.bool)
        rest[written] = False
        assert (c[:rows][rest] == SENT).all(), "a write to a row that the row list does not name"
    return c[:rows, :d].contiguous()


def take_vec(buf, n):
    c = buf.cpu()
    assert (c[n:] == SENT).all(), "a write behind the end of a vector"
    return c[:n].contiguous()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def rows_of(ref, idx):
    return LnRef(*(t[idx] for t in ref))


# ---- forward ----
def run_fwd(lib, export, dtype, d, pads, x, gamma, beta, rows=None, out_f32=False, lo_mode=0, add=None, add_lp=None, ov=None, xout=False, row_index=None, stats=True):
    """One launch of a forward export between guards; returns the results' windows on the host (lo: T values, or the e4m3 codes as uint8)."""
    dt, tt = DT[dtype]
    rows = x.shape[0] if rows is None else rows
    ldo = d + pads["out"]
    xc, gc, bc = dev_in(x, pads["x"]), vec_in(gamma), vec_in(beta)
    out = dev_out(rows, d, pads["out"], torch.float32 if out_f32 else tt)
    lo = dev_out(rows, d, pads["out"], tt) if lo_mode == 1 else torch.full((rows + 1, 2 * ldo), 0x5A, dtype=torch.uint8, device="cuda") if lo_mode == 2 else None
    mean, rstd = (vec_out(rows), vec_out(rows)) if stats else (None, None)
    ac = None if add is None else dev_in(add, pads["add"])
    alp = None if add_lp is None else dev_in(add_lp, pads["add"])
    oc = None if ov is None else dev_in(ov)
    xo = dev_out(rows, d, pads["xout"]) if xout else None
    ic = None if row_index is None else row_index.to(torch.int32).cuda()
    kw = dict(dtype=dt, x=xc, ldx=d + pads["x"], gamma=gc, beta=bc, out=out, ldo=ldo, rows=rows, d=d)
    if export != "mudpt_layernorm_fwd_split":
        kw.update(out_f32=int(out_f32), mean=mean, rstd=rstd)
    if export in ("mudpt_layernorm_fwd", "mudpt_layernorm_fwd_ex"):
        kw.update(row_index=ic)
    if export in ("mudpt_layernorm_fwd_split", "mudpt_layernorm_fwd_ex"):
        kw.update(out_lo=lo, lo_mode=lo_mode)
    if export in ("mudpt_layernorm_fwd_fused", "mudpt_layernorm_fwd_ex"):
        kw.update(add=ac, add_lp=alp, ldadd=d + pads["add"], ov_rows=oc, ov_row0=SPLICE[0], ov_n=SPLICE[1], ov_L=SPLICE[2], xout=xo, ldxout=d + pads["xout"])
    ok(lib, capi.call(export, **kw))
    res = {"out": take(out, rows, d)}
    if lo_mode == 1:
        res["lo"] = take(lo, rows, d)
    elif lo_mode == 2:  # rows of 2 ldo bytes: d codes, then bytes d .. 2 ldo untouched
        c = lo.cpu()
        assert (c[:rows, d:] == 0x5A).all() and (c[rows:] == 0x5A).all(), "a write outside the e4m3 codes"
        res["lo"] = c[:rows, :d].contiguous()
    if stats:
        res["mean"], res["rstd"] = take_vec(mean, rows), take_vec(rstd, rows)
    if xout:
        res["xout"] = take(xo, rows, d)
    return res


def check_stats(tag, res, ref, gamma, groups):
    b = ln_bounds(ref, gamma)
    ln_check(tag, "mean", res["mean"], ref.mean, b["mean"], groups, record=WORST)
    ln_check(tag, "rstd", res["rstd"], ref.rstd, b["rstd"], groups, record=WORST)


def check_y(tag, dtype, res, ref, gamma, groups, out_f32=False, lo_mode=0):
    if lo_mode:
        lo = res["lo"].double() if lo_mode == 1 else res["lo"].view(torch.float8_e4m3fn).float().double() / 4096.0
        bound = ln_bounds(ref, gamma, dtype, lo_mode, hi=res["out"])["y"]
        ln_check(tag, f"pair_{dtype}_lo{lo_mode}", res["out"].double() + lo, ref.y, bound, groups, record=WORST)
    what, bound = ("y", ln_bounds(ref, gamma)["y"]) if out_f32 else ("y_" + dtype, ln_bounds(ref, gamma, dtype)["y"])
    assert res["out"].dtype == (torch.float32 if out_f32 else DT[dtype][1])
    ln_check(tag, what, res["out"], ref.y, bound, groups, record=WORST)


def assert_same_results(a, b, keys=None):
    for k in keys or a:
        assert same_bits(a[k], b[k]), f"{k}: two launches differ"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("d,strided", LAYOUTS, ids=LAYOUT_IDS)
def test_forward_plain_and_split(lib, dtype, d, strided):
    """T output, fp32 output and the split pair in both forms: each against float64 with the statistics, the T output bit for bit the same
    whether or not a low half is written beside it, each launch twice (the second through the narrower export of the same launcher)."""
    x, gamma, beta, _, _, ref = case(d)
    pads, groups, tag = pads_of(strided), ln_groups(), f"fwd {dtype} d={d}{' strided' if strided else ''}"
    t = run_fwd(lib, "mudpt_layernorm_fwd_ex", dtype, d, pads, x, gamma, beta)
    check_stats(tag + " T", t, ref, gamma, groups)
    check_y(tag + " T", dtype, t, ref, gamma, groups)
    assert_same_results(t, run_fwd(lib, "mudpt_layernorm_fwd", dtype, d, pads, x, gamma, beta))
    f = run_fwd(lib, "mudpt_layernorm_fwd_ex", dtype, d, pads, x, gamma, beta, out_f32=True)
    check_stats(tag + " f32", f, ref, gamma, groups)
    check_y(tag + " f32", dtype, f, ref, gamma, groups, out_f32=True)
    assert_same_results(f, run_fwd(lib, "mudpt_layernorm_fwd", dtype, d, pads, x, gamma, beta, out_f32=True))
    assert same_bits(f["mean"], t["mean"]) and same_bits(f["rstd"], t["rstd"])
    for lo_mode in (1, 2):
        s = run_fwd(lib, "mudpt_layernorm_fwd_ex", dtype, d, pads, x, gamma, beta, lo_mode=lo_mode)
        check_stats(f"{tag} lo{lo_mode}", s, ref, gamma, groups)
        check_y(f"{tag} lo{lo_mode}", dtype, s, ref, gamma, groups, lo_mode=lo_mode)
        assert same_bits(s["out"], t["out"]), "the high half is not the plain T output"
        assert_same_results(run_fwd(lib, "mudpt_layernorm_fwd_split", dtype, d, pads, x, gamma, beta, lo_mode=lo_mode, stats=False), s, keys=("out", "lo"))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("add_kind", ["f32", "lp"])
@pytest.mark.parametrize("d,strided", LAYOUTS, ids=LAYOUT_IDS)
def test_forward_fused_add_splice_xout(lib, dtype, add_kind, d, strided):
    """v = x + add (fp32 addend with a T output, T addend with an fp32 output), rows 2..4 of every 7 replaced by prompt rows, v saved bit for
    bit.  x is the regimes minus the addend, so that v has the regimes' statistics; the prompt rows are an offset, an outlier and a zero row."""
    tt = DT[dtype][1]
    x0, gamma, beta, _, _, _ = case(d)
    g = torch.Generator().manual_seed(3000 + d)
    add = torch.randn(ROWS, d, generator=g) * 0.5
    add = add if add_kind == "f32" else add.to(tt)
    x = x0 - add.float()
    ov = ln_regimes(1, d, g)[[1, 5, 6]]
    row0, n, L = SPLICE
    v = (x + add.float()).view(ROWS // L, L, d).clone()  # one fp32 add, as the kernel's
    v[:, row0:row0 + n] = ov
    v = v.view(ROWS, d)
    ref = ln64(v, gamma, beta)
    pads, groups, tag = pads_of(strided), ln_groups(), f"fused {add_kind} {dtype} d={d}{' strided' if strided else ''}"
    kw = dict(add=add if add_kind == "f32" else None, add_lp=add if add_kind == "lp" else None, ov=ov, xout=True, out_f32=add_kind == "lp")
    r = run_fwd(lib, "mudpt_layernorm_fwd_fused", dtype, d, pads, x, gamma, beta, **kw)
    assert same_bits(r["xout"], v), "xout is not x + add with the splice applied"
    check_stats(tag, r, ref, gamma, groups)
    check_y(tag, dtype, r, ref, gamma, groups, out_f32=kw["out_f32"])
    assert_same_results(r, run_fwd(lib, "mudpt_layernorm_fwd_ex", dtype, d, pads, x, gamma, beta, **kw))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("d,strided", LAYOUTS, ids=LAYOUT_IDS)
def test_forward_gather(lib, dtype, d, strided):
    """row_index out of order and with one row named twice: result and statistics row r come from x[row_index[r]]."""
    x, gamma, beta, _, _, ref = case(d)
    idx = torch.randperm(ROWS, generator=torch.Generator().manual_seed(d))
    idx[7] = idx[20]
    pads, tag = pads_of(strided), f"gather {dtype} d={d}{' strided' if strided else ''}"
    ref, groups = rows_of(ref, idx), ln_groups()[idx]
    r = run_fwd(lib, "mudpt_layernorm_fwd", dtype, d, pads, x, gamma, beta, rows=ROWS, row_index=idx)
    check_stats(tag, r, ref, gamma, groups)
    check_y(tag, dtype, r, ref, gamma, groups)
    assert same_bits(r["out"][7], r["out"][20])
    assert_same_results(r, run_fwd(lib, "mudpt_layernorm_fwd_ex", dtype, d, pads, x, gamma, beta, rows=ROWS, row_index=idx))
    f = run_fwd(lib, "mudpt_layernorm_fwd_ex", dtype, d, pads, x, gamma, beta, rows=ROWS, row_index=idx, out_f32=True)
    check_y(tag + " f32", dtype, f, ref, gamma, groups, out_f32=True)


# ---- backward ----
def run_bwd(lib, dtype, d, pads, x, gamma, dy, mean, rstd, dres=None, want=("dx", "dx_lp"), row_index=None, index_mode=0, side=False, export="mudpt_layernorm_bwd_ex"):
    """One launch of ln_bwd_kernel between guards.  x / dres / dx / dx_lp have x.shape[0] rows; dy, mean and rstd whatever the index mode
    says.  dy and dres pick the kernel form by their dtype (fp32 or T)."""
    dt, tt = DT[dtype]
    total = x.shape[0]
    rows = total if row_index is None else len(row_index)
    xc, gc, dyc, mc, rc = dev_in(x, pads["x"]), vec_in(gamma), dev_in(dy, pads["dy"]), vec_in(mean), vec_in(rstd)
    drc = None if dres is None else dev_in(dres, pads["dres"])
    lp = dres is not None and dres.dtype != torch.float32
    dx = dev_out(total, d, pads["dx"]) if "dx" in want else None
    dx_lp = dev_out(total, d, pads["dx_lp"], tt) if "dx_lp" in want else None
    ic = None if row_index is None else row_index.to(torch.int32).cuda()
    row0, n, L = SPLICE
    side_ldb = n * d + 36
    sd = torch.full((total // L + 1, side_ldb), SENT, device="cuda") if side else None
    kw = dict(dtype=dt, dy=dyc, lddy=d + pads["dy"], dy_f32=int(dy.dtype == torch.float32), x=xc, ldx=d + pads["x"], row_index=ic, mean=mc, rstd=rc, gamma=gc,
              dres=None if lp else drc, lddres=d + pads["dres"], dx=dx, lddx=d + pads["dx"], dx_lp=dx_lp, lddx_lp=d + pads["dx_lp"], rows=rows, d=d)
    if export == "mudpt_layernorm_bwd_ex":
        kw.update(dres_lp=drc if lp else None, side=sd, side_row0=row0, side_n=n, side_L=L, side_ldb=side_ldb, index_mode=index_mode)
    ok(lib, capi.call(export, **kw))
    res = {}
    if dx is not None:
        res["dx"] = take(dx, total, d, row_index)
    if dx_lp is not None:
        res["dx_lp"] = take(dx_lp, total, d, row_index)
    if side:
        c = sd.cpu()
        assert (c[:, n * d:] == SENT).all() and (c[total // L:] == SENT).all(), "a write outside the side rows"
        res["side"] = c[:total // L, :n * d].reshape(total // L, n, d)
    return res


def check_dx(tag, dtype, res, ref, bref, dy, groups, rows=None):
    rows = slice(None) if rows is None else rows
    if "dx" in res:
        ln_check(tag, "dx", res["dx"][rows], bref.dx, ln_bwd_bounds(ref, bref, dy)["dx"], groups, record=WORST)
    if "dx_lp" in res:
        ln_check(tag, "dx_" + dtype, res["dx_lp"][rows], bref.dx, ln_bwd_bounds(ref, bref, dy, dtype)["dx"], groups, record=WORST)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("dy_kind", ["T", "f32"])
@pytest.mark.parametrize("d,strided", LAYOUTS, ids=LAYOUT_IDS)
def test_backward_forms(lib, dtype, dy_kind, d, strided):
    """dy in T or fp32 x the residual gradient in fp32, in T or absent x dx, dx_lp or both; mean / rstd are float64's rounded to fp32."""
    tt = DT[dtype][1]
    x, gamma, _, dy, dres, ref = case(d)
    dy = dy if dy_kind == "f32" else dy.to(tt)
    mean, rstd = ln_stats32(ref)
    pads, groups = pads_of(strided), ln_groups()
    for res_kind, dr in (("dres", dres), ("dres_lp", dres.to(tt)), ("none", None)):
        bref = ln_bwd64(ref, gamma, dy, dr)
        for want in (("dx",), ("dx_lp",), ("dx", "dx_lp")):
            tag = f"bwd {dtype} dy {dy_kind} {res_kind} -> {'+'.join(want)} d={d}{' strided' if strided else ''}"
            r = run_bwd(lib, dtype, d, pads, x, gamma, dy, mean, rstd, dr, want)
            check_dx(tag, dtype, r, ref, bref, dy, groups)
            if res_kind == "dres_lp":
                again = run_bwd(lib, dtype, d, pads, x, gamma, dy, mean, rstd, dr, want)
            else:  # the narrower export of the same launcher
                again = run_bwd(lib, dtype, d, pads, x, gamma, dy, mean, rstd, dr, want, export="mudpt_layernorm_bwd")
            assert_same_results(r, again)
            if len(want) == 2:
                assert same_bits(r["dx_lp"], r["dx"].to(tt)), "dx_lp is not dx rounded to T"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("d,strided", LAYOUTS, ids=LAYOUT_IDS)
def test_backward_side_splice(lib, dtype, d, strided):
    """Rows 2..4 of every 7-row sequence go to side[sequence] in fp32 and leave exact zeros in dx / dx_lp."""
    tt = DT[dtype][1]
    x, gamma, _, dy, dres, ref = case(d)
    dy = dy.to(tt)
    mean, rstd = ln_stats32(ref)
    bref = ln_bwd64(ref, gamma, dy, dres)
    row0, n, L = SPLICE
    spliced = (torch.arange(ROWS) % L >= row0) & (torch.arange(ROWS) % L < row0 + n)
    tag = f"bwd side {dtype} d={d}{' strided' if strided else ''}"
    r = run_bwd(lib, dtype, d, pads_of(strided), x, gamma, dy, mean, rstd, dres, side=True)
    assert (r["dx"][spliced] == 0).all() and (r["dx_lp"][spliced] == 0).all()
    merged = {"dx": r["dx"].clone(), "dx_lp": r["dx_lp"].clone()}
    merged["dx"][spliced] = r["side"].reshape(-1, d)
    merged["dx_lp"][spliced] = r["side"].reshape(-1, d).to(tt)
    check_dx(tag, dtype, merged, ref, bref, dy, ln_groups())
    assert_same_results(r, run_bwd(lib, dtype, d, pads_of(strided), x, gamma, dy, mean, rstd, dres, side=True))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("d,strided", LAYOUTS, ids=LAYOUT_IDS)
def test_backward_index_modes(lib, dtype, mode, d, strided):
    """23 of the 35 rows in a shuffled order: x, dres and the result at row_index[r]; dy and the statistics compact (mode 0), both by token
    row (1), the statistics by token row (2).  bf16 runs the T stream forms, fp16 the fp32 ones; rows not named keep the sentinel."""
    tt = DT[dtype][1]
    lp = dtype == "bf16"
    x, gamma, _, dy, dres, ref = case(d)
    dy, dres = (dy.to(tt), dres.to(tt)) if lp else (dy, dres)
    idx = torch.randperm(ROWS, generator=torch.Generator().manual_seed(100 + d))[:23]
    mean, rstd = ln_stats32(ref)
    sub = rows_of(ref, idx)
    bref = ln_bwd64(sub, gamma, dy[idx], dres[idx])
    dy_arg = dy if mode == 1 else dy[idx].contiguous()
    mean_arg, rstd_arg = (mean[idx].contiguous(), rstd[idx].contiguous()) if mode == 0 else (mean, rstd)
    tag = f"bwd index mode {mode} {dtype} d={d}{' strided' if strided else ''}"
    r = run_bwd(lib, dtype, d, pads_of(strided), x, gamma, dy_arg, mean_arg, rstd_arg, dres, row_index=idx, index_mode=mode)
    check_dx(tag, dtype, r, sub, bref, dy[idx], ln_groups()[idx], rows=idx)
    assert_same_results(r, run_bwd(lib, dtype, d, pads_of(strided), x, gamma, dy_arg, mean_arg, rstd_arg, dres, row_index=idx, index_mode=mode))


def run_affine(lib, d, pads, x, gamma, dy, mean, rstd, dres, accumulate, dgamma, dbeta):
    rows = x.shape[0]
    xc, gc, dyc, mc, rc = dev_in(x, pads["x"]), vec_in(gamma), dev_in(dy, pads["dy"]), vec_in(mean), vec_in(rstd)
    drc = None if dres is None else dev_in(dres, pads["dres"])
    dx = dev_out(rows, d, pads["dx"])
    ok(lib, capi.call("mudpt_layernorm_bwd_affine", x=xc, ldx=d + pads["x"], mean=mc, rstd=rc, gamma=gc, dy=dyc, lddy=d + pads["dy"], dres=drc, lddres=d + pads["dres"],
                      dx=dx, lddx=d + pads["dx"], dgamma=dgamma, dbeta=dbeta, accumulate=accumulate, rows=rows, d=d))
    return take(dx, rows, d)


@pytest.mark.parametrize("d,strided", LAYOUTS, ids=LAYOUT_IDS)
def test_backward_affine(lib, d, strided):
    """The fp32 backward with dgamma / dbeta, with and without the residual gradient; accumulate is one fp32 add onto the old contents."""
    x, gamma, _, dy, dres, ref = case(d)
    mean, rstd = ln_stats32(ref)
    pads, groups = pads_of(strided), ln_groups()
    first = None
    for dr in (dres, None):
        tag = f"affine {'dres' if dr is not None else 'no dres'} d={d}{' strided' if strided else ''}"
        bref = ln_bwd64(ref, gamma, dy, dr)
        b = ln_bwd_bounds(ref, bref, dy)
        dga, dbe = vec_out(d), vec_out(d)
        dx = run_affine(lib, d, pads, x, gamma, dy, mean, rstd, dr, 0, dga, dbe)
        dga, dbe = take_vec(dga, d), take_vec(dbe, d)
        ln_check(tag, "affine_dx", dx, bref.dx, b["dx"], groups, record=WORST)
        ln_check(tag, "dgamma", dga, bref.dgamma, b["dgamma"], record=WORST)
        ln_check(tag, "dbeta", dbe, bref.dbeta, b["dbeta"], record=WORST)
        if first is not None:
            assert same_bits(dga, first[0]) and same_bits(dbe, first[1])
        first = first or (dga, dbe)
        g = torch.Generator().manual_seed(d)
        prev_g, prev_b = torch.randn(d, generator=g), torch.randn(d, generator=g)
        acc_g, acc_b = torch.cat([prev_g, torch.full((3,), SENT)]).cuda(), torch.cat([prev_b, torch.full((3,), SENT)]).cuda()
        dx2 = run_affine(lib, d, pads, x, gamma, dy, mean, rstd, dr, 1, acc_g, acc_b)
        assert same_bits(dx2, dx), "two launches differ"
        assert same_bits(take_vec(acc_g, d), prev_g + dga) and same_bits(take_vec(acc_b, d), prev_b + dbe)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("d,strided", [(260, True), (1024, False)], ids=["d260-strided", "d1024"])
@pytest.mark.parametrize("regime", ["offset", "outliers"])
def test_one_row(lib, dtype, d, strided, regime):
    """rows = 1: three of the block's four waves leave at once."""
    tt = DT[dtype][1]
    x, gamma, beta, dy, dres, _ = case(d)
    i = LN_REGIMES.index(regime) * LN_ROWS_PER_REGIME
    x, dy, dres = x[i:i + 1], dy[i:i + 1].to(tt), dres[i:i + 1]
    ref = ln64(x, gamma, beta)
    pads, tag = pads_of(strided), f"one row ({regime}) {dtype} d={d}"
    r = run_fwd(lib, "mudpt_layernorm_fwd", dtype, d, pads, x, gamma, beta)
    check_stats(tag, r, ref, gamma, None)
    check_y(tag, dtype, r, ref, gamma, None)
    mean, rstd = ln_stats32(ref)
    bref = ln_bwd64(ref, gamma, dy, dres)
    check_dx(tag, dtype, run_bwd(lib, dtype, d, pads, x, gamma, dy, mean, rstd, dres), ref, bref, dy, None)
    dga, dbe = vec_out(d), vec_out(d)
    bref32 = ln_bwd64(ref, gamma, dy.float(), dres)
    dx = run_affine(lib, d, pads, x, gamma, dy.float(), mean, rstd, dres, 0, dga, dbe)
    b = ln_bwd_bounds(ref, bref32, dy.float())
    ln_check(tag, "affine_dx", dx, bref32.dx, b["dx"], record=WORST)
    ln_check(tag, "dgamma", take_vec(dga, d), bref32.dgamma, b["dgamma"], record=WORST)
    ln_check(tag, "dbeta", take_vec(dbe, d), bref32.dbeta, b["dbeta"], record=WORST)

