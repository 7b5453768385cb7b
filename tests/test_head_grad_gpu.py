"""The head's backward from a given logit gradient (launch_head_grad through mudpt_head_grad) against a float64 evaluation of its formula

    dimg = gmul * (l2norm_bwd(scale * G   . txt_n, img_n, img_inv) + Eimg)      l2norm_bwd(d, n, inv) = inv * (d - n <d, n>) per row
    dtxt = gmul * (l2norm_bwd(scale * G^T . img_n, txt_n, txt_inv) + Etxt)

on states made by a float64 normalisation rounded to fp32.  Every operand sits between NaN guard rows, every output between sentinel guard
rows, and all of them must come back as they were.  Bounds: the fused kernels hold FUSED_BOUND's gradient figure of tests/test_kernels_gpu.py
(the same exact-fp32 contraction: largest error <= 2e-5 x the reference tensor's rms); the unfused launchers 4 x the error of a plain fp32 CPU
evaluation against the float64 one on the same inputs, computed here (the measured_bound recipe of that file).  Every shape runs on what
the dispatch takes (path 0: the fused kernels only where they fit AND are the faster form, B <= 16 and C <= 16), on the unfused launchers
(path 1) and, where they fit, on the fused kernels (path 2); the path taken is held to that rule."""
import ctypes as C
import functools

import pytest
import torch

from mudpt_amd import capi
from tests.helpers import SENT

pytestmark = pytest.mark.gpu

SCALE, GMUL = 14.2857, 384.0
FUSED = 2e-5  # tests/test_kernels_gpu.py FUSED_BOUND["dimg"] / ["dtxt"]
GUARD = 8     # guard rows around every tensor
# (B, C, e): the tiny fixtures' shape; exact tiles; ragged rows and classes with five e-tiles (a wave's group of four has a tail); the LDS
# limit; the real class count; e % 16 != 0 and e > 1024 (both unfused)
SHAPES = [(3, 11, 128), (16, 16, 64), (17, 33, 80), (33, 5, 1024), (37, 1000, 512), (5, 7, 72), (4, 9, 1040)]
FORM_SHAPES = [(17, 33, 80), (5, 7, 72)]
KINDS = ("ce", "dense")
_CASES, _UNFUSED = {}, {}


FUSED_MAX_ROWS = 16  # include/mudpt.h mudpt_head_grad: with more images or classes the dispatch takes the unfused form, the faster one there


def fused_fits(e):
    """The [16][e] fp32 tile in 64 KB of LDS."""
    return e % 16 == 0 and e <= 1024


def path_rule(path, B, Cn, e):
    """The documented form of a call: 0 fused, 1 unfused (path 0: the dispatch; 1: unfused; 2: fused, only where it fits)."""
    return 0 if path == 2 or (path == 0 and fused_fits(e) and B <= FUSED_MAX_ROWS and Cn <= FUSED_MAX_ROWS) else 1


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return capi.load()


def make_case(B, Cn, e, kind):
    """State and gradient inputs on the CPU in fp32 (what the kernels read), computed once per (shape, kind) and left unchanged."""
    key = (B, Cn, e, kind)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * B + 10 * Cn + e + (7 if kind == "ce" else 0))
        img, txt = torch.randn(B, e, generator=g, dtype=torch.float64), torch.randn(Cn, e, generator=g, dtype=torch.float64)
        inv_i, inv_t = 1.0 / img.norm(dim=1), 1.0 / txt.norm(dim=1)
        if kind == "ce":
            z = 3.0 * torch.randn(B, Cn, generator=g, dtype=torch.float64)
            y = torch.randint(0, Cn, (B,), generator=g)
            G = (torch.softmax(z, dim=1) - torch.nn.functional.one_hot(y, Cn)) / B
        else:
            G = 1e-2 * torch.randn(B, Cn, generator=g, dtype=torch.float64)
        Eimg, Etxt = 1e-3 * torch.randn(B, e, generator=g, dtype=torch.float64), 1e-3 * torch.randn(Cn, e, generator=g, dtype=torch.float64)
        _CASES[key] = {"img_n": (img * inv_i[:, None]).float(), "img_inv": inv_i.float(), "txt_n": (txt * inv_t[:, None]).float(), "txt_inv": inv_t.float(),
                       "G": G.float(), "Eimg": Eimg.float(), "Etxt": Etxt.float()}
    return _CASES[key]


def evaluate(c, dtype, G=True, Eimg=True, Etxt=True, gmul=GMUL, scale=SCALE):
    """The formula in `dtype` on the fp32 inputs: (dimg, dtxt)."""
    t = {k: v.to(dtype) for k, v in c.items()}

    def half(Gm, other_n, n, inv, E):
        out = torch.zeros_like(n)
        if G:
            d = scale * (Gm @ other_n)
            out = inv[:, None] * (d - n * (d * n).sum(dim=1, keepdim=True))
        return gmul * (out + E) if E is not None else gmul * out

    return (half(t["G"], t["txt_n"], t["img_n"], t["img_inv"], t["Eimg"] if Eimg else None),
            half(t["G"].t(), t["img_n"], t["txt_n"], t["txt_inv"], t["Etxt"] if Etxt else None))


def guarded(t, fill, pad_cols=0):
    """t between GUARD rows of `fill` on the device (pad_cols more columns of `fill` in every row): (whole buffer, the view the kernel gets)."""
    rows = t.shape[0]
    shape = (rows + 2 * GUARD,) + ((t.shape[1] + pad_cols,) if t.dim() == 2 else ())
    buf = torch.full(shape, fill, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + rows]
    if t.dim() == 2:
        view[:, :t.shape[1]] = t.cuda()
    else:
        view[:] = t.cuda()
    return buf, view


def untouched(buf, rows, cols, fill):
    """The guard rows (and padding columns) of a guarded buffer still hold `fill`."""
    same = (lambda x: torch.isnan(x).all()) if fill != fill else (lambda x: (x == fill).all())
    okay = same(buf[:GUARD]) and same(buf[GUARD + rows:])
    if buf.dim() == 2 and buf.shape[1] > cols:
        okay = okay and same(buf[GUARD:GUARD + rows, cols:])
    return bool(okay)


def _run(lib, c, path=0, G=True, Eimg=True, Etxt=True, dimg=True, dtxt=True, pad=0, gmul=GMUL, rows=None):
    """mudpt_head_grad on guarded device copies; returns (dimg | None, dtxt | None on the CPU, path taken).  pad: ldg = C + pad with NaN in
    the padding columns.  rows: image rows to keep (a call on a subset of the batch).  A NULL output's buffer is passed nowhere and must
    keep its sentinels."""
    nan = float("nan")
    sub = {k: (v[rows] if rows is not None and k in ("img_n", "img_inv", "G", "Eimg") else v) for k, v in c.items()}
    B, e = sub["img_n"].shape
    Cn = sub["txt_n"].shape[0]
    ops = {k: guarded(v, nan, pad if k == "G" else 0) for k, v in sub.items()}
    o_img, v_img = guarded(torch.full((B, e), SENT), SENT)
    o_txt, v_txt = guarded(torch.full((Cn, e), SENT), SENT)
    taken = C.c_int32(-1)
    use = {"G": G, "Eimg": Eimg, "Etxt": Etxt}
    rc = capi.call("mudpt_head_grad", **{k: (ops[k][1] if use.get(k, True) else None) for k in ops}, ldg=Cn + pad, scale=SCALE, gmul=gmul, B=B, C=Cn, e=e,
                   dimg=v_img if dimg else None, dtxt=v_txt if dtxt else None, path=path, path_taken=C.byref(taken))
    assert rc == 0, lib.mudpt_last_error().decode()
    torch.cuda.synchronize()
    for k, (buf, view) in ops.items():
        assert untouched(buf, view.shape[0], sub[k].shape[1] if sub[k].dim() == 2 else 0, nan), f"guards of {k}"
        assert torch.equal(view[:, :sub[k].shape[1]].cpu() if view.dim() == 2 else view.cpu(), sub[k]), f"{k} was written"
    assert untouched(o_img, B, e, SENT) and untouched(o_txt, Cn, e, SENT), "an output's guard rows were written"
    if not dimg:
        assert (v_img == SENT).all(), "dimg was NULL and its buffer was written"
    if not dtxt:
        assert (v_txt == SENT).all(), "dtxt was NULL and its buffer was written"
    return (v_img.cpu() if dimg else None), (v_txt.cpu() if dtxt else None), taken.value


def rel_err(got, ref):
    return (got.double() - ref).abs().max().item() / (ref.pow(2).mean().sqrt().item() + 1e-300)


def unfused_bound():
    """4 x the worst error of the fp32 CPU evaluation against the float64 one over every shape and both forms of G, per output."""
    if not _UNFUSED:
        worst = {"dimg": 0.0, "dtxt": 0.0}
        for B, Cn, e in SHAPES:
            for kind in KINDS:
                c = make_case(B, Cn, e, kind)
                for extras in (True, False):  # the inputs test_against_float64 runs: with and without the addends
                    for k, a, r in zip(worst, evaluate(c, torch.float32, Eimg=extras, Etxt=extras), evaluate(c, torch.float64, Eimg=extras, Etxt=extras)):
                        worst[k] = max(worst[k], rel_err(a, r))
        _UNFUSED.update({k: 4 * v for k, v in worst.items()})
        print("unfused bound (4 x the fp32 CPU evaluation's error / rms):", {k: f"{v:.3e}" for k, v in _UNFUSED.items()})
    return _UNFUSED


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64(lib, shape, kind):
    """Both outputs on the dispatched path and on each forced form (the fused one where it fits), with and without the feature-gradient addends."""
    c = make_case(*shape, kind)
    for extras in (True, False):
        ref = evaluate(c, torch.float64, Eimg=extras, Etxt=extras)
        for path in (0, 1, 2) if fused_fits(shape[2]) else (0, 1):
            dimg, dtxt, taken = _run(lib, c, path=path, Eimg=extras, Etxt=extras)
            assert taken == path_rule(path, *shape), (shape, path, taken)
            for k, got, r in (("dimg", dimg, ref[0]), ("dtxt", dtxt, ref[1])):
                err = rel_err(got, r)
                bound = FUSED if taken == 0 else unfused_bound()[k]
                print(f"{shape} {kind} extras={extras} path {path} (took {taken}) {k}: max err / rms {err:.3e} (bound {bound:.3e}, ratio {err / bound:.3f})")
                assert err <= bound, (shape, kind, path, k, err, bound)


@pytest.mark.parametrize("shape,form", [(FORM_SHAPES[0], 2), (FORM_SHAPES[0], 0), (FORM_SHAPES[1], 0)], ids=["17x33x80-fused", "17x33x80-dispatch", "5x7x72-dispatch"])
def test_forms(lib, shape, form):
    """Every nullable operand and output, a row stride beyond C and a row alone in its call: on the fused kernels, and on what the dispatch takes."""
    c = make_case(*shape, "dense")
    B, Cn, e = shape
    full = _run(lib, c, path=form)
    assert full[2] == path_rule(form, *shape)
    run = functools.partial(_run, path=form)  # the forms below run on the same path
    # a NULL output is not computed and changes no bit of the other
    only_txt, only_img = run(lib, c, dimg=False), run(lib, c, dtxt=False)
    assert only_txt[0] is None and torch.equal(only_txt[1], full[1])
    assert only_img[1] is None and torch.equal(only_img[0], full[0])
    # the addends: NULL against given differ by gmul * E (to the rounding of one fp32 addition), and a NULL one leaves the other output alone
    no_e = run(lib, c, Eimg=False, Etxt=False)
    for got, base, E in ((full[0], no_e[0], c["Eimg"]), (full[1], no_e[1], c["Etxt"])):
        want = base.double() + GMUL * E.double()
        assert (got.double() - want).abs().max().item() <= 2.0 ** -23 * want.abs().max().item()
        assert not torch.equal(got, base)
    half_e = run(lib, c, Etxt=False)
    assert torch.equal(half_e[0], full[0]) and torch.equal(half_e[1], no_e[1])
    # G NULL: a feature-only loss, no contraction; gmul * E to the last bit, zeros where that E is NULL too
    for gmul in (GMUL, 3.0):
        fo = run(lib, c, G=False, gmul=gmul)
        assert torch.equal(fo[0], gmul * c["Eimg"]) and torch.equal(fo[1], gmul * c["Etxt"])
    fo = run(lib, c, G=False, Etxt=False)
    assert torch.equal(fo[0], GMUL * c["Eimg"]) and torch.count_nonzero(fo[1]) == 0
    # a row stride beyond C, NaN in the padding columns: the same bits
    padded = run(lib, c, pad=5)
    assert torch.equal(padded[0], full[0]) and torch.equal(padded[1], full[1])
    # an image row's gradient does not depend on the rows beside it: alone in its call, the same bits
    for b in (0, B - 1):
        alone = run(lib, c, rows=[b], dtxt=False)
        assert torch.equal(alone[0][0], full[0][b]), b
    # forced unfused: every form above again agrees with float64 (bounds: test_against_float64); here the NULL handling
    u = _run(lib, c, path=1)
    u_txt, u_pad = _run(lib, c, path=1, dimg=False), _run(lib, c, path=1, pad=5)
    assert u[2] == 1 and torch.equal(u_txt[1], u[1]) and torch.equal(u_pad[0], u[0]) and torch.equal(u_pad[1], u[1])
    fo = _run(lib, c, path=1, G=False)
    assert torch.equal(fo[0], GMUL * c["Eimg"]) and torch.equal(fo[1], GMUL * c["Etxt"])


def test_refusals_write_nothing(lib):
    """The refusals of tests/test_custom_loss_cpu.py on real buffers: the sentinel-filled outputs stay as they were."""
    c = make_case(3, 11, 128, "dense")
    d = {k: v.cuda() for k, v in c.items()}
    dimg, dtxt = torch.full((3, 128), SENT, device="cuda"), torch.full((11, 128), SENT, device="cuda")
    base = dict(d, ldg=11, scale=SCALE, gmul=GMUL, B=3, C=11, e=128, dimg=dimg, dtxt=dtxt, path=0)
    for change, word in ((dict(txt_inv=None), "txt_inv"), (dict(B=0), "B=0"), (dict(ldg=10), "ldg=10"), (dict(dimg=None, dtxt=None), "dimg and dtxt"),
                         (dict(G=None, Eimg=None, Etxt=None), "G, Eimg and Etxt")):
        rc = capi.call("mudpt_head_grad", **dict(base, **change))
        torch.cuda.synchronize()
        assert rc == 1 and word in lib.mudpt_last_error().decode(), (change, lib.mudpt_last_error().decode())
        assert (dimg == SENT).all() and (dtxt == SENT).all()
