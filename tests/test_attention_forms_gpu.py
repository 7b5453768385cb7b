"""Every attention kernel INSTANTIATION -- (form, NC = padded length / 32, mask) for L <= 224, the persistent loops over pairs, the single-query
and the long forms -- against float64, between guards, through the C ABI.

Guards: every operand (qkv, dout, the forward output the backward reads) lies inside a larger flat allocation with ATTN_GUARD_ROWS rows of NaN
before and after it -- a value consumed from outside the tensor poisons the result, even where P = 0 multiplies it; every output (out, lse,
dqkv, delta) lies between rows of a sentinel that must survive bit for bit, and is itself pre-filled with NaN, so an element the launch did not
write shows.  lse[.., L:Lp] is zero after every forward form.

Parity: forward output, lse and dqkv of every form and kernel-choice flag against helpers.attn64 / attn64_fwd_bwd on the T-rounded inputs, with
the tolerances of test_attention_fwd_bwd; two forms agree to 2 EPS x scale; every form is bit for bit the same run to run; every launch takes the
form its table entry names (mudpt_attention_form; tests/test_capi_cpu.py holds the same tables to it without a GPU).

Isolation (kernels.h, AttnArgs: "rows of another sequence must be finite"): the middle sequence alone, between zero neighbours and between
neighbours of 64 x the magnitude gives EQUAL out, lse, dqkv and delta, for every form.

Peaked rows in the backward (test_attention_backward_peaked_rows): q and k scaled by 3 (scores of +-70 and more, rows dominated by one key), where
dS = p (dP - delta) cancels.  The bound comes from a second float64 reference, attn64_fwd_bwd(round_to=T), which rounds to T exactly where the
kernels do and nowhere else:
  forward   exp(s - rowmax) -> T before P.V (Attn::pack2 in fwd_pv_store; the row sum l is taken from the unrounded values);
            O = (P.V) / l -> T at the store (store_t_out);
  backward  delta = rowsum(dO * O) from that T-rounded O, in fp32 (never rounded);
            P = exp(s - lse) -> T before P^T.dO (dV; pack2 in the dK / dV blocks);
            dS = P (dP - delta) -> T before dS.K (dQ) and dS^T.Q (dK) (pack2; the sweep form carries the same T value through LDS);
            dQ, dK (x 1/8) and dV -> T at the store (store_t).
A kernel's largest deviation from the plain float64 gradient may be 4 x that emulation's (fp32 summation order and the fast exp2 are not
emulated), and never has to be below the unit-gain tolerance.  Measured on an MI355X, largest |error| over the backward flags of a case, as a
multiple of EPS x max|dref| (emulation | kernel):
    NC  mask     bf16 emulation | kernel    fp16 emulation | kernel
    1   none      1.13 |  1.13              1.50 |  1.50
    1   causal    1.04 |  1.04              0.88 |  0.88
    2   none      1.55 |  1.55              1.40 |  1.40
    2   causal    1.05 |  1.05              1.21 |  1.21
    3   none      1.46 |  1.46              1.50 |  1.50
    3   causal    1.32 |  1.32              1.11 |  1.11
    4   none      1.26 |  1.26              1.36 |  1.36
    4   causal    1.15 |  1.15              2.10 |  1.69
    5   none      1.34 |  1.34              1.10 |  1.10
    5   causal    1.60 |  1.60              1.46 |  1.46
    6   none      1.48 |  1.48              1.28 |  1.28
    6   causal    1.10 |  1.10              0.85 |  0.86
    7   none      1.14 |  1.14              1.29 |  1.29
    7   causal    1.33 |  1.33              1.11 |  1.11
The forms of a case agree to the digits shown.  The emulation reproduces the kernels' error (its roundings are the ones that matter), and 4 x
its error (3.4 .. 8.4 EPS x max|dref|) stays below the unit-gain tolerance of 12 EPS x max|dref|, which therefore is the bound in force here.
"""
import functools

import pytest
import torch

from mudpt_amd import capi
from tests.helpers import (ATTN_GUARD_ROWS, ATTN_INSTANCE_CASES, ATTN_LONG_CASES, ATTN_MULTI_PAIR_CASES, ATTN_PEAKED_CASES, ATTN_PEAKED_GAIN,
                           ATTN_SINGLE_EDGE_CASES, SENT, P, attn64, attn64_fwd_bwd, attn_instance_launches, attn_long_launches, ok)

pytestmark = pytest.mark.gpu

DT = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16)}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # half ulp relative
G = ATTN_GUARD_ROWS
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return capi.load()


@functools.lru_cache(maxsize=None)
def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def guarded(shape, dtype, guard, values=None, fill=NAN):
    """A flat device buffer of G rows of `guard`, the tensor, G rows of `guard` (a row = the tensor's last dimension), and the tensor's view in
    it, holding `values` (a CPU tensor) or `fill`.  G rows of any tensor here are a multiple of 16 bytes: the view keeps the allocation's alignment."""
    width, n = shape[-1], 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * G * width,), guard, dtype=dtype, device="cuda")
    win = buf[G * width:G * width + n].view(shape)
    assert win.data_ptr() % 16 == 0
    if values is not None:
        win.copy_(values.to(dtype))
    else:
        win.fill_(fill)
    return buf, win


def assert_guards(buf, win, guard, what):
    width, n = win.shape[-1], win.numel()
    bad = (torch.cat([buf[:G * width], buf[G * width + n:]]) != guard).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} guard elements written, first at flat guard index {bad[0].item()} (the tensor starts at {G * width})"


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32), b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def same_values(a, b):
    """Equal element for element (a zero may differ in sign); NaN -- an element no kernel of this form writes -- only where the other has it."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def inputs(B, L, H, tt, seed, gain=1.0):
    """qkv [B, L, 3 H 64] and dout [B, L, H 64] in T on the CPU; gain scales q and k only (values and dout stay O(1))."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g)
    qkv[..., :2 * H * 64] *= gain
    return qkv.to(tt), torch.randn(B, L, H * 64, generator=g).to(tt)


class Launches:
    """mudpt_attention_fwd / _bwd on one problem: guarded operands, fresh guarded outputs per launch, the form and the guards checked every time."""

    def __init__(self, lib, dtype, qkv, dout, H):
        self.lib, (self.dt, self.tt), self.H = lib, DT[dtype], H
        self.B, self.L = qkv.shape[:2]
        self.Lp = lib.mudpt_attention_padded_len(self.L)
        assert self.Lp % 32 == 0 and 0 <= self.Lp - self.L < 32
        _, self.qkv = guarded(qkv.shape, self.tt, NAN, qkv)
        _, self.dout = guarded(dout.shape, self.tt, NAN, dout)

    def takes(self, bwd, flags, form):
        got = self.lib.mudpt_attention_form(bwd, self.L, flags, 0)
        assert got == capi.ATTN_FORMS.index(form), f"L={self.L} flags={flags}: form {capi.ATTN_FORMS[got] if got >= 0 else got}, the case is there for {form}"

    def fwd(self, flags, form):
        self.takes(0, flags, form)
        B, L, H, Lp = self.B, self.L, self.H, self.Lp
        obuf, out = guarded((B, L, H * 64), self.tt, SENT)
        lbuf, lse = guarded((B, H, Lp), torch.float32, SENT)
        ok(self.lib, capi.call("mudpt_attention_fwd", dtype=self.dt, qkv=self.qkv, out=out, lse=lse, B=B, L=L, H=H, causal=flags))
        assert_guards(obuf, out, SENT, f"{form} out")
        assert_guards(lbuf, lse, SENT, f"{form} lse")
        assert not out.isnan().any(), f"{form}: out has unwritten or poisoned elements"
        assert lse[..., :L].isfinite().all(), f"{form}: lse has unwritten or poisoned elements"
        assert (lse[..., L:] == 0).all(), f"{form}: lse[.., L:Lp] must be zero (the backward reads it)"
        return out, lse

    def bwd(self, flags, form, out, lse):
        self.takes(1, flags, form)
        B, L, H, Lp = self.B, self.L, self.H, self.Lp
        _, o = guarded(out.shape, self.tt, NAN)
        o.copy_(out)
        dbuf, dqkv = guarded((B, L, 3 * H * 64), self.tt, SENT)
        ebuf, delta = guarded((B, H, Lp), torch.float32, SENT)
        ok(self.lib, capi.call("mudpt_attention_bwd", dtype=self.dt, qkv=self.qkv, out=o, dout=self.dout, lse=lse, delta=delta, dqkv=dqkv, B=B, L=L, H=H, causal=flags))
        assert_guards(dbuf, dqkv, SENT, f"{form} dqkv")
        assert_guards(ebuf, delta, SENT, f"{form} delta")
        assert not dqkv.isnan().any(), f"{form}: dqkv has unwritten or poisoned elements"
        # delta is scratch: the two-kernel, resident and staged forms pass it through memory (every real row), the others may keep it on chip
        if form in ("BWD_TWO", "BWD_RESIDENT", "BWD_STAGED"):
            assert delta[..., :L].isfinite().all(), f"{form}: delta has unwritten or poisoned elements"
        return dqkv, delta


def check_forward(dtype, out, lse, qkv, H, causal, ref_lse):
    L = qkv.shape[1]
    torch.testing.assert_close(out.cpu().double(), attn64(qkv, H, causal), atol=6 * EPS[dtype], rtol=6 * EPS[dtype])
    torch.testing.assert_close(lse[..., :L].cpu().double(), ref_lse, atol=1e-3, rtol=1e-4)


def check_delta(delta, out, dout, H):
    """delta = rowsum(dO * O) of the T values, 64 terms summed in fp32: within 2 x 64 x 2^-24 of the sum of the terms' magnitudes."""
    B, L, _ = out.shape
    t = (out.cpu().double() * dout.double()).view(B, L, H, 64)
    ref, mag = t.sum(-1).transpose(1, 2), t.abs().sum(-1).transpose(1, 2)
    bad = (delta[..., :L].cpu().double() - ref).abs() > 2.0 ** -17 * mag + 1e-30
    assert not bad.any(), f"delta differs from rowsum(dO * O) on {int(bad.sum())} rows"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal", ATTN_INSTANCE_CASES)
def test_attention_instance_parity_guarded(lib, dtype, B, L, H, causal):
    """Forward and every backward flag at one (NC, mask, L): parity, guards, the named form, bit-identical reruns, form-to-form agreement."""
    tt = DT[dtype][1]
    qkv, dout = inputs(B, L, H, tt, 1000 * L + causal)
    _, ref_lse, dref = attn64_fwd_bwd(qkv, dout, H, causal)
    run = Launches(lib, dtype, qkv, dout, H)
    (_, f0, form0), *backward = attn_instance_launches(L, causal)
    out, lse = run.fwd(f0, form0)
    check_forward(dtype, out, lse, qkv, H, causal, ref_lse)
    out2, lse2 = run.fwd(f0, form0)
    assert same_bits(out, out2) and same_bits(lse, lse2), f"{form0}: two runs differ"
    scale = dref.abs().max().item()
    first = None
    for _, flags, form in backward:
        dqkv, delta = run.bwd(flags, form, out, lse)
        torch.testing.assert_close(dqkv.cpu().double(), dref, atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype], msg=lambda m: f"{form} flags {flags}: {m}")
        if form == "BWD_TWO":
            check_delta(delta, out, dout, H)
        again, _ = run.bwd(flags, form, out, lse)
        assert same_bits(again, dqkv), f"{form} flags {flags}: two runs differ"
        if first is None:
            first = dqkv
        else:
            torch.testing.assert_close(dqkv.float(), first.float(), atol=2 * EPS[dtype] * scale, rtol=2 * EPS[dtype], msg=lambda m: f"{form} against the default form: {m}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal", ATTN_INSTANCE_CASES)
def test_attention_instance_isolation(lib, dtype, B, L, H, causal):
    """The padded keys and queries of sequence b are the first rows of sequence b + 1: the middle sequence's results must not move with its
    neighbours' (finite) values.  Alone, between zeros, between rows of 64 x the magnitude: equal out, lse, dqkv and delta, for every form."""
    tt = DT[dtype][1]
    assert B == 3
    qkv, dout = inputs(B, L, H, tt, 1000 * L + causal)
    launches = attn_instance_launches(L, causal)

    def neighbours(t, factor):
        r = (t.float() * factor).to(tt)
        r[1] = t[1]
        assert r.float().isfinite().all()
        return r

    def middle(q, d, i):
        run = Launches(lib, dtype, q, d, H)
        out, lse = run.fwd(launches[0][1], launches[0][2])
        res = {"out": out[i], "lse": lse[i]}
        for _, flags, form in launches[1:]:
            dqkv, delta = run.bwd(flags, form, out, lse)
            res[f"dqkv, {form} flags {flags}"], res[f"delta, {form} flags {flags}"] = dqkv[i], delta[i][:, :L]
        return res

    alone = middle(qkv[1:2], dout[1:2], 0)
    for name, factor in (("zero", 0.0), ("64 x", 64.0)):
        other = middle(neighbours(qkv, factor), neighbours(dout, factor), 1)
        for key, want in alone.items():
            assert same_values(other[key], want), f"{key}: the middle sequence between {name} neighbours differs from the sequence alone"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", ATTN_MULTI_PAIR_CASES, ids=lambda c: f"{c.kernel}-nc{c.NC}-{'causal' if c.causal else 'full'}")
def test_attention_persistent_kernels_walk_several_pairs(lib, dtype, case):
    """More (sequence, head) pairs than resident workgroups, the last round ragged: the persistent forward and the fused backward (one and two
    blocks per wave) stream the next pair in while they compute the current one, per NC with its own image size and wave count."""
    tt = DT[dtype][1]
    L, H, causal = case.L, case.H, case.causal
    B, cap = case.batch(device_cus()), case.cap(device_cus())
    assert B * H > cap and B * H % cap != 0
    qkv, dout = inputs(B, L, H, tt, 77 * case.NC + causal)
    _, ref_lse, dref = attn64_fwd_bwd(qkv, dout, H, causal)
    run = Launches(lib, dtype, qkv, dout, H)
    out, lse = run.fwd(int(causal), "FWD_PAIR" if causal else "FWD_PERSISTENT")
    check_forward(dtype, out, lse, qkv, H, causal, ref_lse)
    if case.kernel == "fwd":
        out2, lse2 = run.fwd(0, case.form)
        assert same_bits(out, out2) and same_bits(lse, lse2)
        return
    scale = dref.abs().max().item()
    dqkv, _ = run.bwd(case.flags, case.form, out, lse)
    torch.testing.assert_close(dqkv.cpu().double(), dref, atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype])
    again, _ = run.bwd(case.flags, case.form, out, lse)
    assert same_bits(again, dqkv)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal", ATTN_PEAKED_CASES)
def test_attention_backward_peaked_rows(lib, dtype, B, L, H, causal):
    """Every backward flag on rows dominated by one key: within 4 x the error of the float64 emulation that rounds to T where the kernels do
    (the module docstring lists the points and the measured figures), or within the unit-gain tolerance where that is larger."""
    tt = DT[dtype][1]
    qkv, dout = inputs(B, L, H, tt, 31 * L + causal, gain=ATTN_PEAKED_GAIN)
    _, ref_lse, dref = attn64_fwd_bwd(qkv, dout, H, causal)
    _, _, emu = attn64_fwd_bwd(qkv, dout, H, causal, round_to=tt)
    emu_err, scale = (emu - dref).abs().max().item(), dref.abs().max().item()
    allowed = torch.maximum(torch.full_like(dref, 4 * emu_err), 12 * EPS[dtype] * scale + 8 * EPS[dtype] * dref.abs())
    run = Launches(lib, dtype, qkv, dout, H)
    (_, f0, form0), *backward = attn_instance_launches(L, causal)
    out, lse = run.fwd(f0, form0)
    check_forward(dtype, out, lse, qkv, H, causal, ref_lse)
    worst = []
    for _, flags, form in backward:
        dqkv, _ = run.bwd(flags, form, out, lse)
        err = (dqkv.cpu().double() - dref).abs()
        unit = EPS[dtype] * scale
        print(f"PEAKED nc={run.Lp // 32} causal={int(causal)} {dtype} flags={flags} {form}: emulation {emu_err / unit:.2f} kernel {err.max().item() / unit:.2f} (x EPS x max|dref| = {unit:.3e})")
        if (err > allowed).any():
            worst.append(f"{form} flags {flags}: {int((err > allowed).sum())} elements beyond the bound, largest error {err.max().item():.3e} against 4 x {emu_err:.3e}")
    assert not worst, "; ".join(worst)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal", ATTN_LONG_CASES)
def test_attention_long_forms_guarded(lib, dtype, B, L, H, causal):
    """L > 224: the staged form at 4096 rows and at 1025 under the mask, the resident forms at their edges; default and staged-by-switch,
    forward and backward, between guards and at the parity bounds of the short forms."""
    tt = DT[dtype][1]
    qkv, dout = inputs(B, L, H, tt, 13 * L + causal)
    ref_out, ref_lse, dref = attn64_fwd_bwd(qkv, dout, H, causal)
    scale = dref.abs().max().item()
    run = Launches(lib, dtype, qkv, dout, H)
    fwd = None
    for bwd, flags, form in attn_long_launches(L, causal):
        if not bwd:
            out, lse = run.fwd(flags, form)
            torch.testing.assert_close(out.cpu().double(), ref_out, atol=6 * EPS[dtype], rtol=6 * EPS[dtype], msg=lambda m: f"{form} flags {flags}: {m}")
            torch.testing.assert_close(lse[..., :L].cpu().double(), ref_lse, atol=1e-3, rtol=1e-4, msg=lambda m: f"{form} flags {flags}: {m}")
            fwd = fwd or (out, lse)
            continue
        dqkv, delta = run.bwd(flags, form, *fwd)
        torch.testing.assert_close(dqkv.cpu().double(), dref, atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype], msg=lambda m: f"{form} flags {flags}: {m}")
        check_delta(delta, fwd[0], dout, H)
        again, _ = run.bwd(flags, form, *fwd)
        assert same_bits(again, dqkv), f"{form} flags {flags}: two runs differ"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,H,causal,positions", ATTN_SINGLE_EDGE_CASES)
def test_attention_single_query_edges_guarded(lib, dtype, B, L, H, causal, positions):
    """The single-query forms at causal position 0 (one visible key), position L - 1 and L = 1, every compact operand (q_sel, dout_sel, out_sel)
    between NaN rows and every output (out_sel, lse_sel, dq_sel, dqkv) between sentinels; the q third of dqkv stays unwritten."""
    dt, tt = DT[dtype]
    Hd = H * 64
    qkv, _ = inputs(B, L, H, tt, 100 * B + L)
    pos = torch.tensor(positions if causal else [0] * B)
    assert len(pos) == B
    rows = torch.arange(B)
    dsel = torch.randn(B, Hd, generator=torch.Generator().manual_seed(L)).to(tt)
    dout = torch.zeros(B, L, Hd, dtype=tt)
    dout[rows, pos] = dsel
    ref_out, ref_lse, dref = attn64_fwd_bwd(qkv, dout, H, causal)
    _, qc = guarded(qkv.shape, tt, NAN, qkv)
    _, q_sel = guarded((B, Hd), tt, NAN, qkv[rows, pos, :Hd])
    sel = (rows * L + pos).to(torch.int32).cuda()
    obuf, out_sel = guarded((B, Hd), tt, SENT)
    lbuf, lse_sel = guarded((B, H), torch.float32, SENT)
    ok(lib, capi.call("mudpt_attention_fwd_single", dtype=dt, qkv=qc, q_sel=q_sel, sel_rows=sel, out_sel=out_sel, lse_sel=lse_sel, B=B, L=L, H=H, causal=int(causal)))
    assert_guards(obuf, out_sel, SENT, "out_sel")
    assert_guards(lbuf, lse_sel, SENT, "lse_sel")
    torch.testing.assert_close(out_sel.cpu().double(), ref_out[rows, pos], atol=6 * EPS[dtype], rtol=6 * EPS[dtype])
    torch.testing.assert_close(lse_sel.cpu().double(), ref_lse[rows, :, pos], atol=1e-3, rtol=1e-4)
    _, o_in = guarded((B, Hd), tt, NAN)
    o_in.copy_(out_sel)
    _, d_in = guarded((B, Hd), tt, NAN, dsel)
    scale = dref.abs().max().item()
    tol = dict(atol=12 * EPS[dtype] * scale, rtol=8 * EPS[dtype])
    res = []
    for _ in range(2):
        dbuf, dqkv = guarded((B, L, 3 * Hd), tt, SENT)
        qbuf, dq_sel = guarded((B, Hd), tt, SENT)
        ok(lib, lib.mudpt_attention_bwd_single(dt, P(qc), P(q_sel), P(sel), P(o_in), P(d_in), P(lse_sel), P(dqkv), P(dq_sel), B, L, H, int(causal), None))
        assert_guards(dbuf, dqkv, SENT, "dqkv")
        assert_guards(qbuf, dq_sel, SENT, "dq_sel")
        assert dqkv[..., :Hd].isnan().all(), "the q third of dqkv must stay unwritten"
        torch.testing.assert_close(dq_sel.cpu().double(), dref[rows, pos, :Hd], **tol)
        torch.testing.assert_close(dqkv[..., Hd:].cpu().double(), dref[..., Hd:], **tol)  # every key row, zeros behind the causal limit
        res.append((dqkv[..., Hd:].clone(), dq_sel))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
