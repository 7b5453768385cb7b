"""The fp32 kernels of UMuDPT's prompt generator (mudpt_amd/csrc/promptgen.hip) one by one through the C ABI, and the whole generator
(mudpt_promptgen_forward / _backward: the code the model path runs), against float64 references.  Destinations are sentinel-filled, so
a write outside the result shows."""
import dataclasses
import math

import pytest
import torch

from mudpt_amd import capi
from oracle import mudpt_oracle as O
from tests import umudpt_reference as R
from tests.helpers import SENT, P, ok, refused

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def bits(t):
    return t.contiguous().view(torch.int32)


def ln_fwd(lib, x, gamma, beta):
    rows, d = x.shape
    y, mean, rstd = torch.empty(rows, d, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    ok(lib, capi.call("mudpt_layernorm_fwd", dtype=1, x=x, ldx=d, gamma=gamma, beta=beta, out=y, ldo=d, out_f32=1, mean=mean, rstd=rstd, rows=rows, d=d))
    return y, mean, rstd


@pytest.mark.parametrize("rows,d", [(1, 128), (2, 128), (16, 512), (96, 512), (7, 768), (384, 512)])
def test_ln_bwd_affine(lib, rows, d):
    """dx as test_layernorm_fwd_bwd checks it (atol = rtol = 2e-5, with the residual gradient added); dgamma = sum_r dy xhat and
    dbeta = sum_r dy against float64 with test_colsum's bound for a sum of `rows` unit-variance terms, 4e-6 sqrt(rows) (dy and xhat are
    both unit-variance, and so is their product); accumulate = the plain result plus the old contents in ONE fp32 add; two runs agree bit
    for bit (fixed order, no atomics)."""
    g = torch.Generator().manual_seed(rows * 1000 + d)
    x = torch.randn(rows, d, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    dy, dres = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    torch.nn.functional.layer_norm(x64, (d,), g64, b64, 1e-5).backward(dy.double())
    xc, gc, bc, dyc, drc = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda(), dres.cuda()
    _, mean, rstd = ln_fwd(lib, xc, gc, bc)

    def run(accumulate, dgamma, dbeta, with_dres=True):
        dx = torch.full((rows + 1, d), SENT, device="cuda")
        ok(lib, lib.mudpt_layernorm_bwd_affine(P(xc), d, P(mean), P(rstd), P(gc), P(dyc), d, P(drc) if with_dres else None, d, P(dx), d,
                                               P(dgamma), P(dbeta), accumulate, rows, d, None))
        return dx.cpu()
    dga, dbe = torch.full((d + 3,), SENT, device="cuda"), torch.full((d + 3,), SENT, device="cuda")
    dx = run(0, dga, dbe)
    assert (dx[rows] == SENT).all() and (dga[d:] == SENT).all() and (dbe[d:] == SENT).all()
    torch.testing.assert_close(dx[:rows].double(), x64.grad + dres.double(), atol=2e-5, rtol=2e-5)
    tol = 4e-6 * rows ** 0.5
    eg, eb = (dga[:d].cpu().double() - g64.grad).abs().max().item(), (dbe[:d].cpu().double() - b64.grad).abs().max().item()
    print(f"ln_bwd_affine {rows}x{d}: dgamma err {eg:.2e} dbeta err {eb:.2e} (bound {tol:.2e})")
    assert eg <= tol and eb <= tol
    # without the residual gradient
    dga0, dbe0 = torch.full((d + 3,), SENT, device="cuda"), torch.full((d + 3,), SENT, device="cuda")
    dx0 = run(0, dga0, dbe0, with_dres=False)
    torch.testing.assert_close(dx0[:rows].double(), x64.grad, atol=2e-5, rtol=2e-5)
    assert torch.equal(bits(dga0), bits(dga)) and torch.equal(bits(dbe0), bits(dbe))
    # accumulate: ONE fp32 add onto the previous contents
    prev_g, prev_b = torch.randn(d + 3, generator=g), torch.randn(d + 3, generator=g)
    acc_g, acc_b = prev_g.clone().cuda(), prev_b.clone().cuda()
    dx2 = run(1, acc_g, acc_b)
    assert torch.equal(bits(acc_g[:d].cpu()), bits(prev_g[:d] + dga[:d].cpu())) and torch.equal(acc_g[d:].cpu(), prev_g[d:])
    assert torch.equal(bits(acc_b[:d].cpu()), bits(prev_b[:d] + dbe[:d].cpu())) and torch.equal(acc_b[d:].cpu(), prev_b[d:])
    # two runs: bit-identical
    dga2, dbe2 = torch.full((d + 3,), SENT, device="cuda"), torch.full((d + 3,), SENT, device="cuda")
    dx3 = run(0, dga2, dbe2)
    assert torch.equal(bits(dx3), bits(dx)) and torch.equal(bits(dx2), bits(dx))
    assert torch.equal(bits(dga2), bits(dga)) and torch.equal(bits(dbe2), bits(dbe))


def test_ln_bwd_affine_refusals(lib):
    f = lambda *s: torch.full(s, SENT, device="cuda")  # noqa: E731
    x, st, gm, out, dg = f(4, 128), f(4), f(128), f(4, 128), f(128)
    call = lambda **k: lib.mudpt_layernorm_bwd_affine(  # noqa: E731
        P(k.get("x", x)), k.get("ldx", 128), P(st), P(st), P(gm), P(x), k.get("lddy", 128), None, 0, P(out), k.get("lddx", 128), P(k.get("dg", dg)), P(dg),
        0, k.get("rows", 4), k.get("d", 128), None)
    refused(lib, call(x=None), "ln_bwd_affine")
    refused(lib, call(dg=None), "ln_bwd_affine")
    refused(lib, call(rows=0), "ln_bwd_affine")
    refused(lib, call(d=126), "ln_bwd_affine")
    refused(lib, call(d=2048, ldx=2048, lddy=2048, lddx=2048), "ln_bwd_affine")
    refused(lib, call(ldx=64), "ln_bwd_affine")
    refused(lib, call(lddx=64), "ln_bwd_affine")
    assert (out == SENT).all() and (dg == SENT).all()


ATTN_ATOL, ATTN_RTOL = 3e-5 * math.sqrt(64), 1e-5  # test_sgemm's fp32 bound for a contraction of 64 unit-variance products


@pytest.mark.parametrize("N,H,L", [(1, 1, 1), (3, 2, 2), (8, 8, 2), (12, 8, 4), (5, 3, 7), (2, 12, 16)])
def test_pg_attention_fwd_bwd(lib, N, H, L):
    """softmax(q k^T / 8) v over the L rows of one sequence, no mask, and its backward, against float64 attention and its autograd."""
    d = H * 64
    g = torch.Generator().manual_seed(N * 100 + H * 10 + L)
    qkv, dout = torch.randn(N, L, 3 * d, generator=g), torch.randn(N, L, d, generator=g)
    q64 = qkv.double().requires_grad_(True)
    ref = O.attention(q64, H, None)
    ref.backward(dout.double())
    qc, dc = qkv.cuda(), dout.cuda()
    out, probs = torch.full((N * L + 1, d), SENT, device="cuda"), torch.full((N * H * L * L + 3,), SENT, device="cuda")
    ok(lib, lib.mudpt_pg_attention_fwd(P(qc), P(out), P(probs), N, L, H, d, None))
    assert (out[N * L] == SENT).all() and (probs[N * H * L * L:] == SENT).all()
    torch.testing.assert_close(out[:N * L].cpu().double().view(N, L, d), ref.detach(), atol=ATTN_ATOL, rtol=ATTN_RTOL)
    p = probs[:N * H * L * L].cpu().view(N, H, L, L)
    assert (p.sum(-1) - 1).abs().max().item() <= 1e-6 and (p >= 0).all()
    dqkv = torch.full((N * L + 1, 3 * d), SENT, device="cuda")
    ok(lib, lib.mudpt_pg_attention_bwd(P(qc), P(probs), P(dc), P(dqkv), N, L, H, d, None))
    assert (dqkv[N * L] == SENT).all()
    err = (dqkv[:N * L].cpu().double().view(N, L, 3 * d) - q64.grad).abs().max().item()
    print(f"pg_attention N={N} H={H} L={L}: out err {(out[:N * L].cpu().double().view(N, L, d) - ref.detach()).abs().max().item():.2e} dqkv err {err:.2e}")
    torch.testing.assert_close(dqkv[:N * L].cpu().double().view(N, L, 3 * d), q64.grad, atol=ATTN_ATOL, rtol=ATTN_RTOL)
    dqkv2 = torch.full((N * L + 1, 3 * d), SENT, device="cuda")
    ok(lib, lib.mudpt_pg_attention_bwd(P(qc), P(probs), P(dc), P(dqkv2), N, L, H, d, None))
    assert torch.equal(bits(dqkv2), bits(dqkv))


def test_pg_attention_refusals(lib):
    f = lambda *s: torch.full(s, SENT, device="cuda")  # noqa: E731
    qkv, out, probs = f(2 * 17, 3 * 128), f(2 * 17, 128), f(2 * 2 * 17 * 17)
    refused(lib, lib.mudpt_pg_attention_fwd(P(qkv), P(out), P(probs), 2, 17, 2, 128, None), "L=17")
    refused(lib, lib.mudpt_pg_attention_bwd(P(qkv), P(probs), P(out), P(qkv), 2, 17, 2, 128, None), "L=17")
    refused(lib, lib.mudpt_pg_attention_fwd(P(qkv), P(out), P(probs), 2, 0, 2, 128, None), "pg_attn_fwd")
    refused(lib, lib.mudpt_pg_attention_fwd(P(qkv), P(out), P(probs), 2, 4, 0, 0, None), "pg_attn_fwd")      # H < 1
    refused(lib, lib.mudpt_pg_attention_fwd(P(qkv), P(out), P(probs), 2, 4, 2, 96, None), "pg_attn_fwd")     # d_t % 64
    refused(lib, lib.mudpt_pg_attention_fwd(P(qkv), P(out), P(probs), 2, 4, 2, 192, None), "pg_attn_fwd")    # d_t != H * 64
    refused(lib, lib.mudpt_pg_attention_fwd(P(qkv), None, P(probs), 2, 4, 2, 128, None), "null")
    refused(lib, lib.mudpt_pg_attention_bwd(P(qkv), None, P(out), P(qkv), 2, 4, 2, 128, None), "null")
    refused(lib, lib.mudpt_pg_attention_fwd(P(qkv), P(out), P(probs), 0, 4, 2, 128, None), "pg_attn_fwd")
    assert (out == SENT).all() and (probs == SENT).all() and (qkv == SENT).all()


@pytest.mark.parametrize("n", [5, 16 * 2048 + 3])
def test_quickgelu(lib, n):
    """y = u sigmoid(1.702 u) with u spanning +-12: relative error <= 1e-5 against float64 (an exp, a divide and two or three multiplies
    at fp32's epsilon 6e-8; at |u| = 12 the exponent's argument, 20, multiplies its own rounding: still fourfold margin).  The backward
    du = dy QuickGELU'(u), QuickGELU'(u) = s + 1.702 u s (1 - s), has a ZERO at u = -0.7525 where its two terms cancel and no fp32
    evaluation holds an elementwise relative bound; it is held to 1e-5 of |dy| (|s| + |1.702 u s (1 - s)|), the magnitude of the terms,
    which is the elementwise relative bound wherever they do not cancel."""
    u = torch.linspace(-12.0, 12.0, n)
    g = torch.Generator().manual_seed(n)
    dy = torch.randn(n, generator=g)
    u64 = u.double()
    s = torch.sigmoid(1.702 * u64)
    y_ref, t1, t2 = u64 * s, s, 1.702 * u64 * s * (1 - s)
    uc, dyc = u.cuda(), dy.cuda()
    y, du = torch.full((n + 3,), SENT, device="cuda"), torch.full((n + 3,), SENT, device="cuda")
    ok(lib, lib.mudpt_quickgelu_fwd(P(uc), P(y), n, None))
    ok(lib, lib.mudpt_quickgelu_bwd(P(dyc), P(uc), P(du), n, None))
    assert (y[n:] == SENT).all() and (du[n:] == SENT).all()
    ey = ((y[:n].cpu().double() - y_ref).abs() / y_ref.abs().clamp_min(1e-300)).max().item()
    ed = ((du[:n].cpu().double() - dy.double() * (t1 + t2)).abs() / (dy.double().abs() * (t1.abs() + t2.abs())).clamp_min(1e-300)).max().item()
    print(f"quickgelu n={n}: fwd rel err {ey:.2e} bwd rel err {ed:.2e}")
    assert ey <= 1e-5 and ed <= 1e-5
    inplace = dyc.clone()  # du may be dy
    ok(lib, lib.mudpt_quickgelu_bwd(P(inplace), P(uc), P(inplace), n, None))
    assert torch.equal(bits(inplace), bits(du[:n]))
    refused(lib, lib.mudpt_quickgelu_fwd(P(uc), P(y), 0, None), "quickgelu_fwd")
    refused(lib, lib.mudpt_quickgelu_bwd(P(dyc), None, P(du), n, None), "quickgelu_bwd")


GEN_SHAPES = [(3, 2, 128, 192), (1, 3, 128, 192), (8, 2, 512, 768), (12, 4, 512, 768)]


@pytest.fixture(scope="module", params=GEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def gen_case(request):
    """Seeded parameters (non-degenerate LayerNorms and biases), X = cat(ctx, deep_prompts), a unit-variance dG and the float64 reference
    of the generator and its autograd, computed once per shape."""
    depth, n, d, dv = request.param
    cfg = dataclasses.replace(O.TINY, n_ctx=n, depth=depth, t_width=d, v_width=dv)
    params = R.seeded_params(cfg, 100 + depth)
    X = R.prompt_tables(params)
    dG = torch.randn(depth, n, dv, generator=torch.Generator().manual_seed(depth))
    G, dX, grads = R.generator_backward(params, X, dG)
    keys = [k for k, _ in R.trainable_keys(cfg)][2:]
    return dict(shape=request.param, params=params, X=X, dG=dG, G=G, dX=dX, grads=grads, keys=keys)


def test_promptgen_forward_backward(lib, gen_case):
    """G, dX and the 18 weight / bias / gamma / beta gradients against tests/umudpt_reference.generator in float64 and its autograd.  Every
    output is held to test_sgemm's fp32 bound at the longest contraction on its path, c_proj's 4 d_t: atol 3e-5 sqrt(4 d_t), rtol 1e-5."""
    depth, n, d, dv = gen_case["shape"]
    R_, keys = depth * n, gen_case["keys"]
    flat = torch.cat([gen_case["params"][k].reshape(-1) for k in keys])
    assert lib.mudpt_promptgen_param_numel(d, dv) == flat.numel()
    ws_n = lib.mudpt_promptgen_workspace(depth, n, d, dv)
    ws = torch.zeros(ws_n, device="cuda")
    pc, Xc, dGc = flat.cuda(), gen_case["X"].reshape(R_, d).contiguous().cuda(), gen_case["dG"].reshape(R_, dv).contiguous().cuda()
    G = torch.full((R_ + 1, dv), SENT, device="cuda")
    ok(lib, lib.mudpt_promptgen_forward(depth, n, d, dv, P(pc), P(Xc), P(G), P(ws), ws_n, None))
    assert (G[R_] == SENT).all()
    atol, rtol = 3e-5 * math.sqrt(4 * d), 1e-5
    eG = (G[:R_].cpu().double() - gen_case["G"].reshape(R_, dv)).abs().max().item()
    torch.testing.assert_close(G[:R_].cpu().double(), gen_case["G"].reshape(R_, dv), atol=atol, rtol=rtol)
    dX, grads = torch.full((R_ + 1, d), SENT, device="cuda"), torch.full((flat.numel() + 5,), SENT, device="cuda")
    ok(lib, lib.mudpt_promptgen_backward(depth, n, d, dv, P(pc), P(Xc), P(dGc), P(dX), P(grads), P(ws), ws_n, None))
    assert (dX[R_] == SENT).all() and (grads[flat.numel():] == SENT).all()
    torch.testing.assert_close(dX[:R_].cpu().double(), gen_case["dX"].reshape(R_, d), atol=atol, rtol=rtol)
    off, worst = 0, (0.0, "")
    for k in keys:
        ref = gen_case["grads"][k]
        got = grads[off:off + ref.numel()].cpu().double().view_as(ref)
        off += ref.numel()
        err = (got - ref).abs().max().item()
        worst = max(worst, (err / (atol + rtol * ref.abs().max().item()), k))
        torch.testing.assert_close(got, ref, atol=atol, rtol=rtol, msg=lambda m, k=k: f"{k}: {m}")
    print(f"promptgen {gen_case['shape']}: G err {eG:.2e} (atol {atol:.2e}); worst gradient {worst[1]} at {worst[0]:.3f} of its bound")
    # the same call again: bit-identical (fixed-order sums everywhere)
    grads2, dX2 = torch.full_like(grads, SENT), torch.full_like(dX, SENT)
    ok(lib, lib.mudpt_promptgen_forward(depth, n, d, dv, P(pc), P(Xc), P(G), P(ws), ws_n, None))
    ok(lib, lib.mudpt_promptgen_backward(depth, n, d, dv, P(pc), P(Xc), P(dGc), P(dX2), P(grads2), P(ws), ws_n, None))
    assert torch.equal(bits(grads2), bits(grads)) and torch.equal(bits(dX2), bits(dX))


def test_promptgen_refusals(lib):
    ws = torch.zeros(lib.mudpt_promptgen_workspace(3, 2, 128, 192), device="cuda")
    f = lambda *s: torch.full(s, SENT, device="cuda")  # noqa: E731
    p, X, G = f(lib.mudpt_promptgen_param_numel(128, 192)), f(6, 128), f(6, 192)
    refused(lib, lib.mudpt_promptgen_forward(0, 2, 128, 192, P(p), P(X), P(G), P(ws), ws.numel(), None), "PROMPT_DEPTH")
    refused(lib, lib.mudpt_promptgen_forward(3, 17, 128, 192, P(p), P(X), P(G), P(ws), ws.numel(), None), "n_ctx 17")
    refused(lib, lib.mudpt_promptgen_forward(3, 2, 96, 192, P(p), P(X), P(G), P(ws), ws.numel(), None), "multiple of 64")
    refused(lib, lib.mudpt_promptgen_forward(3, 2, 128, 192, P(p), P(X), P(G), P(ws), ws.numel() - 1, None), "workspace")
    refused(lib, lib.mudpt_promptgen_forward(3, 2, 128, 192, None, P(X), P(G), P(ws), ws.numel(), None), "null")
    refused(lib, lib.mudpt_promptgen_backward(3, 2, 128, 192, P(p), P(X), P(G), None, P(p), P(ws), ws.numel(), None), "null")
    assert (G == SENT).all() and (p == SENT).all() and (ws == 0).all()
