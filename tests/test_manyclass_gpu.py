"""GPU parity and full-size properties for the many-class workloads (BASELINE configs[2]: C = 1000; configs[3] and [4] at full size).

With hundreds of class prompts the text tower stops being a handful of small launches: its GEMMs go through the persistent
256 x 256 kernel and its half tiles, fp16 mode contracts split [hi | lo] operands at large M, ``reduce_rows`` sums over hundreds of
sequences, the trimmed length Le = max(EOT) + 1 is 20-26 instead of 9 with a different EOT row per class, and the cross-entropy runs
over hundreds of columns.  Pins:

* ``mudpt_vitb16_c208_b2`` -- a fixture generated from the REFERENCE's own modules (tests/golden/gen_golden.py --many-only):
  208 class prompts of 1-9 words (EOT positions 7..25), B = 2: logits, loss, all ten gradients;
* C = 1000 (``synth.synthetic_tokenized_prompts``) against the CPU oracle (itself pinned by the fixture above at C = 208;
  no reference fixture at C = 1000: "parity unpinned" beyond the oracle);
* the full sizes of BASELINE configs[2], [3], [4], where the oracle is too slow, through size-independent properties: images are
  independent units, so logits of a batch equal the logits of its chunks BIT FOR BIT and follow a permutation of the images; the
  loss is the mean of the chunk losses; every gradient is finite and the batch gradient is the mean of the chunk gradients.
"""
import pytest
import torch

from oracle import mudpt_oracle as O
from tests.helpers import GoldenCase, assert_training_forward_is_the_inference_forward, check_grads

pytestmark = pytest.mark.gpu

LOGIT_RMS = {"fp16": 5e-4, "bf16": 1.6e-2}   # as tests/test_model_gpu.py (north_star: 1e-3 on fp16 logits)
LOGIT_ATOL = {"fp16": 1e-3, "bf16": 3.2e-2}
GRAD_RTOL = {"fp16": 2e-2, "bf16": 1.5e-1}   # relative to each gradient tensor's RMS (max error <= 4x that, cosine below)


def build(cfg, frozen, tokens, params, dtype, max_batch, knobs=None):
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape.from_config(cfg, cfg.n_ctx, cfg.depth)
    m = CustomCLIP(shape, frozen, tokens, max_batch=max_batch, dtype=dtype, knobs=knobs)
    m.set_params(params)
    return m


MAX_AND_COSINE = {"rms_err": False, "cos": True}  # what this suite and the class-parallel one ask of helpers.check_grads: the largest error and the direction


# ---- 208 classes: the reference's own numbers ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case208():
    c = GoldenCase("mudpt_vitb16_c208_b2")
    # full gradients from the oracle (the fixture stores strided samples of the three big Linear weights); the oracle itself is held
    # to the fixture on CPU (tests/test_oracle_golden.py::test_many_class_fixture_matches_reference)
    _, _, c.oracle_grads = O.forward_backward(c.cfg, c.frozen, c.params, c.class_embedding, c.eot, c.images, c.labels)
    return c


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_c208_logits_loss_grads_match_reference(case208, dtype):
    case = case208
    m = build(case.cfg, case.frozen, case.tokens, case.params, dtype, len(case.labels))
    rows, buckets, Le = m.text_layout()
    assert Le == int(case.eot.max()) + 1 and Le >= 17  # the trimmed text tower runs well past the 9 positions of the 11-class cases
    assert buckets > 1 and rows < 208 * Le  # and in length buckets: this test pins the bucketed tower to the reference's numbers
    loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
    torch.cuda.synchronize()
    d = logits.cpu() - case.logits
    err, rms = d.abs().max().item(), d.pow(2).mean().sqrt().item()
    print(f"C=208 {dtype}: |logit - reference| max {err:.3e} rms {rms:.3e}")
    assert err <= LOGIT_ATOL[dtype] and rms <= LOGIT_RMS[dtype], (err, rms)
    assert abs(loss.item() - case.loss) <= LOGIT_ATOL[dtype]
    got = {k: v.detach().cpu() for k, v in m.grads().items()}
    check_grads(got, case.oracle_grads, dtype, f"C=208 {dtype}", **MAX_AND_COSINE)
    for k in O.TRAINABLE_ORDER:  # and directly against the reference's autograd where the fixture holds the tensor / its sample
        full, sample = case.grad(k), case.grad_sample(k)
        rms_g = case.oracle_grads[k].pow(2).mean().sqrt().item()
        if full is not None:
            assert (got[k] - full).abs().max().item() <= GRAD_RTOL[dtype] * rms_g * 4 + 1e-9, k
        else:
            assert (got[k][::8, ::8] - sample).abs().max().item() <= GRAD_RTOL[dtype] * rms_g * 4 + 1e-9, k
    assert_training_forward_is_the_inference_forward(logits, m(case.images), dtype)  # forward-only call: same kernels; a 2-image training batch splits K
    m.close()


def test_c208_text_tower_trim_changes_nothing(case208):
    """Le = 26 of 77 positions with a different EOT row per class: logits, loss and gradients equal the untrimmed run up to the
    summation order inside attention (fp16 mode: split operands through the large-M GEMMs in both runs)."""
    case, out = case208, {}
    for trim in (1, 0):
        m = build(case.cfg, case.frozen, case.tokens, case.params, "fp16", 2, knobs={"txt_trim": trim})
        loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
        out[trim] = (logits.cpu(), loss.item(), {k: g.detach().cpu().clone() for k, g in m.grads().items()})
        m.close()
    torch.testing.assert_close(out[1][0], out[0][0], atol=2e-5, rtol=0)
    assert abs(out[1][1] - out[0][1]) < 2e-6
    for k, g in out[0][2].items():
        scale = g.pow(2).mean().sqrt().item()
        print(f"trim vs no trim, {k}: max diff {(out[1][2][k] - g).abs().max().item() / max(scale, 1e-30):.2e} x rms")
        torch.testing.assert_close(out[1][2][k], g, atol=2e-4 * scale + 1e-12, rtol=0, msg=k)


def test_c208_length_buckets_change_nothing(case208):
    """The class prompts sorted by length and run in 2-4 buckets, each to its own longest EOT, against the single-bucket run (every prompt to
    position 25): sequences are independent in every kernel of the tower, so the text features -- hence the logits and the loss -- are
    BIT-identical; the gradients differ by the order of the fp32 sums over classes only."""
    case, out, rows = case208, {}, {}
    for nb in (1, 2, 3, 4):
        # txt_bucket_cost 0: cut wherever it saves a row (the default charges 1024 rows per extra bucket and stops at 2 here)
        m = build(case.cfg, case.frozen, case.tokens, case.params, "fp16", 2, knobs={"txt_buckets": nb, "txt_bucket_cost": 0})
        rows[nb] = m.text_layout()
        loss, logits = m.forward_backward(case.images, case.labels, return_logits=True)
        torch.cuda.synchronize()
        out[nb] = (logits.cpu(), loss.item(), {k: g.detach().cpu().clone() for k, g in m.grads().items()})
        m.eval()
        assert_training_forward_is_the_inference_forward(out[nb][0], m(case.images), "fp16")
        m.close()
    print("text layouts (rows, buckets, longest):", rows)
    assert rows[1][1] == 1 and rows[1][0] == 208 * rows[1][2]
    assert all(rows[nb][1] == nb for nb in (2, 3, 4)) and rows[4][0] < rows[3][0] < rows[2][0] < 0.8 * rows[1][0]
    for nb in (2, 3, 4):
        assert torch.equal(out[nb][0], out[1][0]) and out[nb][1] == out[1][1], nb
        for k, g in out[1][2].items():
            scale = g.pow(2).mean().sqrt().item()
            assert (out[nb][2][k] - g).abs().max().item() <= 2e-5 * scale + 1e-12, (nb, k)


# ---- 1000 classes against the oracle -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1000():
    """Inputs by the seeded recipe, expected outputs from the stored ORACLE fixture (tests/golden/gen_oracle_c1000.py; the oracle is
    deterministic, and recomputing it here cost 65 s of the GPU suite).  tests/test_oracle_golden.py re-derives the fixture's logits on the
    CPU, so a changed oracle cannot leave it stale."""
    import os
    import numpy as np
    from tests.golden import gen_oracle_c1000 as G
    cfg, frozen, tok, params, images, labels = G.inputs()
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vitb16_c1000_b2.npz"), allow_pickle=False)
    assert int(z["tokens_checksum"]) == int(tok.sum())
    return dict(cfg=cfg, frozen=frozen, tok=tok, params=params, images=images, labels=labels, loss=float(z["loss"]), logits=torch.from_numpy(z["logits"]), z=z)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_c1000_against_the_oracle(case1000, dtype):
    """BASELINE configs[2]'s class count (synthetic names, long-tailed lengths, Le = 19-20), B = 2.  Reference fixtures stop at
    C = 208: beyond that the oracle is the pin ("parity unpinned" against the reference itself at this size)."""
    from tests.golden.gen_oracle_c1000 import SAMPLE
    c = case1000
    m = build(c["cfg"], c["frozen"], c["tok"], c["params"], dtype, 2)
    loss, logits = m.forward_backward(c["images"], c["labels"], return_logits=True)
    torch.cuda.synchronize()
    d = logits.cpu() - c["logits"]
    err, rms = d.abs().max().item(), d.pow(2).mean().sqrt().item()
    print(f"C=1000 {dtype}: |logit - oracle| max {err:.3e} rms {rms:.3e}, loss {loss.item():.6f} vs {c['loss']:.6f}")
    assert err <= LOGIT_ATOL[dtype] and rms <= LOGIT_RMS[dtype], (err, rms)
    assert abs(loss.item() - c["loss"]) <= LOGIT_ATOL[dtype]
    z = c["z"]
    for k, g in m.grads().items():
        g = g.detach().cpu()
        rms_g = float(z["grad_stats." + k][0])  # RMS of the oracle's FULL tensor
        if "grad." + k in z.files:
            r = torch.from_numpy(z["grad." + k])
        else:  # the three big Linear weights: a [::4, ::4] sample of the oracle's gradient
            r, g = torch.from_numpy(z["grad_sample." + k]), g[::SAMPLE, ::SAMPLE]
        e = (g - r).abs().max().item()
        cos = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
        print(f"C=1000 {dtype} {k}: rms {rms_g:.3e} max err {e / rms_g:.3e} x rms, cos {cos:.6f}")
        assert e <= GRAD_RTOL[dtype] * rms_g * 4 + 1e-9, (k, e, rms_g)
        assert cos > (0.9995 if dtype == "fp16" else 0.99), (k, cos)
    m.close()


# ---- full sizes: properties ----------------------------------------------------------------------------------------------------
def batch_properties(m, images, labels, chunk, grad_rel):
    """Images are independent units: chunk / permutation equality of the logits bit for bit, loss = mean of the chunk
    losses, finite gradients, batch gradient = mean of the chunk gradients (to the T-precision noise of two differently scaled sums)."""
    B, g = images.shape[0], torch.Generator().manual_seed(5)
    m.eval()
    full = m(images)
    assert torch.isfinite(full).all() and full.shape == (B, m.n_cls)
    chunks = torch.cat([m(images[i:i + chunk]) for i in range(0, B, chunk)])
    assert torch.equal(full, chunks)
    perm = torch.randperm(B, generator=g).cuda()
    assert torch.equal(m(images[perm]), full[perm])
    m.train()
    loss, logits = m.forward_backward(images, labels, return_logits=True)
    assert torch.equal(logits, full)  # the training step's forward is the same computation
    loss = loss.item()
    ref_loss = torch.nn.functional.cross_entropy(full.double(), labels).item()
    assert abs(loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)  # the fused CE head against torch on the library's own logits
    grad = m.flat_grads.clone()
    assert torch.isfinite(grad).all()
    n = B // chunk
    acc, losses = torch.zeros_like(grad), []
    for i in range(0, B, chunk):
        losses.append(m.forward_backward(images[i:i + chunk], labels[i:i + chunk]).item())
        acc += m.flat_grads / n
    assert abs(loss - sum(losses) / n) <= 1e-5 * max(1.0, abs(loss))
    off = 0
    for k, p in m.named_parameters():
        a, b = grad[off:off + p.numel()], acc[off:off + p.numel()]
        off += p.numel()
        rms = a.pow(2).mean().sqrt().item()
        assert rms > 0, k
        assert (a - b).pow(2).mean().sqrt().item() <= grad_rel * rms, k


def test_full_size_c1000_properties_bf16():
    """BASELINE configs[2] per GPU: ViT-B/16, B = 256, C = 1000, bf16."""
    from mudpt_amd import synth
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape()
    m = CustomCLIP(shape, synth.random_clip_state(shape, seed=0), synth.synthetic_tokenized_prompts(1000), ctx_token_ids=synth.CTX_INIT_TOKENS,
                   max_batch=256, dtype="bf16", seed=1)
    g = torch.Generator().manual_seed(11)
    images, labels = torch.randn(256, 3, 224, 224, generator=g).cuda(), torch.randint(0, 1000, (256,), generator=g).cuda()
    batch_properties(m, images, labels, 64, 0.1)
    m.close()


def test_full_size_vitl14_336_c1000_properties_bf16():
    """BASELINE configs[4] per GPU: ViT-L/14@336, depth 24, B = 128, C = 1000, bf16 (tiled attention at L = 581)."""
    from mudpt_amd import synth
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape(image_size=336, patch=14, v_width=1024, v_layers=24, v_heads=16, t_width=768, t_layers=12, t_heads=12, embed_dim=768, n_ctx=4, depth=24)
    m = CustomCLIP(shape, synth.random_clip_state(shape, seed=0), synth.synthetic_tokenized_prompts(1000), ctx_token_ids=synth.CTX_INIT_TOKENS,
                   max_batch=128, dtype="bf16", seed=1)
    g = torch.Generator().manual_seed(12)
    images, labels = torch.randn(128, 3, 336, 336, generator=g).cuda(), torch.randint(0, 1000, (128,), generator=g).cuda()
    batch_properties(m, images, labels, 32, 0.1)
    m.close()


def test_full_size_cocoop_b64_properties_bf16():
    """BASELINE configs[3]: CoCoOp ViT-B/16, B = 64, C = 11 (704 text sequences per step), bf16."""
    from oracle import cocoop_oracle as CO
    from mudpt_amd import synth
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape(depth=1)
    m = CustomCLIP(shape, synth.random_clip_state(shape, seed=0), synth.bench_tokenized_prompts(), ctx_token_ids=synth.CTX_INIT_TOKENS,
                   max_batch=64, dtype="bf16", seed=1, variant="cocoop")
    assert m.param_names == CO.TRAINABLE_ORDER
    g = torch.Generator().manual_seed(13)
    images, labels = torch.randn(64, 3, 224, 224, generator=g).cuda(), torch.randint(0, 11, (64,), generator=g).cuda()
    # meta_net's gradients are sums of nearly cancelling per-class terms (tests/test_cocoop_gpu.py): bf16 noise is amplified
    batch_properties(m, images, labels, 16, 0.35)
    m.close()


def test_full_size_exact_mode_properties():
    """BASELINE configs[1]'s size (ViT-B/16, B = 256, C = 11) in the EXACT mode (dtype "fp32"): the split-operand GEMMs at M = 51 456 (the
    persistent kernel's fp32 and [hi | lo] epilogues), the fp32 attention forward over 3072 (sequence, head) pairs, the [hi | lo] patch
    rows -- held to the same size-independent properties as the bf16 runs (chunk / permutation equality of the logits bit for bit, loss =
    mean of chunk losses, batch gradient = mean of chunk gradients), with the fp16 backward's noise level."""
    from mudpt_amd import synth
    from mudpt_amd.model import CustomCLIP, ModelShape
    shape = ModelShape()
    m = CustomCLIP(shape, synth.random_clip_state(shape, seed=0), synth.bench_tokenized_prompts(), ctx_token_ids=synth.CTX_INIT_TOKENS,
                   max_batch=256, dtype="fp32", seed=1)
    g = torch.Generator().manual_seed(14)
    images, labels = torch.randn(256, 3, 224, 224, generator=g).cuda(), torch.randint(0, 11, (256,), generator=g).cuda()
    batch_properties(m, images, labels, 64, 0.02)
    m.close()
