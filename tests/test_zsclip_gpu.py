"""GPU tests of the zero-shot path (trainers/zsclip.py) through the C ABI: a frozen handle (``mudpt_create_frozen``) against the fixtures of the
reference's own ``ZeroshotCLIP`` / ``ZeroshotCLIP2`` (tests/golden/gen_golden_zsclip.py), its bitwise properties, its refusals, the two
kernels of zeroshot.hip against float64, and the two plugins end to end."""
import ctypes as C
import math

import pytest
import torch

from mudpt_amd import capi
from oracle import mudpt_oracle as O
from tests import zsclip_reference as R
from tests.helpers import SENT, P, check_logits, ok, refused

pytestmark = pytest.mark.gpu
PARITY = [f for f in R.FIXTURES if not f.endswith("_s100")]
S100 = [f for f in R.FIXTURES if f.endswith("_s100")]

# encode_image against the fixtures' raw image_features: max over the images of |F - ref| / |ref|.  The project had no bound for the raw
# features; these are TWICE the values measured on the first MI355X run against the fixtures (the run is deterministic, the margin is for
# toolchain changes).  Measured, (3-layer tiny shape, ViT-B/16):
ENCODE_REL_MEASURED = {"fp16": (2.746e-4, 1.840e-4), "bf16": (3.391e-3, 2.298e-3), "fp32": (None, 3.347e-5)}  # fp32: the ViT-B/16 _s100 fixtures only
ENCODE_REL_BOUND = {k: tuple(None if x is None else 2 * x for x in v) for k, v in ENCODE_REL_MEASURED.items()}


def build(case, dtype, max_batch=None, knobs=None, tokens=None):
    from mudpt_amd.zsclip import FrozenCLIP
    return FrozenCLIP(case.shape(), case.frozen, case.tokens if tokens is None else tokens, max_batch=max_batch or len(case.labels), dtype=dtype, knobs=knobs)


def launches(m):
    return int(m.debug_read("text_launches")[0].item())


@pytest.fixture(scope="module")
def cases():
    return {}


def get(cases, name):
    if name not in cases:
        cases[name] = R.ZsCase(name)
    return cases[name]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", PARITY)
def test_logits_and_features_match_the_reference(cases, name, dtype):
    case = get(cases, name)
    m = build(case, dtype)
    logits = m(case.images).cpu()
    txt = m.text_features().cpu()
    raw = m.encode_image(case.images).cpu()
    m.close()
    rel = ((raw - case.image_features).norm(dim=-1) / case.image_features.norm(dim=-1)).max().item()
    print(f"{name} {dtype}: text features max {(txt - case.text_features).abs().max().item():.3e}; raw image features, relative: {rel:.3e}")
    check_logits(logits, case, dtype, f"{name} {dtype}")
    assert (txt.double().norm(dim=-1) - 1).abs().max().item() <= 1e-6
    bound = ENCODE_REL_BOUND[dtype][0 if case.cfg.v_layers < 12 else 1]
    assert bound is not None and rel <= bound, (rel, bound)


@pytest.mark.parametrize("name", S100)
def test_parity_mode_at_logit_scale_100(cases, name):
    case = get(cases, name)
    m = build(case, "fp32")
    logits = m(case.images).cpu()
    txt = m.text_features().cpu()
    raw = m.encode_image(case.images).cpu()
    m.close()
    err = (logits - case.logits).abs().max().item()
    rel = ((raw - case.image_features).norm(dim=-1) / case.image_features.norm(dim=-1)).max().item()
    print(f"{name} parity mode: |logit - reference| max {err:.3e}; raw image features, relative: {rel:.3e}")
    assert err <= 1e-3  # the project's stated bound
    assert (txt.double().norm(dim=-1) - 1).abs().max().item() <= 1e-6
    assert ENCODE_REL_BOUND["fp32"][1] is not None and rel <= ENCODE_REL_BOUND["fp32"][1], rel


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("name", ["zsclip2_tiny", "zsclip_vitb16_b2"])
def test_encode_image_is_what_the_logits_are_made_of(cases, name, dtype):
    """scale * normalise(encode_image) . text_features^T recomputed in float64 equals the handle's logits within the fp32 dot-product bound
    2 * scale * e * 2^-24: a wrong normalisation or a stale buffer is orders of magnitude outside it."""
    case = get(cases, name)
    m = build(case, dtype)
    F = m.encode_image(case.images).cpu().double()
    logits = m(case.images).cpu().double()
    assert torch.equal(m.debug_read("image_features", len(case.labels)).view(len(case.labels), -1).double(), F)
    txt = m.text_features().cpu().double()
    assert torch.equal(m.debug_read("text_features").view_as(txt).double(), txt)
    m.close()
    scale = math.exp(float(case.frozen["logit_scale"]))
    want = scale * (F / F.norm(dim=-1, keepdim=True)) @ txt.t()
    err = (logits - want).abs().max().item()
    print(f"{name} {dtype}: |logits - scale normalise(F) T^t| {err:.3e} (bound {2 * scale * case.cfg.embed_dim * 2.0 ** -24:.3e})")
    assert err <= 2 * scale * case.cfg.embed_dim * 2.0 ** -24


def test_encode_image_needs_no_tokens_and_forward_does(cases):
    case = get(cases, "zsclip_tiny")
    m = build(case, "fp16", tokens=torch.zeros(0, len(case.classnames), 77, dtype=torch.int32))
    F = m.encode_image(case.images)
    with pytest.raises(capi.MudptError, match="bad state"):
        m(case.images)
    with pytest.raises(capi.MudptError, match="bad state"):
        m.text_features()
    m.set_tokens(case.tokens)
    logits = m(case.images)
    m2 = build(case, "fp16")
    assert torch.equal(m2.encode_image(case.images), F) and torch.equal(m2(case.images), logits)
    m.close()
    m2.close()
    # the tokens before the embedding table: a call-order error
    lib, h = capi.load(), C.c_void_p()
    c = case.cfg
    cfg = capi.Config(c.image_size, c.patch, c.v_width, c.v_layers, c.v_heads, c.t_width, c.t_layers, c.t_heads, c.ctx_len, c.embed_dim, 0, 1,
                      len(case.classnames), 1, capi.F16, 0)
    ok(lib, lib.mudpt_create_frozen(C.byref(cfg), C.byref(h)))
    tok = case.tokens.contiguous()
    assert lib.mudpt_set_text_tokens(h, P(tok), 1) == 3 and b"token_embedding.weight" in lib.mudpt_last_error()
    lib.mudpt_destroy(h)


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_logits_of_an_image_do_not_depend_on_its_batch(cases, dtype):
    case = get(cases, "zsclip2_tiny")
    m = build(case, dtype)
    whole = m(case.images)
    for i in range(len(case.labels)):
        assert torch.equal(m(case.images[i:i + 1])[0], whole[i]), i
        assert torch.equal(m.encode_image(case.images[i:i + 1])[0], m.encode_image(case.images)[i]), i
    m.close()


def test_text_features_are_built_once_and_rebuilt_when_they_must(cases):
    case = get(cases, "zsclip2_tiny")
    m, m2 = build(case, "fp16"), build(case, "fp16")
    assert launches(m) == 0  # nothing runs before the first forward / text_features
    t1 = m.text_features()
    assert torch.equal(t1, m2.text_features())  # two handles, the same tokens: bit for bit
    first = launches(m)
    assert first == len(case.templates)
    logits = m(case.images)
    for _ in range(2):
        assert torch.equal(m(case.images), logits) and torch.equal(m.text_features(), t1)
    lib, img, again = m.lib, case.images.cuda(), torch.empty_like(logits)
    assert lib.mudpt_forward_ex(m._h, P(img), 3, P(again), capi.FWD_REUSE_TEXT, None) == 0  # accepted, changes nothing
    torch.cuda.synchronize()
    assert launches(m) == first and torch.equal(again, logits)
    w = case.frozen["ln_final.bias"] + 0.5
    m.set_weight("ln_final.bias", w)
    logits2 = m(case.images)
    assert launches(m) == 2 * first and not torch.equal(logits2, logits)
    m.set_tokens(case.tokens)
    logits3 = m(case.images)
    assert launches(m) == 3 * first and torch.equal(logits3, logits2)
    m.close()
    m2.close()


def bucket_tokens(vocab, seed=5):
    """96 prompts x 2 templates: ids random below the vocabulary's largest, which is used once per row as EOT -- at position 5 for one half of the
    prompts and 39 for the other, the halves swapped in the second template."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.zeros(2, 96, 77, dtype=torch.int32)
    for t in range(2):
        for c in range(96):
            eot = 5 if (c < 48) == (t == 0) else 39
            tok[t, c, :eot] = torch.randint(0, vocab - 1, (eot,), generator=g, dtype=torch.int32)
            tok[t, c, eot] = vocab - 1
    return tok


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_length_buckets_through_the_device_embedding(cases, dtype):
    """By the cut search's own arithmetic one bucket costs 96 * 40 + 1024 = 4864 rows and two cost 48 * 6 + 48 * 40 + 2 * 1024 = 4256: the default
    layout has 2 buckets per template, and its features equal the one-bucket and the untrimmed runs bit for bit."""
    case = get(cases, "zsclip_tiny")
    tok = bucket_tokens(case.cfg.vocab)
    assert (tok.argmax(dim=-1) == torch.where(tok == case.cfg.vocab - 1)[2].view(2, 96)).all()
    layouts, feats = {}, {}
    for key, knobs in (("default", None), ("one bucket", {"txt_buckets": 1}), ("untrimmed", {"txt_trim": 0})):
        m = build(case, dtype, knobs=knobs, tokens=tok)
        layouts[key], feats[key] = m.text_layout(), m.text_features().cpu()
        m.close()
    assert layouts["default"] == (2 * (48 * 6 + 48 * 40), 2, 40)
    assert layouts["one bucket"] == (2 * 96 * 40, 1, 40)
    assert layouts["untrimmed"] == (2 * 96 * 77, 1, 77)
    assert torch.isfinite(feats["default"]).all() and (feats["default"].double().norm(dim=-1) - 1).abs().max().item() <= 1e-6
    assert torch.equal(feats["default"], feats["one bucket"])
    assert torch.equal(feats["default"], feats["untrimmed"])
    # against the CPU restatement: the device embedding, the buckets' row tables and the scatter back all have to be right
    with torch.no_grad():
        ref = R.text_features(case.cfg, case.frozen, tok)
    err = (feats["default"] - ref).abs().max().item()
    print(f"bucketed text features {dtype}: max error against the restatement {err:.3e}")
    assert err <= (2e-3 if dtype == "fp16" else 3e-2)  # unit-norm features: the operand format's grade (2^-11 / 2^-8 relative per rounding, 3 blocks)


def test_a_frozen_handle_refuses_what_it_cannot_do(cases):
    case = get(cases, "zsclip_tiny")
    m = build(case, "fp16")
    lib, h = m.lib, m._h
    assert lib.mudpt_param_count(h) == 0 and lib.mudpt_param_numel(h) == 0
    assert list(m.parameters()) == [] and m.state_dict() == {}
    buf = torch.zeros(64, device="cuda")
    lab = torch.zeros(3, dtype=torch.int64, device="cuda")
    img = case.images.cuda()
    f, df, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    calls = {
        "bind_params": lambda: lib.mudpt_bind_params(h, P(buf), P(buf)),
        "forward_backward": lambda: lib.mudpt_forward_backward(h, P(img), P(lab), 3, 1.0, P(buf), None, None),
        "sgd_step": lambda: lib.mudpt_sgd_step(h, 0.1, 0.9, 0.0, 0.0, 0, None),
        "set_class_prompts": lambda: lib.mudpt_set_class_prompts(h, P(torch.zeros(4)), P(torch.zeros(4, dtype=torch.int32))),
        "set_class_token_position": lambda: lib.mudpt_set_class_token_position(h, 0, None),
        "set_class_shard": lambda: lib.mudpt_set_class_shard(h, 0, 1),
        "cp_buffers": lambda: lib.mudpt_cp_buffers(h, C.byref(f), C.byref(df), C.byref(n)),
        "cp_forward": lambda: lib.mudpt_cp_forward(h, P(img), 3, 0, None),
        "cp_head": lambda: lib.mudpt_cp_head(h, None, 3, 1.0, None, P(buf), 0, None),
        "cp_backward": lambda: lib.mudpt_cp_backward(h, capi.CP_VISION, None),
        "allreduce_grads": lambda: lib.mudpt_allreduce_grads(h, None, None),
    }
    for name, call in calls.items():
        refused(lib, call(), "frozen")
        assert name.split("_")[0] in lib.mudpt_last_error().decode(), name
    # an id outside the embedding table: equal to vocab, and negative
    for bad in (case.cfg.vocab, -1):
        tok = case.tokens.clone()
        tok[0, 2, 3] = bad
        refused(lib, lib.mudpt_set_text_tokens(h, P(tok), 1), "outside")
    refused(lib, lib.mudpt_set_text_tokens(h, P(case.tokens), 0), "n_templates")
    refused(lib, lib.mudpt_set_text_tokens(h, None, 1), "null")
    logits = m(case.images)  # the refused calls left the handle as it was
    m2 = build(case, "fp16")
    assert torch.equal(logits, m2(case.images))
    m.close()
    m2.close()
    # ... and the frozen entry points refuse every other handle
    from mudpt_amd.model import CustomCLIP, ModelShape
    c = O.TINY
    shape = ModelShape.from_config(c, c.n_ctx, c.depth)
    mm = CustomCLIP(shape, case.frozen, O.synthetic_tokens(c, 5).long(), max_batch=3, dtype="fp16")
    refused(lib, lib.mudpt_set_text_tokens(mm._h, P(case.tokens), 1), "not a frozen handle")
    refused(lib, lib.mudpt_text_features(mm._h, P(buf), None), "not a frozen handle")
    refused(lib, lib.mudpt_encode_image(mm._h, P(img), 3, P(buf), None), "not a frozen handle")
    mm.close()


EMBED_GRID_ROWS = 2048 * 4  # zeroshot.hip kEmbedMaxBlocks workgroups of 4 waves: one pass of the capped grid


@pytest.mark.parametrize("d", [128, 512, 768])
def test_embed_tokens_is_bit_exact(d):
    lib = capi.load()
    g = torch.Generator().manual_seed(d)
    vocab, npos = 37, 77
    table = torch.randn(vocab, d, generator=g).cuda()
    pos = (torch.randn(npos, d, generator=g) * 0.01).cuda()
    for rows in (1, 77, EMBED_GRID_ROWS + 77):
        tok = torch.randint(0, vocab, (rows,), generator=g, dtype=torch.int32)
        p = torch.randint(0, npos, (rows,), generator=g, dtype=torch.int32)  # not monotonic
        tok[0], tok[-1] = vocab - 1, 0
        if rows > 3:
            tok[1] = tok[2] = 0  # repeated ids
            p[1], p[2] = npos - 1, 0
        tok, p = tok.cuda(), p.cuda()
        out = torch.full((rows + 1, d), SENT, device="cuda")
        ok(lib, lib.mudpt_embed_tokens(P(table), vocab, P(tok), P(p), P(pos), P(out), rows, d, None))
        assert torch.equal(out[:rows], table[tok.long()] + pos[p.long()]), (d, rows)
        assert (out[rows] == SENT).all()


@pytest.mark.parametrize("e", [128, 512, 768])
def test_feature_ensemble_against_float64(e):
    """Every component within 4e-5: the worst-case fp32 error of a 1024-term sum of squares in any order is (n - 1) 2^-24 / 2 ~ 3e-5 relative,
    plus the T additions; a dropped template or a missing renormalisation is off by 1e-1."""
    lib = capi.load()
    g = torch.Generator().manual_seed(e)
    for Cn in (1, 5, 300):
        for T in (1, 2, 8):
            norms = 10.0 ** (torch.rand(T, Cn, 1, generator=g) * 6 - 3)  # row norms over 1e-3 .. 1e3
            f = torch.randn(T, Cn, e, generator=g)
            f = (f / f.norm(dim=-1, keepdim=True) * norms).cuda()
            runs = []
            for _ in range(2):
                acc = torch.full((Cn + 1, e), SENT, device="cuda")
                out = torch.full((Cn + 1, e), SENT, device="cuda")
                for t in range(T):
                    ok(lib, lib.mudpt_feature_ensemble(P(f[t]), P(acc), P(out), Cn, e, int(t == 0), int(t == T - 1), T, None))
                assert (out[Cn] == SENT).all() and (acc[Cn] == SENT).all()
                runs.append(out[:Cn].cpu())
            assert torch.equal(runs[0], runs[1])
            f64 = f.cpu().double()
            ref = (f64 / f64.norm(dim=-1, keepdim=True)).mean(dim=0)
            ref = ref / ref.norm(dim=-1, keepdim=True)
            err = (runs[0].double() - ref).abs().max().item()
            assert err <= 4e-5, (Cn, T, err)


@pytest.fixture
def zs_cfg(tmp_path, monkeypatch):
    from mudpt_amd import dassl_lite, tokenizer, trainer
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("MUDPT_BPE_VOCAB", R.merge_table_file(tmp_path))
    monkeypatch.setattr(tokenizer, "_default", None)
    monkeypatch.setattr(trainer, "_warned_fp16_scale", False)
    cfg = dassl_lite.default_cfg()
    cfg.DATASET.NAME = "Caltech101"
    cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 4, 6
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 2, 4
    cfg.MODEL.BACKBONE.SYNTHETIC_SEED = 3
    return cfg


def test_plugins_end_to_end(zs_cfg):
    from mudpt_amd import dassl_lite, lpclip, synth, zsclip
    from mudpt_amd.model import ModelShape
    from mudpt_amd.trainer import tokenize_prompts
    cfg = zs_cfg
    cfg.TRAINER.NAME = "ZeroshotCLIP"
    t = dassl_lite.build_trainer(cfg)
    assert type(t) is zsclip.ZeroshotCLIP and t.get_model_names() == [] and not hasattr(t, "optim")
    assert t.templates == ["a photo of a {}."] and t.model.n_templates == 1 and t.model.max_batch == 4 and t.model.dtype_name == "fp16"
    acc = t.test()
    assert 0.0 <= acc <= 100.0
    img = t.test_loader[0]["img"]
    logits = t.model_inference(img.cuda())
    assert tuple(logits.shape) == (4, 11) and torch.isfinite(logits).all()
    # a FrozenCLIP built directly from the same pieces: bit for bit
    state = synth.random_clip_state(ModelShape(), 3)
    names = t.dm.dataset.classnames
    tok = tokenize_prompts(zsclip.prompt_strings(zsclip.CUSTOM_TEMPLATES["Caltech101"], names), 77)[None]
    direct = zsclip.FrozenCLIP(ModelShape(), state, tok, max_batch=4, dtype="fp16")
    assert torch.equal(direct(img), logits)
    direct.close()
    # the linear-probe extractor over the test loader: encode_image batch by batch
    feats, labels = lpclip.extract_features(t.model, t.test_loader)
    n = sum(b["label"].numel() for b in t.test_loader)
    assert tuple(feats.shape) == (n, 512) and feats.dtype == torch.float32 and labels.dtype == torch.int64
    assert torch.equal(labels, torch.cat([b["label"] for b in t.test_loader]))
    assert torch.equal(feats, torch.cat([t.model.encode_image(b["img"]).cpu() for b in t.test_loader]))
    t.model.close()
    # the ensemble: 8 templates, other features, other logits
    cfg.TRAINER.NAME = "ZeroshotCLIP2"
    t2 = dassl_lite.build_trainer(cfg)
    assert type(t2) is zsclip.ZeroshotCLIP2 and len(t2.templates) == 8 and t2.model.n_templates == 8
    logits2 = t2.model_inference(img.cuda())
    assert torch.isfinite(logits2).all() and not torch.equal(logits2, logits)
    assert 0.0 <= t2.test() <= 100.0
    t2.model.close()
    t3 = dassl_lite.build_trainer(cfg)  # a second build in one process: 8 again (the reference would ensemble 9)
    assert len(t3.templates) == 8
    t3.model.close()
