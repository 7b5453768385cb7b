"""UUMuDPT (trainers/uumudpt.py, clip/model.py:600-664) without a GPU: the test-local restatement against the fixtures of the reference's own
modules, the 40 trainables, the initialisation draws at their two seed points, the config defaults, the plugin through dassl_lite with a
stand-in model, and the C ABI's refusals (all before any GPU call), mudpt_linear_bwd's among them."""
import ctypes as C
import dataclasses

import pytest
import torch
from torch import nn

from oracle import mudpt_oracle as O
from tests import uumudpt_reference as R
from tests.test_plugins_cpu import SIGNATURE, files  # noqa: F401  (files: the tiny backbone file and the fixture merge table)


@pytest.fixture(scope="module", params=R.FIXTURES)
def case(request):
    return R.UumudptCase(request.param)


def test_fixture_recipe_and_trainables(case):
    img = case.images.double()
    assert abs(img.sum().item() - float(case.z["images_checksum"][0])) <= 1e-9 * img.abs().sum().item()
    assert len(case.keys) == 40 and set(case.grads) | set(case.grad_samples) == set(case.keys)
    assert not (set(case.grads) & set(case.grad_samples))
    assert case.sample_above == (R.SAMPLE_ABOVE if case.cfg.v_layers == 12 else R.TINY_SAMPLE_ABOVE)
    for k, shp in R.trainable_keys(case.cfg):
        assert tuple(case.params[k].shape) == shp
        if k in case.grads:
            assert case.grads[k].shape == case.params[k].shape and case.params[k].numel() <= case.sample_above
        else:
            rows, vals, rms = case.grad_samples[k]
            assert case.params[k].numel() > case.sample_above and vals.shape == (R.SAMPLE_ROWS, shp[1])
            assert rows == R.sample_rows(k, shp[0], case.seeds[1])
            assert rms > 0 or (case.cfg.depth == 1 and k.startswith(R.V))  # Gen2 idles at depth 1
    # non-degenerate on purpose: no gamma is 1, no beta or bias 0
    for k, v in case.params.items():
        if k.endswith(".weight") and "ln_" in k:
            assert (v - 1).abs().min().item() > 0 and (v - 1).abs().mean().item() > 0.05
        if k.endswith("bias"):
            assert v.abs().mean().item() > 0.01
    # CLIP.load_state_dict: the vision tower owns 20 of the 40, the frozen state dict has none of them (and nothing it does not know)
    assert sorted(case.missing_keys) == sorted("visual." + k[len("image_encoder."):] for k in case.keys if k.startswith(R.V))
    assert len(case.missing_keys) == 20


def test_restatement_reproduces_the_reference(case):
    """Logits, loss, tapped block inputs and every stored gradient to torch-CPU fp32 agreement (the bounds of tests/test_umudpt_cpu.py)."""
    taps = {}
    with torch.no_grad():
        logits = R.forward(case.cfg, case.frozen, case.params, case.class_embedding, case.eot, case.images, taps)
    assert (logits - case.logits).abs().max().item() <= 1e-4
    for key, (ref, rows) in case.taps.items():  # sampled block inputs, after the splice
        got = taps[key.replace(".", ".x_in.", 1)][:, rows]
        assert (got - ref).abs().max().item() <= 1e-4 * (1 + ref.abs().max().item()), key
    if case.name == "uumudpt_vitb16_b2":
        assert set(case.taps) == {"vis.1", "vis.7", "txt.1"}
    loss, _, grads, dG, dT = R.forward_backward(case.cfg, case.frozen, case.params, case.class_embedding, case.eot, case.images, case.labels)
    assert abs(loss.item() - case.loss) <= 1e-5
    c = case.cfg
    for k in case.keys:
        if case.params[k].numel() == 0:  # deep_prompts / visual_ctx_deep_prompts at depth 1
            assert grads[k].shape == case.grads[k].shape
            continue
        if k in case.grads:
            ref, got = case.grads[k], grads[k]
        else:
            rows, ref, rms = case.grad_samples[k]
            got = grads[k][rows]
            assert abs(grads[k].double().pow(2).mean().sqrt().item() - rms) <= 1e-4 * rms, k
        assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-9, k
    # rows of layers the 3-layer towers never reach get no gradient, in either direction
    used_v, used_t = 1 + min(c.v_layers - 1, c.depth - 1), min(c.t_layers - 1, c.depth - 1)
    assert dG.shape == (c.depth, c.n_ctx, c.v_width) and dT.shape == (c.depth - 1, c.n_ctx, c.embed_dim)
    assert dG[:used_v].abs().min(dim=-1).values.max().item() > 0 and (dG[used_v:] == 0).all()
    assert (dT[used_t:] == 0).all() and (used_t == 0 or dT[:used_t].abs().min(dim=-1).values.max().item() > 0)
    # both sums are plain additions: dG is the vision tower's whole gradient of visual_ctx, and of the deep prompts up to Gen2's dX
    assert torch.equal(grads[R.VCTX], dG[0])
    if c.depth == 1:  # Gen2 saw zero rows: its 18 gradients are exactly zero, visual_ctx and Gen1 still train
        assert all((grads[k] == 0).all() for k, _ in R.generator_keys(R.GEN2, c.v_width, c.embed_dim))
        assert grads[R.VCTX].abs().sum() > 0 and all(grads[k].abs().sum() > 0 for k, _ in R.generator_keys(R.GEN1, c.t_width, c.v_width))
    else:
        _, dX2, g2 = R.generator_backward(case.params, R.GEN2, case.params[R.VDEEP], dT, torch.float32)
        assert (grads[R.VDEEP] - (dG[1:] + dX2)).abs().max().item() <= 1e-6 * grads[R.VDEEP].abs().max().item()
        assert all((grads[k] - g).abs().max().item() <= 1e-5 * grads[k].abs().max().item() + 1e-12 for k, g in g2.items())


def test_generators_are_the_umudpt_restatement():
    """Gen1 under the new prefix is tests.umudpt_reference.generator on the same values; Gen2 is that function at width d_v: cross-checked
    against the oracle's own pre-LN block with the two LayerNorms and the Linear around it."""
    from tests import umudpt_reference as U
    cfg = dataclasses.replace(O.TINY, n_ctx=3, depth=4)
    p = R.seeded_params(cfg, 5)
    up = {U.P + k[len(R.P):]: v for k, v in p.items() if k.startswith(R.P)}
    assert len(up) == 20 and torch.equal(R.generator(p, R.GEN1, R.prompt_tables(p)), U.generator(up, U.prompt_tables(up)))
    X = p[R.VDEEP]
    pre, attn, post, proj = R.GEN2
    sd = {k.replace(attn + ".", "b."): v for k, v in p.items() if k.startswith(attn + ".")}
    x = O.layer_norm(X, p[pre + ".weight"], p[pre + ".bias"])
    x = O.block(x, sd, "b.", cfg.v_width // 64, None)
    ref = O.layer_norm(x, p[post + ".weight"], p[post + ".bias"]) @ p[proj + ".weight"].t() + p[proj + ".bias"]
    T = R.generator(p, R.GEN2, X)
    assert T.shape == (3, 3, cfg.embed_dim) and (T - ref).abs().max().item() <= 1e-6
    T64, dX, g = R.generator_backward(p, R.GEN2, X, torch.ones(3, 3, cfg.embed_dim))
    assert T64.dtype == torch.float64 and dX.shape == X.shape and list(g) == [k for k, _ in R.generator_keys(R.GEN2, cfg.v_width, cfg.embed_dim)]
    assert all(v.abs().sum() > 0 for v in g.values())


def test_trainable_keys_are_the_references_forty():
    cfg = dataclasses.replace(O.VIT_B16, n_ctx=2, depth=8)  # train.py:129-133 defaults
    keys = R.trainable_keys(cfg)
    names = [k for k, _ in keys]
    assert len(keys) == 40 and len(set(names)) == 40
    assert all(k.startswith("uumudpt_prompt_learner.") for k in names[:20]) and all(k.startswith("image_encoder.visual_ctx") for k in names[20:])
    shapes = dict(keys)
    assert shapes[R.CTX] == (2, 512) and shapes[R.DEEP] == (7, 2, 512) and shapes[R.VCTX] == (2, 768) and shapes[R.VDEEP] == (7, 2, 768)
    assert shapes[R.P + "self_attn.attn.in_proj_weight"] == (1536, 512) and shapes[R.P + "visual_proj.weight"] == (768, 512)
    assert shapes[R.V + "_self_attn.attn.in_proj_weight"] == (2304, 768) and shapes[R.V + "_self_attn.mlp.c_fc.weight"] == (3072, 768)
    assert shapes[R.V + "_self_attn.mlp.c_proj.weight"] == (768, 3072) and shapes[R.V + "_text_proj.weight"] == (512, 768)
    assert names[20:26] == [R.V, R.V + "_deep_prompts", R.V + "_ln_intra_pre.weight", R.V + "_ln_intra_pre.bias",
                            R.V + "_self_attn.attn.in_proj_weight", R.V + "_self_attn.attn.in_proj_bias"]
    assert names[-4:] == [R.V + "_ln_intra_post.weight", R.V + "_ln_intra_post.bias", R.V + "_text_proj.weight", R.V + "_text_proj.bias"]
    # the first 20 are UMuDPT's under the new prefix, in UMuDPT's order
    from tests import umudpt_reference as U
    assert [(R.P + k[len(U.P):], s) for k, s in U.trainable_keys(cfg)] == keys[:20]
    d1 = dict(R.trainable_keys(dataclasses.replace(cfg, depth=1)))
    assert d1[R.DEEP] == (0, 2, 512) and d1[R.VDEEP] == (0, 2, 768)  # listed though empty: a checkpoint carries them


def test_init_draws_equal_the_references(case):
    """mudpt_amd.model.uumudpt_init_tensors(seed = seeds[1]) reproduces the sum and abs-sum of every tensor of the reference's own freshly
    constructed modules: the vision tower's 20 drawn behind torch.manual_seed(seed) as ``CLIP(...)`` draws them, the prompt learner's 20
    behind a second torch.manual_seed(seed) as ``CustomCLIP(...)`` does (recorded by tests/golden/gen_golden_uumudpt.py)."""
    from mudpt_amd.model import uumudpt_init_tensors
    c = case.cfg
    with torch.random.fork_rng(devices=[]):
        init = uumudpt_init_tensors(c.n_ctx, c.depth, c.t_width, c.v_width, c.embed_dim, c.image_size, c.patch, case.seeds[1], case.ctx_init)
    assert list(init) == case.keys
    for k, v in init.items():
        got = [v.double().sum().item(), v.double().abs().sum().item()]
        assert tuple(v.shape) == dict(R.trainable_keys(c))[k]
        assert got == pytest.approx(case.init_checksums[k], rel=1e-12, abs=1e-12), k
    assert torch.equal(init[R.CTX], case.ctx_init)
    # without a seed both halves continue the caller's stream, the vision half first
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(case.seeds[1])
        stream = uumudpt_init_tensors(c.n_ctx, c.depth, c.t_width, c.v_width, c.embed_dim, c.image_size, c.patch)
    assert torch.equal(stream[R.VCTX], init[R.VCTX]) and torch.equal(stream[R.V + "_text_proj.bias"], init[R.V + "_text_proj.bias"])
    assert not torch.equal(stream[R.CTX], init[R.CTX])


def test_default_cfg_and_registry():
    from mudpt_amd import capi, dassl_lite, trainer, uumudpt
    node = dassl_lite.default_cfg().TRAINER.UUMUDPT  # train.py:129-133
    assert (node.N_CTX, node.CTX_INIT, node.DEEP_PROMPT_DEPTH, node.PREC) == (2, "a photo of a", 8, "fp16")
    assert trainer.TRAINER_REGISTRY.get("UUMuDPT") is uumudpt.UUMuDPT and issubclass(uumudpt.UUMuDPT, trainer.PromptTrainer)
    assert (uumudpt.UUMuDPT.CFG_NODE, uumudpt.UUMuDPT.MODEL_NAME) == ("UUMUDPT", "UnifiedMultimodalDeepPromptTuning")  # uumudpt.py:276
    assert capi.VARIANT_UUMUDPT == 7 and capi.ABI_VERSION == 7


class _StandIn(nn.Module):
    """CustomCLIP needs an MI355X: this keeps the arguments the plugin gave and owns the 40 reference keys plus nothing else."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        bound = SIGNATURE.bind(self, *args, **kwargs)
        bound.apply_defaults()
        self.args = {k: v for k, v in bound.arguments.items() if k != "self"}
        s = self.args["shape"]
        cfg = dataclasses.replace(O.TINY, n_ctx=s.n_ctx, depth=s.depth, t_width=s.t_width, v_width=s.v_width, embed_dim=s.embed_dim)
        self.param_names = []
        for k, shp in R.trainable_keys(cfg):
            mod = self
            *path, leaf = k.split(".")
            for part in path:
                if not hasattr(mod, part):
                    setattr(mod, part, nn.Module())
                mod = getattr(mod, part)
            mod.register_parameter(leaf, nn.Parameter(torch.zeros(shp)))
            self.param_names.append(k)
        self.flat_params = torch.zeros(4)
        self.class_shard = None


def test_plugin_builds_optimises_and_loads_the_forty(monkeypatch, capsys, files, tmp_path):  # noqa: F811
    from mudpt_amd import dassl_lite, tokenizer, trainer, uumudpt  # noqa: F401
    monkeypatch.setattr(trainer, "CustomCLIP", _StandIn)
    loads = []
    monkeypatch.setattr(trainer, "load_pretrained_weights", lambda m, path: loads.append((m, path)))
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_CLASS_PARALLEL"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("MUDPT_BPE_VOCAB", files["vocab"])
    monkeypatch.setattr(tokenizer, "_default", None)
    cfg = dassl_lite.default_cfg()
    cfg.TRAINER.NAME = "UUMuDPT"
    cfg.TRAINER.UUMUDPT.DEEP_PROMPT_DEPTH = 3
    cfg.INPUT.SIZE = (32, 32)
    cfg.MODEL.BACKBONE.PATH = files["tiny"]
    cfg.MODEL.INIT_WEIGHTS = "init.pth.tar"
    t = dassl_lite.build_trainer(cfg)
    out = capsys.readouterr().out
    assert 'Initial context: "a photo"' in out and "Number of context words (tokens): 2" in out and "Depth of deep prompt: 3" in out
    a = t.model.args
    assert (a["variant"], a["shape"].n_ctx, a["shape"].depth, a["ctx_token_ids"], a["dtype"]) == ("uumudpt", 2, 3, [320, 1125], "fp16")
    assert t.get_model_names() == ["UnifiedMultimodalDeepPromptTuning"] and t._models["UnifiedMultimodalDeepPromptTuning"] is t.model
    keys = [k for k, _ in R.trainable_keys(dataclasses.replace(O.TINY, n_ctx=2, depth=3))]
    assert list(t.model.state_dict()) == keys and len(keys) == 40
    held = {id(p) for g in t.optim.param_groups for p in g["params"]}
    assert {n for n, p in t.model.named_parameters() if id(p) in held} == set(keys) and len(held) == 40
    assert loads == [(t.model, "init.pth.tar")]  # MODEL.INIT_WEIGHTS goes to the module that owns the tensors
    # load_model: the fixed token buffers of a reference checkpoint are dropped, the rest loads with strict=False (uumudpt.py:342-352)
    sd = {k: torch.full_like(v, 0.5) for k, v in t.model.state_dict().items()}
    sd[R.P + "token_prefix"], sd[R.P + "token_suffix"] = torch.ones(5, 1, 128), torch.ones(5, 74, 128)
    sd["image_encoder.conv1.weight"] = torch.ones(3)  # a frozen backbone entry of a reference checkpoint
    d = tmp_path / "UnifiedMultimodalDeepPromptTuning"
    d.mkdir()
    torch.save({"state_dict": sd, "epoch": 4}, d / "model.pth.tar-4")
    t.load_model(str(tmp_path), epoch=4)
    assert all(torch.equal(v, torch.full_like(v, 0.5)) for v in t.model.state_dict().values())
    cfg.TRAINER.UUMUDPT.DEEP_PROMPT_DEPTH = 0
    with pytest.raises(AssertionError, match="PROMPT_DEPTH should be > 0"):
        dassl_lite.build_trainer(cfg)


def _cfg(capi, n_ctx, depth, t_width=128, t_heads=2, embed_dim=None, v_width=192, v_heads=3):
    return capi.Config(32, 16, v_width, 3, v_heads, t_width, 3, t_heads, 77, t_width if embed_dim is None else embed_dim, n_ctx, depth, 5, 4, capi.BF16,
                       capi.VARIANT_UUMUDPT)


def test_create_refusals_come_before_any_gpu_call():
    """Every refusal is an argument check (without a GPU a call that got past the checks fails with MUDPT_ERR_HIP instead)."""
    from mudpt_amd import capi
    lib = capi.load()
    h = C.c_void_p()
    assert capi.VARIANT_UUMUDPT == 7
    assert lib.mudpt_create(C.byref(_cfg(capi, 2, 0)), C.byref(h)) == 1 and b"PROMPT_DEPTH should be > 0" in lib.mudpt_last_error()
    assert lib.mudpt_create(C.byref(_cfg(capi, 17, 3)), C.byref(h)) == 1 and b"n_ctx 17" in lib.mudpt_last_error()
    assert lib.mudpt_create(C.byref(_cfg(capi, 2, 3, embed_dim=64)), C.byref(h)) == 1 and b"uumudpt.py:224" in lib.mudpt_last_error()
    # v_width % 64 != 0 (Gen2 has heads of 64): every such width already fails the towers' own "head dim must be 64" check, which comes first;
    # Gen2's pg_check_shape at (depth - 1, n_ctx, v_width, embed_dim) asks nothing the tower checks and Gen1's n_ctx limit do not ask already
    for heads in (2, 3):
        assert lib.mudpt_create(C.byref(_cfg(capi, 2, 3, v_width=160, v_heads=heads)), C.byref(h)) == 1 and b"head dim must be 64" in lib.mudpt_last_error()
    assert lib.mudpt_create(C.byref(_cfg(capi, 17, 1)), C.byref(h)) == 1 and b"n_ctx 17" in lib.mudpt_last_error()  # depth 1: Gen2 idle, Gen1's limit holds
    assert lib.mudpt_create(C.byref(_cfg(capi, 0, 3)), C.byref(h)) == 1
    assert lib.mudpt_create(C.byref(_cfg(capi, 2, 3, t_width=96, t_heads=1)), C.byref(h)) == 1
    ps = capi.PromptShape(2, 2, 2, 2)
    assert lib.mudpt_create_ex(C.byref(_cfg(capi, 2, 3)), C.byref(ps), C.byref(h)) == 1  # the prompt shape is for VPT / MPT only
    bad = _cfg(capi, 2, 3)
    bad.variant = 8
    assert lib.mudpt_create(C.byref(bad), C.byref(h)) == 1 and b"unknown variant 8" in lib.mudpt_last_error()
    if not torch.cuda.is_available():
        for n_ctx, depth in ((2, 3), (3, 1), (16, 5)):
            assert lib.mudpt_create(C.byref(_cfg(capi, n_ctx, depth)), C.byref(h)) == 2, (n_ctx, depth, lib.mudpt_last_error())


def test_linear_bwd_refuses_bad_arguments_on_the_host():
    from mudpt_amd import capi
    lib = capi.load()
    assert "mudpt_linear_bwd" in capi.declared_functions() and "mudpt_linear_bwd" in capi.SIGNATURES
    # addresses that are never dereferenced: every call below is refused on the host.  R = 4, out = 8, in = 16: dy 32, x 64, W / dW 128,
    # db 8, dx 64 floats; the six buffers below are 4 KiB apart
    dy, x, W, dW, db, dx = (C.c_void_p(0x10000 + 0x1000 * i) for i in range(6))
    call = lambda *a: lib.mudpt_linear_bwd(*a, None)  # noqa: E731
    for i in range(6):
        args = [dy, x, W, dW, db, dx]
        args[i] = None
        assert call(4, 8, 16, *args) == 1 and b"null" in lib.mudpt_last_error(), i
    for shape in ((0, 8, 16), (4, 0, 16), (4, 8, 0), (-1, 8, 16)):
        assert call(*shape, dy, x, W, dW, db, dx) == 1 and b"bad arguments" in lib.mudpt_last_error(), shape
    assert call(4, 8, 16, dy, x, W, W, db, dx) == 1 and b"dW aliases the input W" in lib.mudpt_last_error()
    assert call(4, 8, 16, dy, x, W, dW, db, x) == 1 and b"dx aliases the input x" in lib.mudpt_last_error()
    assert call(4, 8, 16, dy, x, W, dW, dy, dx) == 1 and b"db aliases the input dy" in lib.mudpt_last_error()
    assert call(4, 8, 16, dy, x, W, dW, C.c_void_p(dy.value + 4 * 31), dx) == 1  # the last element of dy
    assert call(4, 8, 16, dy, x, W, dW, C.c_void_p(dW.value + 4 * 127), dx) == 1 and b"dW aliases db" in lib.mudpt_last_error()
    assert call(4, 8, 16, dy, x, W, dW, db, C.c_void_p(dW.value - 4 * 63)) == 1  # dx's last element is dW's first
    if not torch.cuda.is_available():  # a call that passes every check reaches the launch
        assert call(4, 8, 16, dy, x, W, dW, db, C.c_void_p(dW.value - 4 * 64)) == 2
