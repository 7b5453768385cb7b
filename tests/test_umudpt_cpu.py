"""UMuDPT (trainers/umudpt.py) without a GPU: the test-local restatement against the fixtures of the reference's own modules, the 20
trainables, the initialisation draws, the config defaults, the plugin through dassl_lite with a stand-in model, and the C ABI's refusals
(all before any GPU call)."""
import ctypes as C
import dataclasses

import pytest
import torch
from torch import nn

from oracle import mudpt_oracle as O
from tests import umudpt_reference as R
from tests.test_plugins_cpu import SIGNATURE, files  # noqa: F401  (files: the tiny backbone file and the fixture merge table)


@pytest.fixture(scope="module", params=R.FIXTURES)
def case(request):
    return R.UmudptCase(request.param)


def test_fixture_recipe_and_trainables(case):
    img = case.images.double()
    assert abs(img.sum().item() - float(case.z["images_checksum"][0])) <= 1e-9 * img.abs().sum().item()
    assert len(case.keys) == 20 and set(case.grads) | set(case.grad_samples) == set(case.keys)
    assert not (set(case.grads) & set(case.grad_samples))
    for k, shp in R.trainable_keys(case.cfg):
        assert tuple(case.params[k].shape) == shp
        if k in case.grads:
            assert case.grads[k].shape == case.params[k].shape
        else:
            rows, vals, rms = case.grad_samples[k]
            assert case.params[k].numel() > R.SAMPLE_ABOVE and vals.shape == (R.SAMPLE_ROWS, shp[1]) and rms > 0
            assert rows == R.sample_rows(k, shp[0], case.seeds[1])
    # non-degenerate on purpose: no gamma is 1, no beta or bias 0
    for k, v in case.params.items():
        if k.endswith(".weight") and "ln_" in k:
            assert (v - 1).abs().min().item() > 0 and (v - 1).abs().mean().item() > 0.05
        if k.endswith("bias"):
            assert v.abs().mean().item() > 0.01


def test_restatement_reproduces_the_reference(case):
    """Logits, loss, tapped block inputs and every stored gradient to torch-CPU fp32 agreement (the bounds of tests/test_vpt_cpu.py)."""
    taps = {}
    with torch.no_grad():
        logits = R.forward(case.cfg, case.frozen, case.params, case.class_embedding, case.eot, case.images, taps)
    assert (logits - case.logits).abs().max().item() <= 1e-4
    for key, (ref, rows) in case.taps.items():  # sampled block inputs, after the splice
        got = taps[key.replace(".", ".x_in.", 1)][:, rows]
        assert (got - ref).abs().max().item() <= 1e-4 * (1 + ref.abs().max().item()), key
    if case.name == "umudpt_vitb16_b2":
        assert set(case.taps) == {"vis.1", "vis.7", "txt.1"}
    loss, _, grads, dG = R.forward_backward(case.cfg, case.frozen, case.params, case.class_embedding, case.eot, case.images, case.labels)
    assert abs(loss.item() - case.loss) <= 1e-5
    for k in case.keys:
        if case.params[k].numel() == 0:  # deep_prompts at depth 1
            assert grads[k].shape == case.grads[k].shape
            continue
        if k in case.grads:
            ref, got = case.grads[k], grads[k]
        else:
            rows, ref, rms = case.grad_samples[k]
            got = grads[k][rows]
            assert abs(grads[k].double().pow(2).mean().sqrt().item() - rms) <= 1e-4 * rms, k
        assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-9, k
    # rows of layers the 3-layer towers never reach get no gradient from the vision tower
    used = 1 + min(case.cfg.v_layers - 1, case.cfg.depth - 1)
    assert dG.shape == (case.cfg.depth, case.cfg.n_ctx, case.cfg.v_width)
    assert dG[:used].abs().min(dim=-1).values.max().item() > 0 and (dG[used:] == 0).all()


def test_generator_matches_the_towers_own_block():
    """The restated block is the oracle's pre-LN block with ln_pre / ln_post / visual_proj around it: cross-checked against O.block."""
    cfg = dataclasses.replace(O.TINY, n_ctx=3, depth=4)
    p = R.seeded_params(cfg, 5)
    X = R.prompt_tables(p)
    sd = {k.replace(R.P + "self_attn.", "b."): v for k, v in p.items() if "self_attn" in k}
    x = O.layer_norm(X, p[R.P + "ln_pre.weight"], p[R.P + "ln_pre.bias"])
    x = O.block(x, sd, "b.", cfg.t_width // 64, None)
    ref = O.layer_norm(x, p[R.P + "ln_post.weight"], p[R.P + "ln_post.bias"]) @ p[R.P + "visual_proj.weight"].t() + p[R.P + "visual_proj.bias"]
    assert (R.generator(p, X) - ref).abs().max().item() <= 1e-6
    G64, dX, g = R.generator_backward(p, X, torch.ones(4, 3, cfg.v_width))
    assert G64.dtype == torch.float64 and dX.shape == X.shape and len(g) == 18 and all(v.abs().sum() > 0 for v in g.values())


def test_trainable_keys_are_the_references_twenty():
    cfg = dataclasses.replace(O.VIT_B16, n_ctx=2, depth=8)  # train.py:122-126 defaults
    keys = R.trainable_keys(cfg)
    assert len(keys) == 20 and all(k.startswith("umudpt_prompt_learner.") for k, _ in keys)
    shapes = dict(keys)
    assert shapes[R.CTX] == (2, 512) and shapes[R.DEEP] == (7, 2, 512)
    assert shapes[R.P + "self_attn.attn.in_proj_weight"] == (1536, 512) and shapes[R.P + "self_attn.mlp.c_fc.weight"] == (2048, 512)
    assert shapes[R.P + "self_attn.mlp.c_proj.weight"] == (512, 2048) and shapes[R.P + "visual_proj.weight"] == (768, 512)
    assert [k[len(R.P):] for k, _ in keys][:6] == ["ctx", "deep_prompts", "ln_pre.weight", "ln_pre.bias", "self_attn.attn.in_proj_weight",
                                                   "self_attn.attn.in_proj_bias"]
    assert [k[len(R.P):] for k, _ in keys][-4:] == ["ln_post.weight", "ln_post.bias", "visual_proj.weight", "visual_proj.bias"]
    total = sum(int(torch.tensor(s).prod()) for _, s in keys)
    assert total == 3556608  # 3.56 M parameters, 14 MB: three times MuDPT's bucket
    assert dict(R.trainable_keys(dataclasses.replace(cfg, depth=1)))[R.DEEP] == (0, 2, 512)  # listed though empty: a checkpoint carries it


def test_init_draws_equal_the_references(case):
    """mudpt_amd.model.umudpt_init_tensors under torch.manual_seed(seeds[1]) reproduces the sum and abs-sum of every tensor of the
    reference's own freshly constructed prompt learner (recorded by tests/golden/gen_golden_umudpt.py)."""
    from mudpt_amd.model import umudpt_init_tensors
    c = case.cfg
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(case.seeds[1])
        init = umudpt_init_tensors(c.n_ctx, c.depth, c.t_width, c.v_width, case.ctx_init)
    assert [R.P + k for k in init] == case.keys
    for k, v in init.items():
        want = case.init_checksums[R.P + k]
        got = [v.double().sum().item(), v.double().abs().sum().item()]
        assert tuple(v.shape) == dict(R.trainable_keys(c))[R.P + k]
        assert got == pytest.approx(want, rel=1e-12, abs=1e-12), k
    assert torch.equal(init["ctx"], case.ctx_init)
    # without CTX_INIT the context is the first draw (umudpt.py:104-108)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        generic = umudpt_init_tensors(c.n_ctx, c.depth, c.t_width, c.v_width)
        torch.manual_seed(7)
        first = torch.empty(c.n_ctx, c.t_width)
        nn.init.normal_(first, std=0.02)
    assert torch.equal(generic["ctx"], first)


def test_default_cfg_and_registry():
    from mudpt_amd import dassl_lite, trainer, umudpt
    node = dassl_lite.default_cfg().TRAINER.UMUDPT  # train.py:122-126
    assert (node.N_CTX, node.CTX_INIT, node.DEEP_PROMPT_DEPTH, node.PREC) == (2, "a photo of a", 8, "fp16")
    assert trainer.TRAINER_REGISTRY.get("UMuDPT") is umudpt.UMuDPT
    assert (umudpt.UMuDPT.CFG_NODE, umudpt.UMuDPT.MODEL_NAME) == ("UMUDPT", "UnifiedMultimodalDeepPromptTuning")  # umudpt.py:270


class _StandIn(nn.Module):
    """CustomCLIP needs an MI355X: this keeps the arguments the plugin gave and owns the 20 reference keys plus nothing else."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        bound = SIGNATURE.bind(self, *args, **kwargs)
        bound.apply_defaults()
        self.args = {k: v for k, v in bound.arguments.items() if k != "self"}
        s = self.args["shape"]
        cfg = dataclasses.replace(O.TINY, n_ctx=s.n_ctx, depth=s.depth, t_width=s.t_width, v_width=s.v_width)
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


def test_plugin_builds_optimises_and_loads_the_twenty(monkeypatch, capsys, files, tmp_path):  # noqa: F811
    from mudpt_amd import dassl_lite, tokenizer, trainer, umudpt  # noqa: F401
    monkeypatch.setattr(trainer, "CustomCLIP", _StandIn)
    loads = []
    monkeypatch.setattr(trainer, "load_pretrained_weights", lambda m, path: loads.append((m, path)))
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_CLASS_PARALLEL"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("MUDPT_BPE_VOCAB", files["vocab"])
    monkeypatch.setattr(tokenizer, "_default", None)
    cfg = dassl_lite.default_cfg()
    cfg.TRAINER.NAME = "UMuDPT"
    cfg.TRAINER.UMUDPT.DEEP_PROMPT_DEPTH = 3
    cfg.INPUT.SIZE = (32, 32)
    cfg.MODEL.BACKBONE.PATH = files["tiny"]
    cfg.MODEL.INIT_WEIGHTS = "init.pth.tar"
    t = dassl_lite.build_trainer(cfg)
    out = capsys.readouterr().out
    assert 'Initial context: "a photo"' in out and "Number of context words (tokens): 2" in out and "Depth of deep prompt: 3" in out
    a = t.model.args
    assert (a["variant"], a["shape"].n_ctx, a["shape"].depth, a["ctx_token_ids"], a["dtype"]) == ("umudpt", 2, 3, [320, 1125], "fp16")
    assert t.get_model_names() == ["UnifiedMultimodalDeepPromptTuning"] and t._models["UnifiedMultimodalDeepPromptTuning"] is t.model
    keys = [k for k, _ in R.trainable_keys(dataclasses.replace(O.TINY, n_ctx=2, depth=3))]
    assert list(t.model.state_dict()) == keys and len(keys) == 20
    held = {id(p) for g in t.optim.param_groups for p in g["params"]}
    assert {n for n, p in t.model.named_parameters() if id(p) in held} == set(keys) and len(held) == 20
    assert loads == [(t.model, "init.pth.tar")]  # MODEL.INIT_WEIGHTS goes to the module that owns the prompt learner's tensors
    # load_model: the fixed token buffers of a reference checkpoint are dropped, the rest loads with strict=False (umudpt.py:336-346)
    sd = {k: torch.full_like(v, 0.5) for k, v in t.model.state_dict().items()}
    sd[R.P + "token_prefix"], sd[R.P + "token_suffix"] = torch.ones(5, 1, 128), torch.ones(5, 74, 128)
    sd["image_encoder.conv1.weight"] = torch.ones(3)  # a frozen backbone entry of a reference checkpoint
    d = tmp_path / "UnifiedMultimodalDeepPromptTuning"
    d.mkdir()
    torch.save({"state_dict": sd, "epoch": 4}, d / "model.pth.tar-4")
    t.load_model(str(tmp_path), epoch=4)
    assert all(torch.equal(v, torch.full_like(v, 0.5)) for v in t.model.state_dict().values())
    cfg.TRAINER.UMUDPT.DEEP_PROMPT_DEPTH = 0
    with pytest.raises(AssertionError, match="PROMPT_DEPTH should be > 0"):
        dassl_lite.build_trainer(cfg)


def _cfg(capi, n_ctx, depth, t_width=128, t_heads=2):
    return capi.Config(32, 16, 192, 3, 3, t_width, 3, t_heads, 77, t_width, n_ctx, depth, 5, 4, capi.BF16, capi.VARIANT_UMUDPT)


def test_create_refusals_come_before_any_gpu_call():
    """Every refusal is an argument check (this box has no GPU: a call that got past the checks fails with MUDPT_ERR_HIP instead)."""
    from mudpt_amd import capi
    lib = capi.load()
    h = C.c_void_p()
    assert capi.VARIANT_UMUDPT == 6
    assert lib.mudpt_create(C.byref(_cfg(capi, 2, 0)), C.byref(h)) == 1 and b"PROMPT_DEPTH should be > 0" in lib.mudpt_last_error()
    assert lib.mudpt_create(C.byref(_cfg(capi, 17, 3)), C.byref(h)) == 1 and b"n_ctx 17" in lib.mudpt_last_error()
    assert lib.mudpt_create(C.byref(_cfg(capi, 0, 3)), C.byref(h)) == 1
    assert lib.mudpt_create(C.byref(_cfg(capi, 2, 3, t_width=96, t_heads=1)), C.byref(h)) == 1
    ps = capi.PromptShape(2, 2, 2, 2)
    assert lib.mudpt_create_ex(C.byref(_cfg(capi, 2, 3)), C.byref(ps), C.byref(h)) == 1  # the prompt shape is for VPT / MPT only
    if not torch.cuda.is_available():
        for n_ctx, depth in ((2, 3), (3, 1), (16, 5)):
            assert lib.mudpt_create(C.byref(_cfg(capi, n_ctx, depth)), C.byref(h)) == 2, (n_ctx, depth, lib.mudpt_last_error())


def test_promptgen_exports_refuse_bad_shapes_on_the_host():
    from mudpt_amd import capi
    lib = capi.load()
    for name in ("mudpt_layernorm_bwd_affine", "mudpt_pg_attention_fwd", "mudpt_pg_attention_bwd", "mudpt_quickgelu_fwd", "mudpt_quickgelu_bwd",
                 "mudpt_promptgen_forward", "mudpt_promptgen_backward", "mudpt_promptgen_workspace", "mudpt_promptgen_param_numel"):
        assert name in capi.declared_functions() and name in capi.SIGNATURES
    assert lib.mudpt_promptgen_param_numel(512, 768) == 3556608 - 8 * 2 * 512
    assert lib.mudpt_promptgen_workspace(8, 2, 512, 768) > 0 and lib.mudpt_promptgen_workspace(8, 17, 512, 768) == 0
    one = C.c_void_p(16)  # never dereferenced: every call below is refused on the host
    assert lib.mudpt_promptgen_forward(0, 2, 128, 192, one, one, one, one, 1 << 30, None) == 1 and b"PROMPT_DEPTH" in lib.mudpt_last_error()
    assert lib.mudpt_promptgen_forward(3, 17, 128, 192, one, one, one, one, 1 << 30, None) == 1 and b"n_ctx 17" in lib.mudpt_last_error()
    assert lib.mudpt_promptgen_forward(3, 2, 96, 192, one, one, one, one, 1 << 30, None) == 1 and b"multiple of 64" in lib.mudpt_last_error()
    assert lib.mudpt_promptgen_forward(3, 2, 128, 192, one, one, one, one, 8, None) == 1 and b"workspace" in lib.mudpt_last_error()
    assert lib.mudpt_promptgen_backward(3, 2, 128, 192, one, one, one, one, one, None, 1 << 30, None) == 1
    assert lib.mudpt_pg_attention_fwd(one, one, one, 2, 17, 2, 128, None) == 1 and b"L=17" in lib.mudpt_last_error()
    assert lib.mudpt_pg_attention_fwd(one, one, one, 2, 4, 0, 0, None) == 1
    assert lib.mudpt_pg_attention_bwd(one, one, None, one, 2, 4, 2, 128, None) == 1 and b"null" in lib.mudpt_last_error()
    assert lib.mudpt_pg_attention_bwd(one, one, one, one, 2, 4, 2, 100, None) == 1
