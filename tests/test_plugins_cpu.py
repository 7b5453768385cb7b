"""What every trainer plugin's ``build_model`` and hooks do, pinned on CPU.

``CustomCLIP`` needs an MI355X, so each module that binds the name gets a recording stand-in: it keeps the arguments the plugin gave,
bound to the real signature (defaults applied, so how they were spelled does not matter), and holds one parameter in a
``prompt_learner`` sub-module and one outside it.  Everything else is the product: dassl_lite.build_trainer on a tiny CLIP file,
parallel.init at world 1, and install_loader (the DevicePrefetcher passes the loader through without a HIP device).

The expected values are literals, recorded from the plugins as they were before they shared a base class and checked by hand against
the reference plugins' build_model / load_model (trainers/mudpt.py:192 / :270, cocoop.py:206 / :290, coop.py:238 / :314, vpt.py:127 /
:203, mpt.py:182 / :261); the log lines are this package's own (their order differs from the reference's, which prints the prompt
settings inside CustomCLIP, after "Building custom CLIP").  Prompts with a prefix other than the benchmark's "a photo of a"
need a BPE merge table: the one of tests/golden/coop_name_merges.json holds the merges the class names use at their real ranks, so the
names (and "x") get CLIP's ids, while other words ("photo") split into byte-level pieces of this table."""
import dataclasses
import gzip
import inspect
import json
import math
import os

import pytest
import torch
from torch import nn

from mudpt_amd import cocoop, coop, dassl_lite, model, synth, tokenizer, trainer, vpt
from tests.test_checkpoint_cpu import TINY, as_checkpoint

HERE = os.path.dirname(os.path.abspath(__file__))
SIGNATURE = inspect.signature(model.CustomCLIP.__init__)
PLUGIN_MODULES = (trainer, cocoop, coop, vpt)


class RecordingCLIP(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        bound = SIGNATURE.bind(self, *args, **kwargs)
        bound.apply_defaults()
        self.args = {k: v for k, v in bound.arguments.items() if k != "self"}
        self.prompt_learner = nn.Module()
        self.prompt_learner.ctx = nn.Parameter(torch.zeros(2, 3))
        self.outer = nn.Parameter(torch.zeros(5))
        self.param_names = ["ctx"]  # one name: the printed set has one order
        self.flat_params = torch.zeros(11)
        self.class_shard = self.args["class_shard"]


# class names (tests/golden/coop_name_merges.json, synth.BENCH_CLASSNAMES) -> their CLIP token ids
NAME_IDS = [[1710], [15931], [33341], [48760], [16451], [13201], [773], [11703], [5992], [22874], [29172, 10940]]
A_PHOTO_OF_A = [320, 1125, 539, 320]  # synth.CTX_INIT_TOKENS, recorded from the reference tokenizer
# "photo" and "of" under the fixture table, which lacks their merges: p, ho, t, o</w> and o, f</w> (CLIP's table: 1125 and 539)
PHOTO, OF = [79, 606, 83, 334], [78, 325]
SOT, DOT, EOT, X = 49406, 269, 49407, 343


def prompts(prefix_ids):
    """clip.tokenize("<prefix> <name>.") of the 11 classes."""
    tok = torch.zeros(11, 77, dtype=torch.int32)
    for c, name in enumerate(NAME_IDS):
        ids = [SOT] + prefix_ids + name + [DOT, EOT]
        tok[c, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return tok


def shape(n_ctx, depth):
    return dataclasses.replace(TINY, n_ctx=n_ctx, depth=depth)


def args(**kw):
    """The CustomCLIP arguments besides clip_state / tokenized_prompts that every case shares, then the case's own."""
    out = dict(ctx_token_ids=None, max_batch=100, dtype="fp16", device="cuda:0", seed=1, variant="mudpt", knobs=None, class_shard=None,
               group=None, class_token_position="end", name_lens=None, prompt_shape=None)
    out.update(kw)
    return out


LOAD = ["Loading CLIP (backbone: ViT-B/16)", "Loading CLIP backbone: ViT-B/16 from <backbone>"]
FROZEN = "Turning off gradients in both the image and the text encoder"
UPDATED = "Parameters to be updated: {'ctx'}"
FP16_NOTE = ('NOTE: PREC "fp16" with exp(logit_scale) = 100.0: this mode rounds GEMM operands to fp16 and is ~4e-3 from the reference\'s '
             'fp32 logits at this scale (1e-3 is only held at the init scale 14.29).  PREC "fp32" selects the parity mode (<= 3.5e-4 at '
             'scale 100, ~1.2x the step time of "fp16"); "amp" is the bf16 throughput mode.')
COOP_NAME_LENS = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2]

# id: (trainer, cfg overrides, needs the merge table, backbone logit scale ln 100, expected)
CASES = {
    "mudpt_default": ("MuDPT", {}, True, False, dict(
        args=args(shape=shape(2, 8), ctx_token_ids=[320, 1125]),
        tokenized=prompts([320] + PHOTO), models={"MultimodalDeepPromptTuning": "model"}, optimized={"prompt_learner.ctx", "outer"},
        init="model",
        stdout=LOAD + ['Initial context: "a photo"', "Number of context words (tokens): 2", "Depth of deep prompt: 8", "Building custom CLIP",
                       UPDATED])),
    "mudpt_generic_fp32": ("MuDPT", {"TRAINER.MUDPT.CTX_INIT": "", "TRAINER.MUDPT.PREC": "fp32"}, True, False, dict(
        args=args(shape=shape(2, 8), dtype="fp32"),
        tokenized=prompts([X, X]), models={"MultimodalDeepPromptTuning": "model"}, optimized={"prompt_learner.ctx", "outer"},
        init="model",
        stdout=LOAD + ["Initializing A Generic Context", 'Initial context: "X X"', "Number of context words (tokens): 2",
                       "Depth of deep prompt: 8", "Building custom CLIP", UPDATED])),
    "cocoop_default": ("CoCoOp", {}, False, False, dict(
        args=args(shape=shape(4, 1), ctx_token_ids=A_PHOTO_OF_A, variant="cocoop"),
        tokenized=prompts(A_PHOTO_OF_A), models={"prompt_learner": "prompt_learner"}, optimized={"prompt_learner.ctx"},
        init="prompt_learner",
        stdout=LOAD + ['Initial context: "a photo of a"', "Number of context words (tokens): 4", "Building custom CLIP", FROZEN, UPDATED])),
    "cocoop_fp16_at_scale_100": ("CoCoOp", {}, False, True, dict(
        args=args(shape=shape(4, 1), ctx_token_ids=A_PHOTO_OF_A, variant="cocoop"),
        tokenized=prompts(A_PHOTO_OF_A), models={"prompt_learner": "prompt_learner"}, optimized={"prompt_learner.ctx"},
        init="prompt_learner",
        stdout=LOAD + [FP16_NOTE, 'Initial context: "a photo of a"', "Number of context words (tokens): 4", "Building custom CLIP", FROZEN,
                       UPDATED])),
    "coop_shared_end": ("CoOp", {}, True, False, dict(
        args=args(shape=shape(16, 1), variant="coop", name_lens=COOP_NAME_LENS),
        tokenized=prompts([X] * 16), models={"prompt_learner": "prompt_learner"}, optimized={"prompt_learner.ctx"},
        init="prompt_learner",
        stdout=LOAD + ["Initializing a generic context", 'Initial context: "' + " ".join(["X"] * 16) + '"',
                       "Number of context words (tokens): 16", "Building custom CLIP", FROZEN, UPDATED])),
    "coop_csc_middle_amp": ("CoOp", {"TRAINER.COOP.CSC": True, "TRAINER.COOP.CLASS_TOKEN_POSITION": "middle", "TRAINER.COOP.PREC": "amp"},
                            True, False, dict(
        args=args(shape=shape(16, 1), dtype="bf16", variant="coop_csc", class_token_position="middle", name_lens=COOP_NAME_LENS),
        tokenized=prompts([X] * 16), models={"prompt_learner": "prompt_learner"}, optimized={"prompt_learner.ctx"},
        init="prompt_learner",
        stdout=LOAD + ["Initializing class-specific contexts", 'Initial context: "' + " ".join(["X"] * 16) + '"',
                       "Number of context words (tokens): 16", "Building custom CLIP", FROZEN, UPDATED])),
    "coop_init_ignores_csc": ("CoOp", {"TRAINER.COOP.CTX_INIT": "a photo of a", "TRAINER.COOP.CSC": True}, True, False, dict(
        args=args(shape=shape(4, 1), ctx_token_ids=A_PHOTO_OF_A, variant="coop", name_lens=COOP_NAME_LENS),
        tokenized=prompts([320] + PHOTO + OF + [320]), models={"prompt_learner": "prompt_learner"}, optimized={"prompt_learner.ctx"},
        init="prompt_learner",
        stdout=LOAD + ['Initial context: "a photo of a"', "Number of context words (tokens): 4", "Building custom CLIP", FROZEN, UPDATED])),
    "vpt_yaml": ("VPT", {"TRAINER.VPT.PROMPTS": vpt.YAML_PROMPTS["VPT"]}, False, False, dict(
        args=args(shape=shape(4, 1), variant="vpt", prompt_shape=(0, 0, 8, 12)),
        tokenized=prompts(A_PHOTO_OF_A), models={"VisualPromptLearner": "model"}, optimized={"prompt_learner.ctx", "outer"},
        init="model",
        stdout=LOAD + ['Initial context: "a photo of a"', "Number of context words (tokens) of deep visual prompt: 8",
                       "Number of context words (tokens) of deep text prompt: 0", "Number of depth of deep visual prompt: 12",
                       "Number of depth of deep text prompt: 0", "Building custom CLIP", FROZEN, UPDATED])),
    "mpt_yaml": ("MPT", {"TRAINER.MPT.PROMPTS": vpt.YAML_PROMPTS["MPT"]}, False, False, dict(
        args=args(shape=shape(4, 1), ctx_token_ids=[320, 1125], variant="mpt", prompt_shape=(2, 12, 2, 12)),
        tokenized=prompts(A_PHOTO_OF_A), models={"MultiModalPromptLearner": "model"}, optimized={"prompt_learner.ctx", "outer"},
        init="model",
        stdout=LOAD + ['Initial context: "a photo of a"', "Number of context words (tokens) of deep visual prompt: 2",
                       "Number of context words (tokens) of deep text prompt: 2", "Number of depth of deep visual prompt: 12",
                       "Number of depth of deep text prompt: 12", "Building custom CLIP", FROZEN, UPDATED])),
    "mpt_generic": ("MPT", {"TRAINER.MPT.PROMPTS": vpt.YAML_PROMPTS["MPT"], "TRAINER.MPT.TEXT_CTX_INIT": ""}, True, False, dict(
        args=args(shape=shape(4, 1), variant="mpt", prompt_shape=(2, 12, 2, 12)),
        tokenized=prompts([X, X]), models={"MultiModalPromptLearner": "model"}, optimized={"prompt_learner.ctx", "outer"},
        init="model",
        stdout=LOAD + ["Initializing a generic context", 'Initial context: "X X"', "Number of context words (tokens) of deep visual prompt: 2",
                       "Number of context words (tokens) of deep text prompt: 2", "Number of depth of deep visual prompt: 12",
                       "Number of depth of deep text prompt: 12", "Building custom CLIP", FROZEN, UPDATED])),
}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The tiny backbone (logit scale of the random init, and ln 100 as released checkpoints) and the fixture merge table."""
    d = tmp_path_factory.mktemp("plugins")
    ck = as_checkpoint(synth.random_clip_state(TINY, seed=3))
    torch.save(ck, d / "tiny.pt")
    ck["logit_scale"] = torch.tensor(math.log(100.0))
    torch.save(ck, d / "tiny_scale100.pt")
    spec = json.load(open(os.path.join(HERE, "golden", "coop_name_merges.json"), encoding="utf-8"))
    (d / "vocab").mkdir()
    vocab = d / "vocab" / "bpe_simple_vocab_16e6.txt.gz"
    with gzip.open(vocab, "wt", encoding="utf-8") as f:
        f.write("\n".join(["#version: 0.2"] + [spec["merges"].get(str(r), f"一{r} 丁") for r in range(spec["n_merges"])]) + "\n")
    return {"tiny": str(d / "tiny.pt"), "scale100": str(d / "tiny_scale100.pt"), "vocab": str(vocab)}


def build(monkeypatch, capsys, files, case, init_weights=""):
    """build_trainer(cfg) with the recording CustomCLIP; returns the trainer, the stdout lines and the INIT_WEIGHTS loads."""
    name, overrides, needs_vocab, scale100, _ = CASES[case]
    for mod in PLUGIN_MODULES:
        if hasattr(mod, "CustomCLIP"):
            monkeypatch.setattr(mod, "CustomCLIP", RecordingCLIP)
    loads = []
    for mod in PLUGIN_MODULES:
        if hasattr(mod, "load_pretrained_weights"):
            monkeypatch.setattr(mod, "load_pretrained_weights", lambda m, path: loads.append((m, path)))
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_CLASS_PARALLEL"):
        monkeypatch.delenv(var, raising=False)
    if needs_vocab:
        monkeypatch.setenv("MUDPT_BPE_VOCAB", files["vocab"])
    else:
        monkeypatch.delenv("MUDPT_BPE_VOCAB", raising=False)
    monkeypatch.setattr(tokenizer, "_default", None)  # the tokenizer of an earlier test's merge table
    monkeypatch.setattr(trainer, "_warned_fp16_scale", False)
    cfg = dassl_lite.default_cfg()
    cfg.TRAINER.NAME = name
    cfg.INPUT.SIZE = (32, 32)
    cfg.MODEL.BACKBONE.PATH = files["scale100" if scale100 else "tiny"]
    cfg.MODEL.INIT_WEIGHTS = init_weights
    for key, value in overrides.items():
        *path, leaf = key.split(".")
        node = cfg
        for part in path:
            node = node[part]
        if leaf == "PROMPTS":
            node.DEEP_TEXT_N_CTX, node.TEXT_PROMPT_DEPTH, node.DEEP_VISUAL_N_CTX, node.VISUAL_PROMPT_DEPTH = value
        else:
            node[leaf] = value
    capsys.readouterr()
    t = dassl_lite.build_trainer(cfg)
    out = capsys.readouterr().out.replace(cfg.MODEL.BACKBONE.PATH, "<backbone>")
    return t, out.splitlines(), loads


def role(t, module):
    return {id(t.model): "model", id(t.model.prompt_learner): "prompt_learner"}.get(id(module), repr(module))


@pytest.mark.parametrize("case", list(CASES))
def test_build_model(monkeypatch, capsys, files, case):
    want = CASES[case][-1]
    t, out, loads = build(monkeypatch, capsys, files, case)
    assert isinstance(t.model, RecordingCLIP)
    got = dict(t.model.args)
    state, tokenized = got.pop("clip_state"), got.pop("tokenized_prompts")
    assert got == want["args"]
    assert torch.equal(tokenized, want["tokenized"]), tokenized[:, :24]
    assert float(state["logit_scale"].exp()) == pytest.approx(100.0 if CASES[case][3] else 1 / 0.07)
    assert "token_embedding.weight" in state and state["visual.conv1.weight"].shape[-1] == TINY.patch
    assert t.get_model_names() == list(want["models"])
    assert {n: role(t, t._models[n]) for n in t.get_model_names()} == want["models"]
    held = {id(p) for g in t.optim.param_groups for p in g["params"]}
    assert {n for n, p in t.model.named_parameters() if id(p) in held} == want["optimized"] and len(held) == len(want["optimized"])
    assert t.scaler is None and not loads
    assert out == want["stdout"]
    assert out.count(FP16_NOTE) == int(CASES[case][3])
    # MODEL.INIT_WEIGHTS: loaded into the module that owns the trainables; nothing else changes
    t, out, loads = build(monkeypatch, capsys, files, case, init_weights="init.pth.tar")
    assert [(role(t, m), p) for m, p in loads] == [(want["init"], "init.pth.tar")]
    assert out == want["stdout"]


# trainer: (cfg node, registered model name, token buffers load_model drops, the skipped note, "acc" in the step's summary)
PLUGINS = {
    "MuDPT": ("MUDPT", "MultimodalDeepPromptTuning", ("mudpt_prompt_learner.token_prefix", "mudpt_prompt_learner.token_suffix"),
              "Note that load_model() is skipped as no pretrained model is given", False),
    "CoCoOp": ("COCOOP", "prompt_learner", ("token_prefix", "token_suffix"),
               "Note that load_model() is skipped as no Pretrained model is given", False),
    "CoOp": ("COOP", "prompt_learner", ("token_prefix", "token_suffix"),
             "Note that load_model() is skipped as no pretrained model is given", True),
    "VPT": ("VPT", "VisualPromptLearner", ("text_prompt_learner.token_prefix", "text_prompt_learner.token_suffix"),
            "Note that load_model() is skipped as no pretrained model is given", True),
    "MPT": ("MPT", "MultiModalPromptLearner", ("text_prompt_learner.token_prefix", "text_prompt_learner.token_suffix"),
            "Note that load_model() is skipped as no pretrained model is given", True),
}


class _StepModel(nn.Module):
    """The surface data_parallel_step uses: flat buckets, forward_backward (logits on request), invalidate_text_cache."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(2))
        self.flat_params, self.flat_grads = self.w.data, torch.zeros(2)
        self.w.grad = self.flat_grads

    def forward_backward(self, image, label, grad_scale=1.0, return_logits=False):
        self.flat_grads.fill_(1.0)
        loss = torch.tensor(0.5)
        return (loss, torch.eye(2)[label]) if return_logits else loss

    def invalidate_text_cache(self):
        pass


def _module_with(keys):
    root = nn.Module()
    for k in keys:
        mod = root
        *path, leaf = k.split(".")
        for part in path:
            if not hasattr(mod, part):
                setattr(mod, part, nn.Module())
            mod = getattr(mod, part)
        mod.register_parameter(leaf, nn.Parameter(torch.zeros(3)))
    return root


@pytest.mark.parametrize("name", list(PLUGINS))
def test_hooks(name, tmp_path, capsys):
    node, model_name, drop, note, with_acc = PLUGINS[name]
    cls = trainer.TRAINER_REGISTRY.get(name)  # train.py --trainer <name>
    assert cls.__name__ == name
    for hook in ("check_cfg", "build_model", "forward_backward", "parse_batch_train", "load_model", "model_inference"):
        assert callable(getattr(cls, hook))
    t = object.__new__(cls)
    cfg = dassl_lite.default_cfg()
    for other in PLUGINS.values():  # only the plugin's own node is checked
        if other[0] != node:
            cfg.TRAINER[other[0]].PREC = "int8"
    t.check_cfg(cfg)
    cfg.TRAINER[node].PREC = "int8"
    with pytest.raises(AssertionError):
        t.check_cfg(cfg)

    m = _module_with(("ctx",) + drop)
    t._models = {model_name: m}
    capsys.readouterr()
    assert t.load_model("") is None
    assert capsys.readouterr().out == note + "\n"
    with pytest.raises(FileNotFoundError):
        t.load_model(str(tmp_path / "missing"), epoch=3)
    (tmp_path / model_name).mkdir()
    path = tmp_path / model_name / "model.pth.tar-3"
    torch.save({"state_dict": {k: torch.ones(3) for k in ("ctx",) + drop}, "epoch": 3}, path)
    t.load_model(str(tmp_path), epoch=3)
    assert capsys.readouterr().out == f'Loading weights to {model_name} from "{path}" (epoch = 3)\n'
    assert torch.equal(m.ctx.detach(), torch.ones(3))
    assert all(torch.equal(p.detach(), torch.zeros(3)) for k, p in m.named_parameters() if k != "ctx")  # the fixed token buffers

    t.model = _StepModel()
    t.optim = torch.optim.SGD(t.model.parameters(), lr=0.1)
    t.device, t.batch_idx, t.num_batches = torch.device("cpu"), 0, 99
    summary = t.forward_backward({"img": torch.zeros(2, 3, 4, 4), "label": torch.tensor([0, 1])})
    assert summary == ({"loss": 0.5, "acc": 100.0} if with_acc else {"loss": 0.5})
    assert torch.allclose(t.model.w.detach(), torch.full((2,), 0.9))
