"""GPU tests of the test pass from cached image features: ``mudpt_forward_features`` / ``mudpt_image_features`` through the C ABI on the tiny
fixtures of every variant, and the trainers' opt-in (MUDPT_TEST_FEATURES / trainer.test_features) through dassl_lite."""
import ctypes as C

import numpy as np
import pytest
import torch

from mudpt_amd import capi
from tests import coop_reference as CR
from tests import zsclip_reference as ZR
from tests.helpers import GoldenCase, P, check_logits
from tests.test_cocoop_gpu import build as build_cocoop
from tests.test_coop_gpu import build as build_coop
from tests.test_model_gpu import build as build_mudpt
from tests.test_umudpt_gpu import build as build_umudpt, load as load_umudpt
from tests.test_uumudpt_gpu import build as build_uumudpt, load as load_uumudpt
from tests.test_vpt_gpu import build as build_vpt
from tests.test_zsclip_gpu import build as build_frozen
from tests import vpt_reference as VR

pytestmark = pytest.mark.gpu
DTYPES = ["fp16", "bf16", "fp32"]
COOP_TINY = ["coop_tiny_end", "coop_tiny_end_csc", "coop_tiny_middle", "coop_tiny_middle_csc"]
_CASES = {}


def case_of(name):
    if name not in _CASES:
        _CASES[name] = (ZR.ZsCase if name.startswith("zsclip") else CR.CoopCase if name.startswith("coop") else GoldenCase)(name)
    return _CASES[name]


def handle(name, dtype, max_batch=None, knobs=None):
    """A frozen, CoOp or CoCoOp handle on a tiny fixture, in eval mode."""
    case = case_of(name)
    if name.startswith("zsclip"):
        m = build_frozen(case, dtype, max_batch=max_batch, knobs=knobs)
    elif name.startswith("coop"):
        m = build_coop(case, dtype, max_batch=max_batch, knobs=knobs)
    else:
        m = build_cocoop(case.cfg, case.frozen, case.tokens, case.params, dtype, max_batch or len(case.labels), knobs=knobs)
    m.eval()
    return case, m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["zsclip_tiny", "zsclip2_tiny"])
def test_reference_features_give_the_reference_logits(name, dtype):
    """The fixture's own raw image_features through forward_features against the fixture's logits, held to what the image path is held to
    (tests/test_zsclip_gpu.py: check_logits with the helpers' bounds and the tiny shape's slack); it exercises less, the text side and the
    head only.  The parity mode ("fp32") has no bound of its own at this logit scale: its operands are fp16 pairs, never coarser than fp16's, so
    it is held to fp16's."""
    case, m = handle(name, dtype)
    logits = m.forward_features(case.image_features).cpu()
    m.close()
    check_logits(logits, case, "fp16" if dtype == "fp32" else dtype, f"{name} {dtype} from the fixture's features")


def chunks(B):
    """The batch in two chunks: uneven where B allows it."""
    return [(0, B)] if B < 2 else [(0, (B + 1) // 2), ((B + 1) // 2, B)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["zsclip_tiny", "zsclip2_tiny"] + COOP_TINY + ["cocoop_tiny"])
def test_forwarded_features_give_the_image_forwards_logits_bit_for_bit(name, dtype):
    case, m = handle(name, dtype)
    B = len(case.labels)
    whole = m(case.images)
    feats = m.image_features()
    assert tuple(feats.shape) == (B, case.cfg.embed_dim) and feats.dtype == torch.float32
    assert torch.equal(feats.cpu(), m.debug_read("image_features", B).view(B, -1))
    assert torch.equal(m.forward_features(feats), whole)
    assert torch.equal(m.image_features(), feats)  # a forward from features leaves them where an image forward does
    parts = [m.forward_features(feats[lo:hi]) for lo, hi in chunks(B)]
    assert torch.equal(torch.cat(parts), whole)
    one = m(case.images[B - 1:])  # B = 1
    f1 = m.image_features()
    assert tuple(f1.shape) == (1, case.cfg.embed_dim) and torch.equal(f1, feats[B - 1:]) and torch.equal(one, whole[B - 1:])
    assert torch.equal(m.forward_features(f1), one)
    if name.startswith("zsclip"):
        assert torch.equal(m.encode_image(case.images), feats)  # the linear-probe extractor's rows are the cached rows
    m.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cocoop_features_across_two_text_tower_chunks(dtype):
    """model.cpp sizes the per-image text tower's chunk as min(what 60 % of the free memory holds, max_batch, the knob cocoop_chunk).  At the
    tiny shape the memory term never binds (it allows far more than 16 images), so no batch <= 16 spans two chunks by it; the rule's cap
    term does: cocoop_chunk = 2 and the fixture's 3 images run as a pass of 2 and a pass of 1."""
    case, m = handle("cocoop_tiny", dtype, knobs={"cocoop_chunk": 2})
    B = len(case.labels)
    assert B == 3
    whole = m(case.images)
    feats = m.image_features()
    assert torch.equal(m.forward_features(feats), whole)
    assert torch.equal(torch.cat([m.forward_features(feats[:1]), m.forward_features(feats[1:])]), whole)  # 1 + 2: other chunk edges
    _, m1 = handle("cocoop_tiny", dtype)  # one pass of 3
    assert torch.equal(m1.forward_features(feats), whole)
    m.close()
    m1.close()


@pytest.mark.parametrize("name", ["coop_tiny_end", "coop_tiny_middle_csc"])
def test_forward_features_follows_a_context_write(name):
    case, m = handle(name, "fp16")
    launches = lambda: int(m.debug_read("text_launches", 1)[0].item())  # noqa: E731
    before = m(case.images)
    feats = m.image_features()
    n0 = launches()
    assert torch.equal(m.forward_features(feats), before)  # unchanged parameters: the text features are reused
    reused = launches() - n0
    with torch.no_grad():
        m.prompt_learner.ctx.data.mul_(1.5)  # a .data write does not move the version counter: the documented invalidation
    m.invalidate_text_cache()
    n1 = launches()
    from_features = m.forward_features(feats)
    assert launches() - n1 > reused and not torch.equal(from_features, before)  # the text tower ran again
    assert torch.equal(m(case.images), from_features)  # forward follows, and reuses what forward_features computed
    with torch.no_grad():
        m.prompt_learner.ctx.mul_(0.5)  # an in-place write moves the version counter
    after = m(case.images)
    assert not torch.equal(after, from_features) and torch.equal(m.forward_features(feats), after)
    # MUDPT_FWD_REUSE_TEXT before any text-tower pass: a state error from either entry
    _, fresh = handle(name, "fp16")
    out = torch.empty_like(before)
    assert fresh.lib.mudpt_forward_features(fresh._h, P(feats), feats.shape[0], P(out), capi.FWD_REUSE_TEXT, None) == 3
    assert b"forward_features: MUDPT_FWD_REUSE_TEXT" in fresh.lib.mudpt_last_error()
    fresh.close()
    m.close()


def test_a_handle_without_vision_weights_runs_from_features():
    from mudpt_amd.zsclip import FrozenCLIP
    case, m = handle("zsclip2_tiny", "fp16")
    logits = m(case.images)
    feats = m.image_features()
    text_only = {k: v for k, v in case.frozen.items() if not k.startswith("visual.")}
    assert len(text_only) < len(case.frozen)
    t = FrozenCLIP(case.shape(), text_only, case.tokens, max_batch=len(case.labels), dtype="fp16")
    assert torch.equal(t.forward_features(feats), logits)
    assert torch.equal(t.text_features(), m.text_features())
    with pytest.raises(capi.MudptError, match="bad state.*visual"):
        t(case.images)
    with pytest.raises(capi.MudptError, match="bad state.*visual"):
        t.encode_image(case.images)
    assert torch.equal(t.forward_features(feats), logits)  # the refused calls left the handle as it was
    t.close()
    m.close()


def other_variants():
    vpt, mpt = VR.VptCase("vpt_tiny"), VR.VptCase("mpt_tiny")
    return [("MuDPT", lambda: (case_of("mudpt_tiny"), build_mudpt(case_of("mudpt_tiny"), "fp16"))), ("VPT", lambda: (vpt, build_vpt(vpt, "fp16"))),
            ("MPT", lambda: (mpt, build_vpt(mpt, "fp16"))), ("UMuDPT", lambda: (load_umudpt("umudpt_tiny"), build_umudpt(load_umudpt("umudpt_tiny"), "fp16"))),
            ("UUMuDPT", lambda: (load_uumudpt("uumudpt_tiny"), build_uumudpt(load_uumudpt("uumudpt_tiny"), "fp16")))]


@pytest.mark.parametrize("variant", ["MuDPT", "VPT", "MPT", "UMuDPT", "UUMuDPT"])
def test_prompt_in_vision_variants_are_refused(variant):
    case, m = dict(other_variants())[variant]()
    m.eval()
    B = len(case.labels)
    before = m(case.images)
    feats = torch.randn(B, case.cfg.embed_dim, device="cuda")
    with pytest.raises(AssertionError, match=rf"refused for {variant}: its trainable prompts run inside the vision tower"):
        m.forward_features(feats)
    with pytest.raises(AssertionError, match=rf"refused for {variant}:"):
        m.image_features()
    assert torch.equal(m(case.images), before)
    m.close()


@pytest.mark.parametrize("name", ["zsclip_tiny", "coop_tiny_end", "cocoop_tiny"])
def test_bad_arguments_launch_nothing(name):
    case, m = handle(name, "fp16")
    lib, h, B, E = m.lib, m._h, len(case.labels), case.cfg.embed_dim
    sent = -1234.5
    out = torch.full((B + 1, m.n_cls), sent, device="cuda")
    feats = torch.randn(B + 1, E, device="cuda")
    # image_features before any forward
    assert lib.mudpt_image_features(h, B, P(feats), None) == 3 and b"no inference forward" in lib.mudpt_last_error()
    want = m(case.images)
    kept = m.image_features()
    launches = m.debug_read("text_launches", 1)[0].item()
    for call, word in ((lambda: lib.mudpt_forward_features(h, P(feats), 0, P(out), 0, None), b"outside 1..max_batch"),
                       (lambda: lib.mudpt_forward_features(h, P(feats), B + 1, P(out), 0, None), b"outside 1..max_batch"),
                       (lambda: lib.mudpt_forward_features(h, P(feats), -1, P(out), 0, None), b"outside 1..max_batch"),
                       (lambda: lib.mudpt_forward_features(h, None, B, P(out), 0, None), b"null"),
                       (lambda: lib.mudpt_forward_features(h, P(feats), B, None, 0, None), b"null"),
                       (lambda: lib.mudpt_image_features(h, B, None, None), b"null")):
        rc = call()
        assert rc == 1 and word in lib.mudpt_last_error(), (rc, lib.mudpt_last_error())
    assert lib.mudpt_image_features(h, B - 1, P(feats), None) == 3 and b"ran on" in lib.mudpt_last_error()  # another batch size
    torch.cuda.synchronize()
    assert (out == sent).all()  # nothing was written
    assert m.debug_read("text_launches", 1)[0].item() == launches
    assert torch.equal(m.debug_read("image_features", B).view(B, E), kept.cpu())  # ... nor copied over the handle's features
    assert torch.equal(m.image_features(), kept) and torch.equal(m.forward_features(kept), want)
    # the module's own checks: width, rank, batch
    for bad in (torch.zeros(B, E + 1), torch.zeros(B, 1, E), torch.zeros(0, E), torch.zeros(B + 1, E)):
        with pytest.raises(AssertionError):
            m.forward_features(bad)
    # a training step ends the validity of the kept features
    if not name.startswith("zsclip"):
        m.train()
        m.forward_backward(case.images, case.labels)
        assert lib.mudpt_image_features(h, B, P(feats), None) == 3 and b"training step" in lib.mudpt_last_error()
    m.close()


# ---- the trainers through dassl_lite ------------------------------------------------------------------------------------------------------
@pytest.fixture
def trainer_cfg(tmp_path, monkeypatch):
    from mudpt_amd import dassl_lite, tokenizer, trainer
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MUDPT_TEST_FEATURES", "MUDPT_DEVICE_TEST"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(tokenizer, "_default", None)
    monkeypatch.setattr(trainer, "_warned_fp16_scale", False)

    def make(name):
        if name.startswith("Zeroshot"):  # the templates' words, as tests/test_zsclip_gpu.py sets them up
            monkeypatch.setenv("MUDPT_BPE_VOCAB", ZR.merge_table_file(tmp_path))
        cfg = dassl_lite.default_cfg()
        cfg.TRAINER.NAME = name
        cfg.DATASET.NAME = "Caltech101"
        cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 4, 8
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 2, 4
        cfg.MODEL.BACKBONE.SYNTHETIC_SEED = 3
        cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH = 4, 2  # n_ctx 4: the benchmark prompts' recorded token ids (no merge table needed)
        cfg.TEST.PER_CLASS_RESULT = cfg.TEST.COMPUTE_CMAT = True
        cfg.OUTPUT_DIR = str(tmp_path / "out")
        (tmp_path / "out").mkdir(exist_ok=True)
        return cfg
    return make


def run_test_pass(t):
    """test() -> (its return value, evaluate()'s results key for key, the evaluator's whole device state: counts, per-class rows, confusion matrix)."""
    acc = t.test()
    return acc, dict(t.evaluator.evaluate()), t.evaluator._state.clone()


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and list(a[1]) == list(b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("name", ["ZeroshotCLIP", "CoOp", "CoCoOp"])
def test_trainer_test_pass_from_features(name, trainer_cfg, tmp_path, monkeypatch, capsys):
    from mudpt_amd import cocoop, coop, dassl_lite, featcache, zsclip  # noqa: F401 -- the plugins register themselves
    t = dassl_lite.build_trainer(trainer_cfg(name))
    model = t.model
    x, y = torch.cat([b["img"] for b in t.test_loader]), torch.cat([b["label"] for b in t.test_loader])
    t.test_loader = [{"img": x[:4], "label": y[:4]}, {"img": x[4:7], "label": y[4:7]}]  # dassl_lite's loader drops a short last batch: give it one
    on_images = run_test_pass(t)
    assert set(on_images[1]) == {"accuracy", "error_rate", "macro_f1", "perclass_accuracy"} and on_images[2].numel() > 11 * 11
    labels = torch.cat([b["label"] for b in t.test_loader])
    assert labels.numel() == 7
    # a store handed over: the same pass without the vision tower
    feats = []
    for b in t.test_loader:
        model(b["img"].cuda())
        feats.append(model.image_features())
    t.test_features = featcache.FeatureStore(torch.cat(feats), labels)
    capsys.readouterr()
    with monkeypatch.context() as mp:
        mp.setattr(type(model), "forward", lambda self, x: (_ for _ in ()).throw(RuntimeError("the image forward ran")))
        assert same(run_test_pass(t), on_images)
    assert "Cached test features: 7 rows" in capsys.readouterr().out
    del t.test_features
    assert "parse_batch_test" not in t.__dict__ and "model_inference" not in t.__dict__ and isinstance(t.test_loader, list)  # put back
    # the switch: the first pass runs on images and writes the file ...
    monkeypatch.setenv("MUDPT_TEST_FEATURES", str(tmp_path / "feat"))
    assert same(run_test_pass(t), on_images)
    path = tmp_path / "feat" / "Caltech101" / "test.npz"
    assert "wrote 7 rows" in capsys.readouterr().out and [p.name for p in path.parent.iterdir()] == ["test.npz"]
    with np.load(path) as z:  # the lpclip format
        assert sorted(z.files) == ["feature_list", "label_list"] and z["feature_list"].dtype == np.float32 and z["label_list"].dtype == np.int64
        assert z["feature_list"].shape == (7, 512) and np.array_equal(z["label_list"], labels.numpy())
        assert np.array_equal(z["feature_list"], torch.cat(feats).cpu().numpy())
    # ... the second reads it and never runs the image forward
    with monkeypatch.context() as mp:
        mp.setattr(type(model), "forward", lambda self, x: (_ for _ in ()).throw(RuntimeError("the image forward ran")))
        assert same(run_test_pass(t), on_images)
    assert f"Cached test features: 7 rows of {path}" in capsys.readouterr().out
    # one label changed: refused with a note, and the image pass runs
    with np.load(path) as z:
        f, y = z["feature_list"], z["label_list"].copy()
    y[3] = (y[3] + 1) % 11
    np.savez(path, feature_list=f, label_list=y)
    assert same(run_test_pass(t), on_images)
    out = capsys.readouterr().out
    assert "Cached test features refused: 1 of 7 labels differ" in out and "row 3" in out and "running on the images" in out
    with np.load(path) as z:
        assert np.array_equal(z["label_list"], y)  # a refused file is left as it is
    model.close()


def test_mudpt_under_the_switch_is_refused_and_tests_as_usual(trainer_cfg, tmp_path, monkeypatch, capsys):
    from mudpt_amd import dassl_lite
    t = dassl_lite.build_trainer(trainer_cfg("MuDPT"))
    on_images = run_test_pass(t)
    monkeypatch.setenv("MUDPT_TEST_FEATURES", str(tmp_path / "feat"))
    capsys.readouterr()
    assert same(run_test_pass(t), on_images)
    out = capsys.readouterr().out
    assert "Cached test features refused: MuDPT carries trainable prompts inside the vision tower" in out
    assert not (tmp_path / "feat").exists()
    t.model.close()
