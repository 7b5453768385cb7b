"""The fused optimizer step on the GPU: mudpt_optim_apply (the kernel alone) against torch.optim in float64, element independence and guard
regions; mudpt_optim_step on a tiny model; BucketOptimizer's HIP backend through the trainer plugin under MUDPT_FUSED_OPTIM=1."""
import copy
import ctypes as C

import pytest
import torch

from tests import optim_reference as R
from tests.helpers import SENT

pytestmark = pytest.mark.gpu

GUARD = 64  # fp32 elements (256 bytes) of SENT on either side of every buffer
# 1, 3: tail only; 4: one vector, no tail; 1031: 257 vectors (two blocks) plus a 3-element tail; 2048 * 256 * 4 + 1031: the capped grid's
# stride loop wraps (its second pass is ragged) and the tail follows it
SIZES = (1, 3, 4, 1031, 2048 * 256 * 4 + 1031)


def guarded(values, n):
    """A device buffer of n fp32 elements (``values``, or zeros) between two guard regions of SENT; the data starts 16-byte aligned and ends
    wherever n ends, so that a vector access over the tail would land in the rear guard."""
    whole = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    data = whole[GUARD:GUARD + n]
    assert data.data_ptr() % 16 == 0
    if values is None:
        data.zero_()
    else:
        data.copy_(values.to(torch.float32))
    return whole, data


def guards_intact(whole, n):
    return bool((whole[:GUARD] == SENT).all() and (whole[GUARD + n:] == SENT).all())


def apply_steps(name, p0, grads):
    """mudpt_optim_apply for every row of ``grads`` from p0 and zero state; returns {"p" | state key: (whole, data)} and g's buffers."""
    from mudpt_amd import capi
    lib, n = capi.load(), p0.numel()
    buf = {"p": guarded(p0, n), **{k: guarded(None, n) for k in R.state_keys(name) if k is not None}}
    gs = []
    for s in range(grads.shape[0]):
        g = guarded(grads[s], n)
        o = R.optim_struct(name, s + 1, {k: d for k, (_, d) in buf.items()})
        capi.check(lib.mudpt_optim_apply(C.byref(o), C.c_void_p(buf["p"][1].data_ptr()), C.c_void_p(g[1].data_ptr()), n, None), "optim_apply")
        gs.append(g)
    torch.cuda.synchronize()
    return buf, gs


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_apply_matches_torch_optim_in_float64(name, n):
    """Five steps of the kernel against torch.optim in float64 on the CPU from the same start: parameters and every state tensor inside the
    bound, the guard regions of all buffers (the read-only gradients included) untouched."""
    p0, grads = R.problem(n)
    ref_p, ref_state = R.reference(name, n)
    buf, gs = apply_steps(name, p0, grads)
    assert set(buf) - {"p"} == set(ref_state)
    for k, (whole, data) in buf.items():
        f = R.fraction(data, ref_p if k == "p" else ref_state[k])
        print(f"{name} n={n} {k}: {f:.3f} of the bound")
        assert f <= 1.0, (name, n, k, f)
        assert guards_intact(whole, n), (name, n, k)
    for s, (whole, data) in enumerate(gs):
        assert guards_intact(whole, n) and torch.equal(data.cpu().double(), grads[s]), (name, n, s)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_elements_are_independent(name):
    """Element i of p and of the states depends on element i of g alone: changing g[i] -- in the first vector, in a later block, in the tail
    -- changes those elements and nothing else, bit for bit; a NaN gradient poisons its own element only.  Two steps, so that the states a
    step reads are not all zero."""
    n = 1031
    p0, grads = R.problem(n)
    base, _ = apply_steps(name, p0, grads[:2])
    picks = [0, 5, 1027, 1030]  # vector 0 lane 0, vector 1 lane 1, the last vector's last lane, the last tail element
    for value in (0.37, float("nan")):
        changed = grads[:2].clone()
        changed[1, picks] = value
        got, _ = apply_steps(name, p0, changed)
        others = torch.ones(n, dtype=torch.bool, device="cuda")
        others[picks] = False
        for k in base:
            a, b = base[k][1], got[k][1]
            assert torch.equal(a[others].view(torch.int32), b[others].view(torch.int32)), (name, k, value)
            if value != value:
                assert torch.isnan(b[picks]).all(), (name, k, b[picks])
            else:
                assert (a[picks] != b[picks]).all() and torch.isfinite(b[picks]).all(), (name, k)


def tiny_model():
    from tests.helpers import GoldenCase
    from tests.test_model_gpu import build
    case = GoldenCase("mudpt_tiny")
    return case, build(case, "fp16")


def test_optim_step_on_a_model_matches_torch_adam():
    """mudpt_optim_step on the bound buckets of a CustomCLIP handle: two forward_backward + Adam steps against torch.optim.Adam in float64 on
    copies of the same gradients, the caller-owned state included."""
    from mudpt_amd import capi
    case, m = tiny_model()
    n = m.flat_params.numel()
    state = {k: torch.zeros(n, dtype=torch.float32, device="cuda") for k in ("exp_avg", "exp_avg_sq")}
    ref = torch.nn.Parameter(m.flat_params.detach().cpu().double())
    theirs = R.torch_optimizer("adam", [ref])
    for step in (1, 2):
        m.forward_backward(case.images, case.labels)
        ref.grad = m.flat_grads.detach().cpu().double()
        with torch.no_grad():
            ref.copy_(m.flat_params.detach().cpu().double())  # each step from the library's own parameters: the bound is per step
        theirs.step()
        o = R.optim_struct("adam", step, state)
        capi.check(m.lib.mudpt_optim_step(m._h, C.byref(o), m._stream()), "optim_step")
        m.invalidate_text_cache()
        torch.cuda.synchronize()
        for k, got in (("p", m.flat_params), ("exp_avg", state["exp_avg"]), ("exp_avg_sq", state["exp_avg_sq"])):
            f = R.fraction(got, ref.detach() if k == "p" else theirs.state[ref][k])
            print(f"step {step} {k}: {f:.3f} of the bound")
            assert f <= 1.0, (step, k, f)
    assert ref.grad.abs().max() > 0
    m.close()


def test_optim_step_refuses_a_frozen_handle():
    from mudpt_amd import capi
    from mudpt_amd.model import library_config, ModelShape
    lib = capi.load()
    cfg = library_config(ModelShape(image_size=32, patch=16, v_width=192, v_layers=3, v_heads=3, t_width=128, t_layers=3, t_heads=2, embed_dim=128), 11, 2, "fp16",
                         frozen=True)
    h = C.c_void_p()
    capi.check(lib.mudpt_create_frozen(C.byref(cfg), C.byref(h)), "create_frozen")
    state = {k: torch.zeros(8, device="cuda") for k in ("exp_avg", "exp_avg_sq")}
    o = R.optim_struct("adam", 1, state)
    assert lib.mudpt_optim_step(h, C.byref(o), None) == 1 and b"frozen" in lib.mudpt_last_error()
    assert lib.mudpt_optim_step(None, C.byref(o), None) == 1 and lib.mudpt_optim_step(h, None, None) == 1
    lib.mudpt_destroy(h)


def test_bucket_optimizer_hip_backend_on_a_model():
    """BucketOptimizer(backend="hip") over a CustomCLIP's trainables against its own torch backend in float64 on copies of the same
    gradients, for one configuration per kernel family; the step invalidates the model's cached text features.  RMSprop runs in its
    centered form without momentum: a model's gradients change sign from step to step, and where they cancel RMSprop's momentum buffer no
    fp32 evaluation holds the bound's absolute term (optim_reference.problem); that form is held by the sequences of
    test_apply_matches_torch_optim_in_float64."""
    from mudpt_amd.optim import BucketOptimizer
    case, m = tiny_model()
    params = list(m.parameters())
    for name in ("amsgrad", "adamw", "rmsprop_centered", "sgd_nesterov"):
        algo, hyper = R.CONFIGS[name]
        mine = BucketOptimizer(params, algo, R.LR, model=m, backend="hip", **hyper)
        twin = torch.nn.Parameter(m.flat_params.detach().cpu().double())
        check = BucketOptimizer([twin], algo, R.LR, backend="torch", **hyper)
        for step in range(2):
            m.forward_backward(case.images, case.labels)
            twin.grad = m.flat_grads.detach().cpu().double()
            with torch.no_grad():
                twin.copy_(m.flat_params.detach().cpu().double())
            m._text_version = 12345
            mine.step()
            assert m._text_version is None
            check.step()
            for k in ["p"] + [k for k in R.state_keys(name) if k is not None]:
                got = m.flat_params if k == "p" else mine._flat[k]
                f = R.fraction(got, twin.detach() if k == "p" else check.state[twin][k])
                print(f"{name} step {step + 1} {k}: {f:.3f} of the bound")
                assert f <= 1.0, (name, step, k, f)
        for p in params:  # torch's keys, as views of the flat state at the parameter's offset
            off = (p.data_ptr() - m.flat_params.data_ptr()) // 4
            for k, flat in mine._flat.items():
                assert mine.state[p][k].data_ptr() == flat.data_ptr() + 4 * off and mine.state[p][k].shape == p.shape
    m.close()


def plugin(tmp_path, optim_name, fused, monkeypatch):
    from mudpt_amd import dassl_lite, trainer  # noqa: F401  (registers the plugin)
    if fused:
        monkeypatch.setenv("MUDPT_FUSED_OPTIM", "1")
    else:
        monkeypatch.delenv("MUDPT_FUSED_OPTIM", raising=False)
    cfg = dassl_lite.default_cfg()
    cfg.OUTPUT_DIR = str(tmp_path / f"{optim_name}_{int(fused)}")
    cfg.OPTIM.NAME, cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.LR = optim_name, 1, 0, 0.0025
    cfg.DATASET.NUM_TRAIN, cfg.DATASET.NUM_TEST = 8, 4
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE = 4, 4
    cfg.TRAINER.MUDPT.N_CTX, cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH = 4, 12
    return dassl_lite.build_trainer(cfg)


@pytest.mark.parametrize("optim_name", ["adam", "sgd"])
def test_plugin_under_the_opt_in_matches_the_run_without_it(optim_name, tmp_path, monkeypatch, capsys):
    """One epoch at B 4 (two steps) on dassl_lite's synthetic data with MUDPT_FUSED_OPTIM=1 against the same run without it: losses equal,
    parameters and optimizer state inside the bound after every step.  The bound is per step from a common start -- Adam divides by the root
    of the second moment, so a last-bit difference in step 1 is a visible difference in the tiny gradient elements of step 2 -- hence the
    plain run takes over the fused run's parameters and, through state_dict / load_state_dict, its optimizer state before step 2.  Then the
    checkpoint each run writes loads into the other kind of run."""
    from mudpt_amd.optim import BucketOptimizer
    a, b = plugin(tmp_path, optim_name, True, monkeypatch), plugin(tmp_path, optim_name, False, monkeypatch)
    assert "Fused optimizer step: " + optim_name in capsys.readouterr().out
    assert isinstance(a.optim, BucketOptimizer) and a.optim.backend == "hip" and type(b.optim) is (torch.optim.Adam if optim_name == "adam" else torch.optim.SGD)
    assert a.sched.optimizer is a.optim
    keys = ["exp_avg", "exp_avg_sq"] if optim_name == "adam" else ["momentum_buffer"]
    for t in (a, b):
        t.set_model_mode("train")
        t.num_batches = len(t.train_loader_x)
    batches = list(b.train_loader_x)
    assert len(batches) == 2
    for step, batch in enumerate(batches):
        if step:
            with torch.no_grad():
                b.model.flat_params.copy_(a.model.flat_params)
            b.optim.load_state_dict(copy.deepcopy(a.optim.state_dict()))  # torch's load_state_dict keeps tensors that need no cast: without the copy b would step a's state
        a.batch_idx = b.batch_idx = step
        la, lb = a.forward_backward(batch)["loss"], b.forward_backward(batch)["loss"]
        assert la == lb and la == la, (step, la, lb)
        assert torch.equal(a.model.flat_grads, b.model.flat_grads)
        fr = {"p": R.fraction(a.model.flat_params, b.model.flat_params.cpu())}
        for k in keys:
            theirs = torch.cat([b.optim.state[p][k].flatten() for p in b.model.parameters()])
            fr[k] = R.fraction(a.optim._flat[k], theirs.cpu())
        print(f"{optim_name} step {step + 1}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()) + " of the bound")
        assert max(fr.values()) <= 1.0, (step, fr)
    assert a.optim.param_groups[0]["lr"] == b.optim.param_groups[0]["lr"]  # the scheduler stepped both at the end of the epoch
    # the checkpoint of each kind of run resumes in the other kind
    from mudpt_amd import dassl_lite
    for src, dst in ((a, b), (b, a)):
        src.save_model(0, src.output_dir)
        ckpt = dassl_lite.load_checkpoint(f"{src.output_dir}/MultimodalDeepPromptTuning/model.pth.tar-1")
        dst.load_model(src.output_dir, epoch=1)
        dst.optim.load_state_dict(ckpt["optimizer"])
        assert torch.equal(dst.model.flat_params, src.model.flat_params)
        for k in keys:
            want = torch.cat([src.optim.state[p][k].flatten() for p in src.model.parameters()])
            got = torch.cat([dst.optim.state[p][k].flatten() for p in dst.model.parameters()])
            assert torch.equal(got, want), k
        out = dst.forward_backward(batches[0])
        assert out["loss"] == out["loss"]
    a.model.close()
    b.model.close()


def test_plugin_refuses_what_the_fused_step_does_not_cover(tmp_path, monkeypatch, capsys):
    """Under the opt-in an optimizer the fused step does not restate stays torch's, after a one-line note, and trains: here build_optimizer
    hands build_model an Adagrad.  The other refusals, on the same model: an SGD over a part of the bucket, maximize."""
    from mudpt_amd import trainer as T
    monkeypatch.setattr(T, "build_optimizer", lambda module, cfg: torch.optim.Adagrad([p for p in module.parameters() if p.requires_grad], lr=cfg.LR))
    t = plugin(tmp_path, "sgd", True, monkeypatch)
    notes = [line for line in capsys.readouterr().out.splitlines() if line.startswith("Fused optimizer step")]
    assert len(notes) == 1 and notes[0].startswith("Fused optimizer step refused: Adagrad is not") and type(t.optim) is torch.optim.Adagrad, notes
    for bad, word in ((torch.optim.SGD(list(t.model.parameters())[:3], lr=0.01), "not exactly the tensors of its bucket"),
                      (torch.optim.Adam(t.model.parameters(), lr=0.01, maximize=True), "maximize")):
        assert T.fused_optimizer(t.model, bad) is bad
        note = capsys.readouterr().out
        assert note.startswith("Fused optimizer step refused: ") and word in note and note.count("\n") == 1, note
    t.set_model_mode("train")
    t.batch_idx, t.num_batches = 0, 99
    before = t.model.flat_params.clone()
    out = t.forward_backward(next(iter(t.train_loader_x)))
    assert out["loss"] == out["loss"] and not torch.equal(t.model.flat_params, before)
    t.model.close()
