"""No-GPU checks of the fused optimizer step: BucketOptimizer's torch backend (the float64 checker of the HIP kernel) against torch.optim
itself, state_dict interchange in both directions, the refusals, dassl_lite.build_optimizer and the host checks of mudpt_optim_apply."""
import copy
import ctypes as C
import types

import pytest
import torch

from tests import optim_reference as R

N = 1031                 # the issue's size: a 4-wide body plus a 3-element tail
SPLIT = (5, 26, 1000)    # ... as three parameters ([5], [2, 13], [1000]) at offsets that are no multiple of 4


def loose_params(dtype):
    """problem(N) as three separate parameters with their .grad tensors, and the gradient steps."""
    p0, grads = R.problem(N)
    params = [torch.nn.Parameter(c.clone().to(dtype).view(2, 13) if c.numel() == 26 else c.clone().to(dtype)) for c in p0.split(SPLIT)]
    for p in params:
        p.grad = torch.zeros_like(p)
    return params, grads


def bucket_model(dtype):
    """The same as views of one flat bucket, behind the two attributes BucketOptimizer reads of a model."""
    p0, grads = R.problem(N)
    model = types.SimpleNamespace(flat_params=p0.clone().to(dtype), flat_grads=torch.zeros(N, dtype=dtype))
    params, off = [], 0
    for n in SPLIT:
        shape = (2, 13) if n == 26 else (n,)
        p = torch.nn.Parameter(model.flat_params[off:off + n].view(shape))
        p.grad = model.flat_grads[off:off + n].view(shape)
        params.append(p)
        off += n
    return model, params, grads


def set_grads(params, g):
    with torch.no_grad():
        for p, c in zip(params, g.split(SPLIT)):
            p.grad.copy_(c.view_as(p))


def flat(tensors):
    return torch.cat([t.detach().flatten() for t in tensors])


def bucket_optimizer(name, params, **kw):
    from mudpt_amd.optim import BucketOptimizer
    algo, hyper = R.CONFIGS[name]
    return BucketOptimizer(params, algo, R.LR, backend="torch", **hyper, **kw)


@pytest.mark.parametrize("layout", ["loose", "bucket"])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_torch_backend_matches_torch_optim(name, layout):
    """Five steps of the torch backend against torch.optim's own class: in float64 equal to 1e-12, in fp32 inside the project's bound against
    the float64 run, parameters and every state tensor; as loose parameters (one rule application each) and as views of one bucket (one
    application for all)."""
    ref_p, ref_state = R.reference(name, N)
    for dtype in (torch.float64, torch.float32):
        if layout == "loose":
            params, grads = loose_params(dtype)
            opt = bucket_optimizer(name, params)
        else:
            model, params, grads = bucket_model(dtype)
            opt = bucket_optimizer(name, params, model=model)
            assert opt._whole
        for s in range(R.STEPS):
            set_grads(params, grads[s])
            opt.step()
        got = {"p": flat(params), **{k: flat([opt.state[p][k] for p in params]) for k in ref_state}}
        assert set(opt.state[params[0]]) - {"step"} == set(ref_state)
        for k, v in got.items():
            ref = ref_p if k == "p" else ref_state[k]
            if dtype == torch.float64:
                torch.testing.assert_close(v, ref, atol=1e-12, rtol=1e-12, msg=lambda m: f"{name} {k}: {m}")
            else:
                f = R.fraction(v, ref)
                print(f"{name} {layout} fp32 {k}: {f:.3f} of the bound")
                assert f <= 1.0, (name, k, f)
        if R.CONFIGS[name][0] != "sgd":
            assert float(opt.state[params[0]]["step"]) == R.STEPS


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_state_dict_interchange_in_both_directions(name):
    """3 steps in one kind of optimizer, state_dict -> load_state_dict into the other kind, 3 more steps: equal to 6 uninterrupted steps of
    torch.optim (float64, 1e-12), whichever kind ran first; the views still alias the flat buffers after the load."""
    p0, grads = R.problem(N, 6)
    want, _ = R.reference(name, N, 6)
    for first in ("torch", "bucket"):
        model, params, _ = bucket_model(torch.float64)
        mine, theirs = bucket_optimizer(name, params, model=model), R.torch_optimizer(name, params)
        a, b = (theirs, mine) if first == "torch" else (mine, theirs)
        for s in range(3):
            set_grads(params, grads[s])
            a.step()
        b.load_state_dict(a.state_dict())
        for s in range(3, 6):
            set_grads(params, grads[s])
            b.step()
        torch.testing.assert_close(model.flat_params, want, atol=1e-12, rtol=1e-12, msg=lambda m: f"{name}, {first} first: {m}")
        for key, buf in mine._flat.items():  # torch's keys are views at the parameter's offset
            off = 0
            for p, n in zip(params, SPLIT):
                assert mine.state[p][key].data_ptr() == buf.data_ptr() + off * buf.element_size() and mine.state[p][key].shape == p.shape
                off += n


def test_refusals():
    from mudpt_amd import dassl_lite
    from mudpt_amd.optim import BucketOptimizer
    params, grads = loose_params(torch.float64)
    theirs = R.torch_optimizer("adam", params)
    set_grads(params, grads[0])
    theirs.step()
    sd = copy.deepcopy(theirs.state_dict())
    sd["state"][1]["step"] = torch.tensor(3.0)  # per-parameter steps that differ
    with pytest.raises(ValueError, match="differing steps"):
        bucket_optimizer("adam", params).load_state_dict(sd)
    with pytest.raises(ValueError, match="does not belong"):  # an Adam state under RMSprop
        bucket_optimizer("rmsprop", params).load_state_dict(theirs.state_dict())
    with pytest.raises(ValueError, match="groups differ"):
        BucketOptimizer([{"params": params[:1]}, {"params": params[1:], "lr": 1e-3}], "adam", R.LR, backend="torch")
    same = BucketOptimizer([{"params": params[:1]}, {"params": params[1:]}], "adam", R.LR, backend="torch")  # groups that agree are one bucket
    same.step()
    same.param_groups[1]["lr"] = 1.0  # ... until they stop agreeing
    with pytest.raises(ValueError, match="groups differ"):
        same.step()
    for bad, word in ((torch.optim.Adagrad(params, lr=0.1), "Adagrad"), (torch.optim.Adam(params, maximize=True), "maximize"),
                      (torch.optim.SGD([{"params": params[:1]}, {"params": params[1:], "momentum": 0.5}], lr=0.1), "groups differ")):
        with pytest.raises(ValueError, match=word):
            BucketOptimizer.from_torch(bad, backend="torch")
    with pytest.raises(ValueError, match="whole bucket"):  # the HIP step is one launch over a model's bucket
        BucketOptimizer(params, "adam", R.LR, backend="hip")
    with pytest.raises(ValueError, match="not one of"):
        BucketOptimizer(params, "radam", R.LR, backend="torch")
    cfg = dassl_lite.default_cfg().OPTIM
    cfg.NAME = "radam"
    with pytest.raises(NotImplementedError, match="radam"):
        dassl_lite.build_optimizer(torch.nn.ParameterList(params), cfg)
    cfg.NAME = "lion"
    with pytest.raises(ValueError, match="must be one of"):
        dassl_lite.build_optimizer(torch.nn.ParameterList(params), cfg)


def test_build_optimizer_for_every_name():
    """dassl_lite.build_optimizer builds Dassl's torch class for each of its names from LR, WEIGHT_DECAY, MOMENTUM, SGD_DAMPNING, SGD_NESTEROV,
    ADAM_BETA1 / ADAM_BETA2 and RMSPROP_ALPHA, and from_torch carries every one of them over."""
    from mudpt_amd import dassl_lite
    from mudpt_amd.optim import BucketOptimizer
    cfg = dassl_lite.default_cfg().OPTIM
    assert (cfg.ADAM_BETA1, cfg.ADAM_BETA2, cfg.RMSPROP_ALPHA) == (0.9, 0.999, 0.99) and cfg.NAME == "sgd"
    cfg.LR, cfg.WEIGHT_DECAY, cfg.MOMENTUM, cfg.ADAM_BETA1, cfg.ADAM_BETA2, cfg.RMSPROP_ALPHA, cfg.SGD_DAMPNING = 0.003, 1e-3, 0.8, 0.85, 0.98, 0.95, 0.0
    params, _ = loose_params(torch.float32)
    module = torch.nn.ParameterList(params + [torch.nn.Parameter(torch.zeros(2), requires_grad=False)])
    want = {"sgd": (torch.optim.SGD, dict(momentum=0.8, dampening=0.0, nesterov=False)),
            "adam": (torch.optim.Adam, dict(betas=(0.85, 0.98), amsgrad=False, decoupled_weight_decay=False)),
            "amsgrad": (torch.optim.Adam, dict(betas=(0.85, 0.98), amsgrad=True, decoupled_weight_decay=False)),
            "adamw": (torch.optim.AdamW, dict(betas=(0.85, 0.98), amsgrad=False, decoupled_weight_decay=True)),
            "rmsprop": (torch.optim.RMSprop, dict(momentum=0.8, alpha=0.95, centered=False))}
    assert set(want) == set(dassl_lite.AVAI_OPTIMS)
    for name, (cls, hyper) in want.items():
        cfg.NAME = name
        opt = dassl_lite.build_optimizer(module, cfg)
        group = opt.param_groups[0]
        assert type(opt) is cls and len(opt.param_groups) == 1 and [id(p) for p in group["params"]] == [id(p) for p in params], name
        assert group["lr"] == 0.003 and group["weight_decay"] == 1e-3 and all(group[k] == v for k, v in hyper.items()), (name, group)
        mine = BucketOptimizer.from_torch(opt, backend="torch")
        assert mine.algo_name == name and {k: v for k, v in mine.param_groups[0].items() if k != "params"} == {k: v for k, v in group.items() if k != "params"}


def test_scheduler_and_zero_grad():
    """param_groups[0]["lr"] is read at every step, so a torch lr_scheduler drives the bucket as it drives torch.optim; zero_grad zeroes
    in place and never detaches the .grad views, whatever set_to_none says."""
    model, params, grads = bucket_model(torch.float64)
    twin, _ = loose_params(torch.float64)
    mine, theirs = bucket_optimizer("adam", params, model=model), R.torch_optimizer("adam", twin)
    scheds = [torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in (mine, theirs)]
    for s in range(3):
        set_grads(params, grads[s])
        set_grads(twin, grads[s])
        for o, sch in zip((mine, theirs), scheds):
            o.step()
            sch.step()
    assert mine.param_groups[0]["lr"] == theirs.param_groups[0]["lr"] == R.LR / 8
    torch.testing.assert_close(model.flat_params, flat(twin), atol=1e-12, rtol=1e-12)
    views = [p.grad for p in params]
    mine.zero_grad()  # set_to_none defaults to True in torch
    mine.zero_grad(set_to_none=True)
    assert all(p.grad is v for p, v in zip(params, views)) and model.flat_grads.abs().sum() == 0
    model.flat_grads.fill_(2.0)
    assert all((p.grad == 2.0).all() for p in params)


def test_optim_struct_mirrors_the_header():
    """capi.Optim is written by hand: its fields, in order, are those of `struct mudpt_optim` in include/mudpt.h, with the header's types."""
    import re
    from mudpt_amd import capi
    body = re.search(r"typedef struct mudpt_optim \{(.*?)\} mudpt_optim;", re.sub(r"/\*.*?\*/", "", open(capi.HEADER_PATH).read(), flags=re.S), flags=re.S).group(1)
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "float*": C.c_void_p * 3}
    fields = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        base, names = decl.split(None, 1)
        for n in (x.strip() for x in names.split(",")):
            fields.append((n.replace("[3]", ""), ctypes_of[base]))
    assert [(n, t._type_ if hasattr(t, "_length_") else t) for n, t in capi.Optim._fields_] == [(n, t._type_ if hasattr(t, "_length_") else t) for n, t in fields]
    assert (capi.OPTIM_SGD, capi.OPTIM_ADAM, capi.OPTIM_ADAMW, capi.OPTIM_RMSPROP) == (0, 1, 2, 3)


def test_optim_apply_refuses_on_the_host():
    """mudpt_optim_apply's checks read no memory, so they answer without a device: every one returns MUDPT_ERR_ARG with a message that names
    what is wrong, before anything is launched (the buffers here are host memory that no kernel could use)."""
    from mudpt_amd import build, capi
    import os
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    lib = capi.load()
    n = 64
    buf = {k: torch.zeros(n + 4) for k in ("p", "g", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "square_avg", "momentum_buffer", "grad_avg")}
    assert all(t.data_ptr() % 16 == 0 for t in buf.values())

    def refused(name, word, p="p", g="g", n=n, step=1, drop=None, edit=None, state=None):
        state = dict(buf, **(state or {}))
        o = R.optim_struct(name, step, state)
        if drop is not None:
            o.state[drop] = None
        if edit:
            setattr(o, *edit)
        ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else state[t].data_ptr())  # noqa: E731
        rc = lib.mudpt_optim_apply(C.byref(o), ptr(p), ptr(g), n, None)
        msg = lib.mudpt_last_error().decode()
        assert rc == 1 and word in msg, (name, word, rc, msg)

    assert lib.mudpt_optim_apply(None, None, None, n, None) == 1 and b"null" in lib.mudpt_last_error()
    for name in ("adam", "rmsprop_centered_momentum", "sgd_nesterov"):
        refused(name, "null", p=None)
        refused(name, "null", g=None)
        refused(name, "n = 0", n=0)
        refused(name, "step = 0", step=0)
        refused(name, "state[0]", drop=0)
        refused(name, "overlaps", g="p")
        refused(name, "overlaps", g=buf["p"].data_ptr() + 4 * (n - 4), n=n)  # the last four elements of p are the first of g
    refused("amsgrad", "state[2] (max_exp_avg_sq)", drop=2)
    refused("rmsprop_centered_momentum", "state[1] (momentum_buffer)", drop=1)
    refused("rmsprop_centered", "state[2] (grad_avg)", drop=2)
    refused("adam", "overlaps", state={"exp_avg_sq": buf["exp_avg"]})
    refused("adam", "p is not 16-byte aligned", p=buf["p"].data_ptr() + 4)
    refused("adam", "exp_avg_sq is not 16-byte aligned", state={"exp_avg_sq": buf["exp_avg_sq"][1:]})
    refused("rmsprop", "g is not 16-byte aligned", g=buf["g"].data_ptr() + 8)
    for name in ("adam", "rmsprop"):
        refused(name, "eps = 0", edit=("eps", 0.0))
        refused(name, "eps = -1", edit=("eps", -1.0))
    refused("adam", "beta1 1", edit=("beta1", 1.0))
    refused("adamw", "beta2 -0.1", edit=("beta2", -0.1))
    refused("adam", "lr", edit=("lr", float("nan")))
    refused("adam", "unknown algo 4", edit=("algo", 4))
    # a slot the configuration does not use may be null: plain Adam without max_exp_avg_sq gets past the state check (and is refused for n)
    refused("adam", "n = -3", n=-3, drop=2)
