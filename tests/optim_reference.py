"""What tests/test_optim_cpu.py and tests/test_optim_gpu.py share: the optimizer configurations, the seeded problem, torch.optim in float64 on
the CPU as the reference (computed once per configuration and size) and the project's bound for its fused optimizer steps."""
import functools

import torch

ATOL, RTOL = 1e-7, 1e-6  # the bound of the fused SGD (tests/test_model_gpu.py::test_sgd_step_matches_torch): |x - ref| <= ATOL + RTOL |ref|
STEPS, LR = 5, 2.5e-3

# name -> (BucketOptimizer algo, its keyword arguments): every algorithm and flag of the fused step.  RMSprop's momentum forms run without
# weight decay (the plain form has it): their step, lr momentum_buffer, is up to 0.1 here and carries small parameters across zero, after
# which grad + weight_decay param cancels and the buffer inherits that sum's absolute error (torch's own fp32 run: 5 - 7 x the bound on
# the buffer at 2 098 183 elements, inside it on everything else) -- see problem() on what the bound can hold
CONFIGS = {
    "adam": ("adam", dict(weight_decay=5e-4)),
    "amsgrad": ("amsgrad", dict(weight_decay=5e-4)),
    "adamw": ("adamw", dict(weight_decay=1e-2)),
    "adam_nowd": ("adam", dict(betas=(0.8, 0.99), eps=1e-6)),
    "rmsprop": ("rmsprop", dict(weight_decay=5e-4)),
    "rmsprop_momentum": ("rmsprop", dict(momentum=0.9)),
    "rmsprop_centered": ("rmsprop", dict(centered=True, alpha=0.9)),
    "rmsprop_centered_momentum": ("rmsprop", dict(centered=True, momentum=0.9)),
    "sgd_nesterov": ("sgd", dict(momentum=0.9, weight_decay=5e-4, nesterov=True)),
    "sgd_dampening": ("sgd", dict(momentum=0.9, weight_decay=5e-4, dampening=0.1)),
}


def torch_optimizer(name, params, lr=LR):
    """The torch.optim class a configuration restates, over ``params``."""
    algo, kw = CONFIGS[name]
    if algo == "sgd":
        return torch.optim.SGD(params, lr=lr, **kw)
    if algo == "rmsprop":
        return torch.optim.RMSprop(params, lr=lr, **kw)
    if algo == "adamw":
        return torch.optim.AdamW(params, lr=lr, **kw)
    return torch.optim.Adam(params, lr=lr, amsgrad=algo == "amsgrad", **kw)


def state_keys(name):
    """The state tensors of a configuration in the order of mudpt_optim.state's slots (None: unused)."""
    from mudpt_amd.optim import _state_keys
    algo, kw = CONFIGS[name]
    group = dict(momentum=kw.get("momentum", 0.0), amsgrad=algo == "amsgrad", centered=kw.get("centered", False))
    return _state_keys("adam" if algo in ("adam", "amsgrad", "adamw") else algo, group)


@functools.lru_cache(maxsize=None)
def problem(n, steps=STEPS):
    """(p0 [n], grads [steps, n]) in float64, every value exactly representable in fp32.  Parameters N(0, 0.02^2), seven of them x 50; gradient
    magnitudes log-uniform in [1e-5, 1], redrawn every step, with 40 exact zeros per step (fewer where n is small): no square is subnormal.
    An element's gradients keep ONE sign over the steps.  The bound's absolute term, 1e-7, is an fp32 half-ulp at magnitude 1; RMSprop's
    momentum buffer sums terms grad / sqrt(square_avg) of magnitude up to 1 / sqrt(1 - alpha) = 10, whose half-ulp is 4.8e-7.  Where a sign
    change cancels that sum, what is left carries the absolute error of its terms, and no fp32 evaluation of the rule holds 1e-7 there: torch's
    own RMSprop(momentum=0.9) in fp32 is at 16.8 x the bound on its momentum buffer after five steps of gradients with random signs per step
    (everything else: inside it).  Without cancellation it is the relative term that binds, which is what the bound is meant to check."""
    g = torch.Generator().manual_seed(1000 + n)
    p = 0.02 * torch.randn(n, generator=g, dtype=torch.float64)
    p[torch.randperm(n, generator=g)[:min(7, n)]] *= 50
    mag = 10.0 ** (-5.0 * torch.rand(steps, n, generator=g, dtype=torch.float64))
    grads = mag * torch.where(p < 0, -1.0, 1.0)
    for s in range(steps):
        grads[s, torch.randperm(n, generator=g)[:min(40, n // 4)]] = 0.0
    return p.float().double(), grads.float().double()


@functools.lru_cache(maxsize=None)
def reference(name, n, steps=STEPS):
    """torch.optim in FLOAT64 on the CPU from problem(n): (parameters [n], {state key: [n]}) after ``steps`` steps.  Computed once; the
    callers leave it unchanged."""
    p0, grads = problem(n, steps)
    p = torch.nn.Parameter(p0.clone())
    opt = torch_optimizer(name, [p])
    for s in range(steps):
        p.grad = grads[s].clone()
        opt.step()
    return p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items() if k != "step" and v is not None}


def fraction(got, ref):
    """The largest |got - ref| as a fraction of the bound; NaN anywhere counts as infinite."""
    got, ref = got.detach().double().cpu().flatten(), ref.double().flatten()
    f = ((got - ref).abs() / (ATOL + RTOL * ref.abs())).max().item()
    return f if f == f else float("inf")


def optim_struct(name, step, state, lr=LR):
    """capi.Optim of a configuration for update ``step``; ``state``: {key: fp32 device tensor}."""
    from mudpt_amd import capi
    algo, kw = CONFIGS[name]
    o = capi.Optim()
    o.algo = {"sgd": capi.OPTIM_SGD, "adam": capi.OPTIM_ADAM, "amsgrad": capi.OPTIM_ADAM, "adamw": capi.OPTIM_ADAMW, "rmsprop": capi.OPTIM_RMSPROP}[algo]
    o.lr, o.step = lr, step
    o.beta1, o.beta2 = kw.get("betas", (0.9, 0.999))
    o.eps, o.weight_decay, o.momentum = kw.get("eps", 1e-8), kw.get("weight_decay", 0.0), kw.get("momentum", 0.0)
    o.alpha, o.dampening = kw.get("alpha", 0.99), kw.get("dampening", 0.0)
    o.nesterov, o.amsgrad, o.centered = int(kw.get("nesterov", False)), int(algo == "amsgrad"), int(kw.get("centered", False))
    for slot, key in enumerate(state_keys(name)):
        o.state[slot] = None if key is None else state[key].data_ptr()
    return o
