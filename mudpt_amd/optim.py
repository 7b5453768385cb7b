"""``BucketOptimizer``: torch.optim's SGD, Adam (amsgrad), AdamW and RMSprop over the ONE flat bucket a model's trainables are views of, the
step being one ``mudpt_optim_step`` launch (mudpt_amd/csrc/optim.hip) instead of torch's chain of foreach launches.

The rules are those of torch 2.10's single-tensor paths (torch/optim/adam.py::_single_tensor_adam, the non-capturable branch;
torch/optim/rmsprop.py::_single_tensor_rmsprop; torch/optim/sgd.py::_single_tensor_sgd).  ``backend="torch"`` restates them in plain torch
ops on any device and dtype: it is the float64 checker of the HIP kernel and runs without a GPU, as ``LogisticProbe(evaluator=...)`` does
for the probe.  ``backend="hip"`` needs the model whose bucket the parameters are views of.

The state lives in flat tensors laid out as the bucket; ``self.state[p]`` holds torch's own keys (``step``, ``exp_avg``, ``exp_avg_sq``,
``max_exp_avg_sq``, ``square_avg``, ``momentum_buffer``, ``grad_avg``) as views at ``p``'s offset, and the parameter group carries the keys
of the torch class it stands for, so ``state_dict()`` is torch's format in both directions: a checkpoint written under either kind of
optimizer resumes under the other.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import torch

ALGOS = ("sgd", "adam", "amsgrad", "adamw", "rmsprop")
_TORCH_CLASSES = {torch.optim.SGD: "sgd", torch.optim.Adam: "adam", torch.optim.AdamW: "adam", torch.optim.RMSprop: "rmsprop"}
_UNSUPPORTED_FLAGS = ("maximize", "capturable", "differentiable")  # each changes the rule or its graph: not restated here


def _state_keys(family: str, group: dict) -> List[str]:
    """The state tensors of the configuration, in the order of mudpt_optim.state's slots (None: the slot is not used)."""
    if family == "sgd":
        return ["momentum_buffer" if group["momentum"] != 0 else None, None, None]
    if family == "adam":
        return ["exp_avg", "exp_avg_sq", "max_exp_avg_sq" if group["amsgrad"] else None]
    return ["square_avg", "momentum_buffer" if group["momentum"] > 0 else None, "grad_avg" if group["centered"] else None]


class BucketOptimizer(torch.optim.Optimizer):
    def __init__(self, params, algo: str, lr: float, *, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, momentum: float = 0.0,
                 alpha: float = 0.99, dampening: float = 0.0, nesterov: bool = False, amsgrad: bool = False, centered: bool = False, model=None,
                 backend: str = "hip"):
        if algo not in ALGOS:
            raise ValueError(f"algo {algo!r} is not one of {', '.join(ALGOS)}")
        if backend not in ("hip", "torch"):
            raise ValueError(f"backend {backend!r} is not 'hip' or 'torch'")
        if lr < 0 or eps <= 0 or weight_decay < 0 or momentum < 0 or alpha < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"invalid hyper-parameter: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}, momentum {momentum}, alpha {alpha}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.family = "adam" if algo in ("adam", "amsgrad", "adamw") else algo
        # the keys of the torch class the group stands for, so that either optimizer loads the other's state_dict
        if self.family == "sgd":
            defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False, foreach=None,
                            differentiable=False, fused=None)
        elif self.family == "adam":
            defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad) or algo == "amsgrad", maximize=False, foreach=None,
                            capturable=False, differentiable=False, fused=None, decoupled_weight_decay=algo == "adamw")
        else:
            defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=bool(centered), weight_decay=weight_decay, capturable=False, foreach=None,
                            maximize=False, differentiable=False)
        super().__init__(params, defaults)
        self.backend, self.model = backend, model
        self._hyper()  # several groups are one group only if their hyper-parameters agree
        plist = [p for g in self.param_groups for p in g["params"]]
        first = plist[0]
        if any(p.dtype != first.dtype or p.device != first.device for p in plist):
            raise ValueError("the parameters differ in dtype or device: they are not one bucket")
        if model is not None:
            bucket, item = model.flat_params, model.flat_params.element_size()
            self._span = {}
            for p in plist:
                off = (p.data_ptr() - bucket.data_ptr()) // item
                inside = p.dtype == bucket.dtype and p.device == bucket.device and p.is_contiguous() and 0 <= off and off + p.numel() <= bucket.numel()
                if not inside or p.grad is None or p.grad.data_ptr() != model.flat_grads.data_ptr() + off * item:
                    raise ValueError("a parameter (or its .grad) is not a view of the model's flat bucket")
                self._span[p] = (off, p.numel())
            self._total = bucket.numel()
            spans = sorted(self._span.values())
            self._whole = sum(n for _, n in spans) == self._total and all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))
        else:
            self._span, self._total, self._whole = {}, 0, False
            for p in plist:
                self._span[p] = (self._total, p.numel())
                self._total += p.numel()
        if backend == "hip":
            if model is None or not self._whole:
                raise ValueError("the HIP step runs over a model's whole bucket: the parameters are not exactly the tensors of its bucket")
            if first.dtype != torch.float32 or first.device.type != "cuda":
                raise ValueError("the HIP step runs on fp32 device memory")
        self._dtype, self._device = first.dtype, first.device
        self._flat: Dict[str, torch.Tensor] = {}
        self._step = 0
        self._step_t = torch.tensor(0.0, dtype=torch.float32)  # torch keeps `step` as a CPU float32 scalar per parameter: here one, shared

    @classmethod
    def from_torch(cls, optim: torch.optim.Optimizer, model=None, backend: str = "hip") -> "BucketOptimizer":
        """The BucketOptimizer of the same hyper-parameters (and, if ``optim`` has stepped, the same state) as a torch.optim.SGD / Adam /
        AdamW / RMSprop.  ValueError, with the reason in one line, for anything else: another class, groups with differing hyper-parameters,
        maximize / capturable / differentiable, parameters that are not the bucket."""
        family = _TORCH_CLASSES.get(type(optim))
        if family is None:
            raise ValueError(f"{type(optim).__name__} is not torch.optim.SGD, Adam, AdamW or RMSprop")
        hypers = [{k: v for k, v in g.items() if k != "params"} for g in optim.param_groups]
        if any(h != hypers[0] for h in hypers[1:]):
            raise ValueError("its parameter groups differ in their hyper-parameters")
        h = hypers[0]
        for flag in _UNSUPPORTED_FLAGS:
            if h.get(flag):
                raise ValueError(f"{flag}=True is not built")
        if isinstance(h["lr"], torch.Tensor):
            raise ValueError("a tensor lr is not built")
        algo = ("adamw" if h.get("decoupled_weight_decay") else "adam") if family == "adam" else family
        names = {"sgd": ("momentum", "dampening", "weight_decay", "nesterov"), "adam": ("betas", "eps", "weight_decay", "amsgrad"),
                 "rmsprop": ("momentum", "alpha", "eps", "centered", "weight_decay")}[family]
        new = cls([{"params": list(g["params"])} for g in optim.param_groups], algo, h["lr"], model=model, backend=backend, **{k: h[k] for k in names})
        if len(optim.state) > 0:
            new.load_state_dict(optim.state_dict())
        return new

    @property
    def algo_name(self) -> str:
        g = self.param_groups[0]
        return {"sgd": "sgd", "rmsprop": "rmsprop"}.get(self.family) or ("adamw" if g["decoupled_weight_decay"] else "amsgrad" if g["amsgrad"] else "adam")

    def _hyper(self) -> dict:
        """The hyper-parameters of this step: param_groups[0]'s, read now (an lr_scheduler writes there).  More than one group is one group
        as long as they agree in every key."""
        groups = self.param_groups
        h = {k: v for k, v in groups[0].items() if k != "params"}
        for g in groups[1:]:
            if {k: v for k, v in g.items() if k != "params"} != h:
                raise ValueError("BucketOptimizer steps one bucket with one set of hyper-parameters: its parameter groups differ")
        for flag in _UNSUPPORTED_FLAGS:
            if h.get(flag):
                raise ValueError(f"BucketOptimizer: {flag}=True is not built")
        return h

    def _ensure_state(self, h: dict):
        """Flat zero buffers for the state tensors the configuration needs, and their views in self.state."""
        keys = [k for k in _state_keys(self.family, h) if k is not None and k not in self._flat]
        for k in keys:
            self._flat[k] = torch.zeros(self._total, dtype=self._dtype, device=self._device)
        if keys or len(self.state) == 0:
            for p, (off, n) in self._span.items():
                st = self.state[p]
                if self.family != "sgd":
                    st["step"] = self._step_t
                for k, flat in self._flat.items():
                    st[k] = flat[off:off + n].view_as(p)

    def _segments(self):
        """(param, grad, {key: state}) runs the torch backend updates: the whole bucket at once where the parameters are exactly that."""
        if self._whole:
            return [(self.model.flat_params, self.model.flat_grads, self._flat)]
        out = []
        for p in self._span:
            if p.grad is None:
                raise RuntimeError("BucketOptimizer keeps one step count for the bucket: every parameter needs a .grad")
            out.append((p.data, p.grad, self.state[p]))
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        h = self._hyper()
        self._ensure_state(h)
        self._step += 1
        if self.backend == "hip":
            self._hip_step(h)
        else:
            rule = {"sgd": self._sgd, "adam": self._adam, "rmsprop": self._rmsprop}[self.family]
            for p, g, st in self._segments():
                rule(p, g, st, h, self._step)
        self._step_t.fill_(self._step)
        if self.model is not None and hasattr(self.model, "invalidate_text_cache"):
            self.model.invalidate_text_cache()  # the parameters moved behind the bucket's version counter (as Model.sgd_step)
        return loss

    def _hip_step(self, h: dict):
        from . import capi
        o = capi.Optim()
        o.algo = {"sgd": capi.OPTIM_SGD, "rmsprop": capi.OPTIM_RMSPROP}.get(self.family, capi.OPTIM_ADAMW if h.get("decoupled_weight_decay") else capi.OPTIM_ADAM)
        o.lr, o.weight_decay, o.step = float(h["lr"]), float(h["weight_decay"]), self._step
        o.beta1, o.beta2 = h.get("betas", (0.9, 0.999))
        o.eps, o.momentum, o.alpha, o.dampening = h.get("eps", 1e-8), h.get("momentum", 0.0), h.get("alpha", 0.99), h.get("dampening", 0.0)
        o.nesterov, o.amsgrad, o.centered = int(bool(h.get("nesterov"))), int(bool(h.get("amsgrad"))), int(bool(h.get("centered")))
        for slot, key in enumerate(_state_keys(self.family, h)):
            o.state[slot] = None if key is None else self._flat[key].data_ptr()
        m = self.model
        capi.check(m.lib.mudpt_optim_step(m._h, C.byref(o), m._stream()), "optim_step")

    # -- the rules, statement by statement as torch's single-tensor paths state them --------------------------------------------
    @staticmethod
    def _sgd(p, g, st, h, step):
        wd, momentum = h["weight_decay"], h["momentum"]
        if wd != 0:
            g = g.add(p, alpha=wd)
        if momentum != 0:
            buf = st["momentum_buffer"]
            if step == 1:
                buf.copy_(g)  # torch: buf = grad.clone()
            else:
                buf.mul_(momentum).add_(g, alpha=1 - h["dampening"])
            g = g.add(buf, alpha=momentum) if h["nesterov"] else buf
        p.add_(g, alpha=-h["lr"])

    @staticmethod
    def _adam(p, g, st, h, step):
        lr, wd, (beta1, beta2) = h["lr"], h["weight_decay"], h["betas"]
        if wd != 0:
            if h["decoupled_weight_decay"]:
                p.mul_(1 - lr * wd)
            else:
                g = g.add(p, alpha=wd)
        m, v = st["exp_avg"], st["exp_avg_sq"]
        m.lerp_(g, 1 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        bias_correction1, bias_correction2 = 1 - beta1 ** step, 1 - beta2 ** step
        step_size, bias_correction2_sqrt = lr / bias_correction1, bias_correction2 ** 0.5
        if h["amsgrad"]:
            vmax = st["max_exp_avg_sq"]
            torch.maximum(vmax, v, out=vmax)
            denom = (vmax.sqrt() / bias_correction2_sqrt).add_(h["eps"])
        else:
            denom = (v.sqrt() / bias_correction2_sqrt).add_(h["eps"])
        p.addcdiv_(m, denom, value=-step_size)

    @staticmethod
    def _rmsprop(p, g, st, h, step):
        lr, wd, alpha, momentum = h["lr"], h["weight_decay"], h["alpha"], h["momentum"]
        if wd != 0:
            g = g.add(p, alpha=wd)
        sq = st["square_avg"]
        sq.mul_(alpha).addcmul_(g, g, value=1 - alpha)
        if h["centered"]:
            gavg = st["grad_avg"]
            gavg.lerp_(g, 1 - alpha)
            avg = sq.addcmul(gavg, gavg, value=-1).sqrt_()
        else:
            avg = sq.sqrt()
        avg = avg.add_(h["eps"])
        if momentum > 0:
            buf = st["momentum_buffer"]
            buf.mul_(momentum).addcdiv_(g, avg)
            p.add_(buf, alpha=-lr)
        else:
            p.addcdiv_(g, avg, value=-lr)

    # -- torch.optim.Optimizer's surface ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def zero_grad(self, set_to_none: bool = True):
        """Zeroes the gradients in place.  ``set_to_none`` is ignored: the .grad views ARE the gradient bucket the library writes to, and a
        parameter that lost its view would train on nothing."""
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    p.grad.zero_()

    def state_dict(self):
        """torch's format.  The bucket's one ``step`` tensor goes out as a copy per parameter: torch's classes count on each in place."""
        out = super().state_dict()
        out["state"] = {i: {k: (v.clone() if k == "step" else v) for k, v in s.items()} for i, s in out["state"].items()}
        return out

    def load_state_dict(self, state_dict):
        """torch's format, from either kind of optimizer.  The tensors are copied INTO the flat buffers; the bucket has one step count, so
        per-parameter ``step`` values that differ are refused."""
        steps = {float(s["step"]) for s in state_dict["state"].values() if "step" in s}
        if len(steps) > 1:
            raise ValueError(f"BucketOptimizer keeps one step count for the bucket: the state holds the differing steps {sorted(steps)}")
        if any(s != int(s) or s < 0 for s in steps):
            raise ValueError(f"step {sorted(steps)} is not a count")
        lacking = sorted({k for k in self.defaults for g in state_dict["param_groups"] if k not in g})
        if lacking:
            raise ValueError(f"the state_dict does not belong to {self.algo_name}: its parameter groups lack {', '.join(lacking)}")
        super().load_state_dict(state_dict)  # copies of the tensors, cast to the parameters' dtype and device; the groups' hyper-parameters
        h = self._hyper()
        loaded = {p: dict(s) for p, s in self.state.items()}
        known = {k for k in _state_keys(self.family, h) if k is not None} | {"step"}
        unknown = sorted({k for s in loaded.values() for k in s} - known)
        if unknown:
            raise ValueError(f"state {', '.join(unknown)} does not belong to {self.algo_name} with these hyper-parameters")
        self.state.clear()
        self._flat = {}
        if steps:
            self._step = int(steps.pop())
        else:  # torch's SGD keeps no count: only whether a momentum buffer exists matters to the rule
            self._step = 1 if any("momentum_buffer" in s for s in loaded.values()) else 0
        self._step_t = torch.tensor(float(self._step), dtype=torch.float32)
        if loaded:
            self._ensure_state(h)
            for p, s in loaded.items():
                for k, t in s.items():
                    if k != "step":
                        self.state[p][k].copy_(t)
