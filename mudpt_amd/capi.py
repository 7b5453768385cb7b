"""ctypes binding of include/mudpt.h (libmudpt_hip.so).  No fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os
import re
from operator import itemgetter

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MUDPT_LIB") or os.path.join(HERE, "lib", "libmudpt_hip.so")  # MUDPT_LIB: A/B runs of two builds on one box
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "mudpt.h")

EPI_STORE, EPI_GELU, EPI_RESIDUAL, EPI_GELU_BWD, EPI_PATCH, EPI_STORE_F32 = range(6)  # kernels.h Epilogue: not a #define of the header


class MudptError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "image_size", "patch", "v_width", "v_layers", "v_heads", "t_width", "t_layers", "t_heads", "ctx_len",
        "embed_dim", "n_ctx", "depth", "n_cls", "max_batch", "dtype", "variant")]


class PromptShape(C.Structure):
    """mudpt_prompt_shape: TRAINER.VPT.* / TRAINER.MPT.* DEEP_TEXT_N_CTX, TEXT_PROMPT_DEPTH, DEEP_VISUAL_N_CTX, VISUAL_PROMPT_DEPTH."""
    _fields_ = [(n, C.c_int32) for n in ("t_n_ctx", "t_depth", "v_n_ctx", "v_depth")]


class ResnetShape(C.Structure):
    """mudpt_resnet_shape: the Bottleneck blocks of ModifiedResNet's four stages, its width and the heads of its attention pool."""
    _fields_ = [(n, C.c_int32) for n in ("layers1", "layers2", "layers3", "layers4", "width", "heads")]


class Optim(C.Structure):
    """mudpt_optim: one optimizer update.  The hyper-parameters are doubles (torch's Python floats), ``step`` the 1-based count of this update,
    ``state`` the caller-owned fp32 device buffers of the algorithm (include/mudpt.h names the slots)."""
    _fields_ = ([("algo", C.c_int32)] + [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "momentum", "alpha", "dampening")] +
                [(n, C.c_int32) for n in ("nesterov", "amsgrad", "centered")] + [("step", C.c_int64), ("state", C.c_void_p * 3)])


_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t}
_RETURNS = {"int": C.c_int32, "size_t": C.c_size_t, "const char*": C.c_char_p}


def parse_header(text):
    """name -> (restype, [(parameter name, ctype)]) of every `ret mudpt_name(params);` of a header, in the vocabulary include/mudpt.h uses:
    the scalars above, `const char*` (c_char_p) and any other pointer, `T**` or `T name[n]` (c_void_p: ctypes takes byref(x) there).  A type
    outside it raises with the declaration's name; nothing is guessed."""
    text = re.sub(r"^[ \t]*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?\**)\s*\b(mudpt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise MudptError(f"{name}: return type '{ret}' is outside the binding's vocabulary")
        args = []
        for p in (q.strip() for q in params.split(",") if params.strip() != "void"):
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\**)\s*(\w+)\s*(\[\d*\])?", p)
            base, stars, pname, array = m.groups() if m else (None, "", None, None)
            if stars or array:
                ctype = C.c_char_p if (base, stars, array) == ("char", "*", None) else C.c_void_p
            elif base in _SCALARS:
                ctype = _SCALARS[base]
            else:
                raise MudptError(f"{name}: parameter '{p}' is outside the binding's vocabulary")
            args.append((pname, ctype))
        out[name] = (_RETURNS[ret], args)
    missed = sorted(set(re.findall(r"\b(mudpt_[a-z0-9_]+)\s*\(", text)) - set(out))
    if missed:
        raise MudptError(f"{', '.join(missed)}: declared in a form that was not read")
    return out


def parse_defines(text, prefix):
    """{NAME: value} of every `#define <prefix>NAME <integer>` of a header."""
    return {n: int(v) for n, v in re.findall(rf"^[ \t]*#define\s+{prefix}(\w+)\s+(-?\d+)\b", text, flags=re.M)}


_HEADER = open(HEADER_PATH).read()
DECLARATIONS = parse_header(_HEADER)  # include/mudpt.h is the only statement of names, types and order
SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in DECLARATIONS.items()}  # name -> (restype, argtypes)
_DEFINES = parse_defines(_HEADER, "MUDPT_")
# spelled out, so that a #define that is gone fails here, at import, with its name (KeyError)
ABI_VERSION = _DEFINES["ABI_VERSION"]
BF16, F16, F32 = itemgetter("BF16", "F16", "F32")(_DEFINES)  # F32: the parity mode
VARIANT_MUDPT, VARIANT_COCOOP, VARIANT_COOP, VARIANT_COOP_CSC, VARIANT_VPT, VARIANT_MPT, VARIANT_UMUDPT, VARIANT_UUMUDPT = itemgetter(
    "VARIANT_MUDPT", "VARIANT_COCOOP", "VARIANT_COOP", "VARIANT_COOP_CSC", "VARIANT_VPT", "VARIANT_MPT", "VARIANT_UMUDPT", "VARIANT_UUMUDPT")(_DEFINES)
CLASS_TOKEN_END, CLASS_TOKEN_MIDDLE, CLASS_TOKEN_FRONT = itemgetter("CLASS_TOKEN_END", "CLASS_TOKEN_MIDDLE", "CLASS_TOKEN_FRONT")(_DEFINES)  # TRAINER.COOP.CLASS_TOKEN_POSITION
CP_VISION, CP_TEXT = itemgetter("CP_VISION", "CP_TEXT")(_DEFINES)  # mudpt_cp_backward parts
OPTIM_SGD, OPTIM_ADAM, OPTIM_ADAMW, OPTIM_RMSPROP = itemgetter("OPTIM_SGD", "OPTIM_ADAM", "OPTIM_ADAMW", "OPTIM_RMSPROP")(_DEFINES)  # mudpt_optim.algo
FWD_REUSE_TEXT, FWD_TRAINING = itemgetter("FWD_REUSE_TEXT", "FWD_TRAINING")(_DEFINES)  # mudpt_forward_ex / mudpt_cp_forward flags
# the codes of mudpt_attention_form / mudpt_gemm_form (MUDPT_ATTN_* / MUDPT_GEMM_*): the names after the prefix, ordered by value
ATTN_FORMS, GEMM_FORMS = (tuple(n[len(pre):] for n in sorted(_DEFINES, key=_DEFINES.get) if n.startswith(pre)) for pre in ("ATTN_", "GEMM_"))

_lib = None


def declared_functions():
    """Function names declared in include/mudpt.h."""
    return sorted(SIGNATURES)


def load():
    """Load libmudpt_hip.so (built by mudpt_amd.build / __graft_entry__.build()); never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MudptError(f"{LIB_PATH} is missing: run `python -m mudpt_amd.build` (hipcc, gfx950) first; "
                         "there is no CPU fallback for the MuDPT path")
    # torch ships its own libamdhip64; importing it first makes the library bind to that same HIP runtime
    # instance (same SONAME), which it must share with torch's allocator and streams.  Loaded the other way
    # round the process ends up with two runtimes and the library sees "no ROCm-capable device".
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().mudpt_last_error().decode(errors="replace")
        kind = {1: "bad argument", 2: "HIP error", 3: "bad state"}.get(rc, f"error {rc}")
        if rc == 1:
            raise AssertionError(f"mudpt {what}: {msg}")  # the reference asserts on bad cfg (trainers/mudpt.py:52,55,190)
        raise MudptError(f"mudpt {what}: {kind}: {msg}")


def call(name, **kw):
    """Call export `name` with the header's parameter names and return its code, unchecked.  A torch tensor passes its data_ptr(); None or
    an omitted pointer is null (`stream`: the null stream), an omitted scalar 0."""
    params = DECLARATIONS[name][1]
    unknown = sorted(set(kw) - {n for n, _ in params})
    if unknown:
        raise TypeError(f"{name} has no parameter {', '.join(unknown)}")
    args = []
    for n, t in params:
        v, pointer = kw.get(n), t in (C.c_void_p, C.c_char_p)
        if hasattr(v, "data_ptr"):
            if not pointer:
                raise TypeError(f"{name}: a tensor for the scalar parameter {n}")
            v = v.data_ptr()
        args.append(0 if v is None and not pointer else v)
    return getattr(load(), name)(*args)


class _DeviceMemory:
    """fp32 device memory the library owns, exposed through the CUDA array interface (no copy, no ownership)."""

    def __init__(self, address: int, numel: int):
        self.__cuda_array_interface__ = {"shape": (numel,), "typestr": "<f4", "data": (address, False), "version": 2}


def device_view(address: int, numel: int, device):
    """torch view (fp32, flat) of library-owned device memory: the operand of a torch.distributed collective."""
    import torch
    t = torch.as_tensor(_DeviceMemory(address, numel), device=device)
    if t.data_ptr() != address:
        raise MudptError("device_view: torch copied the buffer instead of aliasing it")
    return t


def ptr(t):
    """Device / host pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())
