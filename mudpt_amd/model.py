"""Host-side mirror of the reference's ``CustomCLIP`` (trainers/mudpt.py:159-184) over libmudpt_hip.so.

``CustomCLIP`` here is an ``nn.Module`` whose ONLY tensors are the 10 trainable ones, registered under the
reference's state-dict names (``mudpt_prompt_learner.ctx`` ... ``image_encoder.visual_ctx_deep_projections.bias``,
trainers/mudpt.py:205-218) as views of one flat fp32 bucket, so a torch / Dassl optimizer, ``state_dict()``
and the reference's ``load_model`` (``strict=False``) work unchanged.  The frozen CLIP weights live inside
the library in its own HBM layout.  torch supplies device memory and streams only.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import nn

from . import capi


@dataclass(frozen=True)
class ModelShape:
    """Dimensions the reference infers from the checkpoint (clip/model.py:885-904) plus the prompt config."""
    image_size: int = 224
    patch: int = 16
    v_width: int = 768
    v_layers: int = 12
    v_heads: int = 12
    t_width: int = 512
    t_layers: int = 12
    t_heads: int = 8
    ctx_len: int = 77
    embed_dim: int = 512
    n_ctx: int = 4
    depth: int = 12
    # CLIP's ResNet image tower (clip/model.py:101-161): the Bottleneck blocks of its four stages; () = a ViT.  Then v_width is the tower's
    # `width` (64 for RN50), v_heads the attention pool's heads (32 width / 64), v_layers the blocks in all and patch its stride, 32
    v_stages: Tuple[int, ...] = ()

    @property
    def resnet(self) -> bool:
        return len(self.v_stages) > 0

    @staticmethod
    def from_state_dict(sd: Dict[str, torch.Tensor], n_ctx: int, depth: int) -> "ModelShape":
        """Same inference rules as clip/model.py:881-904 build_model: the ViT branch, or -- without "visual.proj" -- the ResNet branch (:890-897)."""
        if "visual.proj" not in sd:
            stages = tuple(len(set(k.split(".")[2] for k in sd if k.startswith(f"visual.layer{b}."))) for b in (1, 2, 3, 4))
            width = sd["visual.layer1.0.conv1.weight"].shape[0]
            grid = round((sd["visual.attnpool.positional_embedding"].shape[0] - 1) ** 0.5)
            assert grid ** 2 + 1 == sd["visual.attnpool.positional_embedding"].shape[0]
            t_width = sd["ln_final.weight"].shape[0]
            return ModelShape(image_size=32 * grid, patch=32, v_width=width, v_layers=sum(stages), v_heads=width * 32 // 64, t_width=t_width,
                              t_layers=len(set(k.split(".")[2] for k in sd if k.startswith("transformer.resblocks"))), t_heads=t_width // 64,
                              ctx_len=sd["positional_embedding"].shape[0], embed_dim=sd["text_projection"].shape[1], n_ctx=n_ctx, depth=depth,
                              v_stages=stages)
        v_width = sd["visual.conv1.weight"].shape[0]
        v_layers = len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
        patch = sd["visual.conv1.weight"].shape[-1]
        grid = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
        t_width = sd["ln_final.weight"].shape[0]
        t_layers = len(set(k.split(".")[2] for k in sd if k.startswith("transformer.resblocks")))
        return ModelShape(image_size=patch * grid, patch=patch, v_width=v_width, v_layers=v_layers, v_heads=v_width // 64,
                          t_width=t_width, t_layers=t_layers, t_heads=t_width // 64,
                          ctx_len=sd["positional_embedding"].shape[0], embed_dim=sd["text_projection"].shape[1],
                          n_ctx=n_ctx, depth=depth)

    @staticmethod
    def from_config(cfg, n_ctx: int, depth: int) -> "ModelShape":
        """The backbone dimensions of ``cfg`` -- any object with this class's backbone fields -- with the prompt config given here: a
        variant decides its own n_ctx / depth."""
        return ModelShape(**{f: getattr(cfg, f) for f in ModelShape.__dataclass_fields__ if f not in ("n_ctx", "depth", "v_stages")}, n_ctx=n_ctx, depth=depth,
                          v_stages=tuple(getattr(cfg, "v_stages", ())))


def umudpt_init_tensors(n_ctx: int, depth: int, d_t: int, d_v: int, ctx_rows: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Initial values of UMuDPT's 20 trainables, drawn as the reference draws them (trainers/umudpt.py:96-124): the same torch modules
    constructed on the CPU in the same order -- ctx (the CTX_INIT rows, or normal_(std=0.02)), deep_prompts normal_(std=0.02), ln_pre, the
    block's nn.MultiheadAttention, ln_1, c_fc, c_proj, ln_2, ln_post, visual_proj -- so that under one torch.manual_seed the draws equal
    the reference's.  Keys carry no prefix ("ctx", "self_attn.attn.in_proj_weight", ...), in named_parameters() order."""
    from collections import OrderedDict
    if ctx_rows is None:
        ctx = torch.empty(n_ctx, d_t)
        nn.init.normal_(ctx, std=0.02)
    else:
        ctx = ctx_rows.detach().to(torch.float32).clone()
    deep = torch.empty(depth - 1, n_ctx, d_t)
    nn.init.normal_(deep, std=0.02)
    ln_pre = nn.LayerNorm(d_t)
    block = nn.Module()
    block.attn = nn.MultiheadAttention(d_t, d_t // 64)
    block.ln_1 = nn.LayerNorm(d_t)
    block.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_t, d_t * 4)), ("c_proj", nn.Linear(d_t * 4, d_t))]))
    block.ln_2 = nn.LayerNorm(d_t)
    ln_post = nn.LayerNorm(d_t)
    visual_proj = nn.Linear(d_t, d_v)
    out = OrderedDict([("ctx", ctx), ("deep_prompts", deep)])
    for prefix, mod in (("ln_pre", ln_pre), ("self_attn", block), ("ln_post", ln_post), ("visual_proj", visual_proj)):
        for k, v in mod.named_parameters():
            out[prefix + "." + k] = v.detach()
    return out


def uumudpt_init_tensors(n_ctx: int, depth: int, d_t: int, d_v: int, embed_dim: int, image_size: int, patch: int, seed: Optional[int] = None,
                         ctx_rows: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Initial values of UUMuDPT's 40 trainables under their full keys, in named_parameters() order.  The reference draws them at TWO points:
    the vision tower's 20 when ``CLIP(...)`` is constructed (clip/model.py:605-623 -- ``visual`` is the first thing CLIP builds, and conv1,
    class_embedding and positional_embedding draw before visual_ctx, so they are drawn and dropped here), the prompt learner's 20 when
    ``CustomCLIP(...)`` is constructed (trainers/uumudpt.py:97-125, the draws of :func:`umudpt_init_tensors`).  ``seed``: each half is drawn
    right behind its own ``torch.manual_seed(seed)`` -- the two seed points the fixtures' checksums pin; None: both halves continue the
    caller's stream, the vision half first, as one process that builds CLIP and then CustomCLIP does."""
    from collections import OrderedDict
    if seed is not None:
        torch.manual_seed(seed)
    nn.Conv2d(3, d_v, patch, patch, bias=False)
    torch.randn(d_v)
    torch.randn((image_size // patch) ** 2 + 1, d_v)
    vis = umudpt_init_tensors(n_ctx, depth, d_v, embed_dim)  # the same constructors in the same order at width d_v, output width embed_dim
    if seed is not None:
        torch.manual_seed(seed)
    out = OrderedDict(("uumudpt_prompt_learner." + k, v) for k, v in umudpt_init_tensors(n_ctx, depth, d_t, d_v, ctx_rows).items())
    names = {"ctx": "", "deep_prompts": "_deep_prompts", "ln_pre": "_ln_intra_pre", "self_attn": "_self_attn", "ln_post": "_ln_intra_post",
             "visual_proj": "_text_proj"}
    for k, v in vis.items():
        head, _, rest = k.partition(".")
        out["image_encoder.visual_ctx" + names[head] + ("." + rest if rest else "")] = v
    return out


DTYPES = {"bf16": capi.BF16, "fp16": capi.F16, "fp32": capi.F32}  # F32: the parity mode
VARIANTS = {"mudpt": capi.VARIANT_MUDPT, "cocoop": capi.VARIANT_COCOOP, "coop": capi.VARIANT_COOP, "coop_csc": capi.VARIANT_COOP_CSC,
            "vpt": capi.VARIANT_VPT, "mpt": capi.VARIANT_MPT, "umudpt": capi.VARIANT_UMUDPT, "uumudpt": capi.VARIANT_UUMUDPT}


def library_config(shape: ModelShape, n_cls: int, max_batch: int, dtype: str, variant: str = "mudpt", frozen: bool = False) -> capi.Config:
    """The ``mudpt_config`` of a handle.  ``frozen``: a ``mudpt_create_frozen`` handle has no prompts and no variant (n_ctx 0, depth 1,
    variant 0).  An unknown ``dtype`` or ``variant`` name is a KeyError."""
    n_ctx, depth, code = (0, 1, 0) if frozen else (shape.n_ctx, shape.depth, VARIANTS[variant])
    return capi.Config(shape.image_size, shape.patch, shape.v_width, shape.v_layers, shape.v_heads, shape.t_width, shape.t_layers,
                       shape.t_heads, shape.ctx_len, shape.embed_dim, n_ctx, depth, int(n_cls), int(max_batch), DTYPES[dtype], code)


class LibraryModel(nn.Module):
    """An ``nn.Module`` that owns one ``mudpt_model*``: everything about the handle that does not depend on what it computes.  ``create(lib,
    cfg, h)`` is the subclass's create call (``mudpt_create`` / ``mudpt_create_ex`` / ``mudpt_create_resnet`` / ``mudpt_create_frozen``) on byref(config) and
    byref(handle); ``config`` are ``library_config``'s keywords.  The knobs are applied right behind it, before any weight or token."""

    def __init__(self, shape: ModelShape, n_cls: int, max_batch: int, dtype: str, device: str, knobs: Optional[Dict[str, int]], create,
                 rn_fused_conv: Optional[bool] = None, **config):
        super().__init__()
        if not torch.cuda.is_available():
            raise capi.MudptError("mudpt_amd needs an MI355X (HIP device); there is no CPU path in the product")
        self.lib = capi.load()
        self.shape = shape
        self.device = torch.device(device)
        self.dtype_name = dtype
        self.n_cls = int(n_cls)
        self.max_batch = int(max_batch)
        cfg = library_config(shape, self.n_cls, self.max_batch, dtype, **config)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        create(self.lib, C.byref(cfg), C.byref(h))
        self._h = h
        self._last_batch = 0  # images of the last inference forward, whose raw features the library still holds (image_features)
        for name, value in (knobs or {}).items():  # per-handle tuning knobs (mudpt_model_set): A/B runs and tests
            self.set_knob(name, value)
        # opt-in: a ResNet tower's convolutions as one launch each (set_resnet_conv_path); None: MUDPT_RN_FUSED_CONV=1 on a ResNet shape
        if rn_fused_conv is None:
            rn_fused_conv = shape.resnet and os.environ.get("MUDPT_RN_FUSED_CONV") == "1"
        if rn_fused_conv:
            self.set_resnet_conv_path(1)

    def set_weight(self, key: str, value: torch.Tensor):
        """One frozen weight, by OpenAI CLIP key (clip/model.py:919 load_state_dict)."""
        t = value.detach().to("cpu", torch.float32).contiguous()
        capi.check(self.lib.mudpt_set_weight(self._h, key.encode(), capi.ptr(t), t.numel()), f"set_weight({key})")

    def set_resnet_conv_path(self, path: int):
        """``mudpt_resnet_conv_path``: 0 = every convolution of the ResNet tower as im2col + GEMM + bias_act (the default), 1 = as one
        ``mudpt_conv2d`` launch.  Between any two forwards; a handle without that tower is refused by the library."""
        capi.check(self.lib.mudpt_resnet_conv_path(self._h, int(path)), "resnet_conv_path")

    def set_knob(self, name: str, value: int):
        """``mudpt_model_set``: "gemm_variant", "lp_grad" and the split-operand knobs ("vis_lo", "txt_lo", "vis_sites", "txt_sites",
        "vis_exact_attn", "txt_exact_attn": include/mudpt.h MUDPT_F32) any time; "txt_trim" / "txt_buckets" only through
        ``knobs=`` at construction (before the class prompts or tokens are ingested)."""
        capi.check(self.lib.mudpt_model_set(self._h, name.encode(), int(value)), f"model_set({name})")

    def text_layout(self):
        """(token rows, length buckets, longest kept length) of one text-tower pass (``mudpt_text_layout``); a frozen handle: the rows summed
        over its templates, the largest bucket count of a template."""
        r, b, l = C.c_int32(), C.c_int32(), C.c_int32()
        capi.check(self.lib.mudpt_text_layout(self._h, C.byref(r), C.byref(b), C.byref(l)), "text_layout")
        return r.value, b.value, l.value

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_images(self, image: torch.Tensor):
        S = self.shape.image_size
        # the library is told only B: a wrong-sized batch would make the patch gather read out of bounds (trainers/mudpt.py:55 asserts
        # the configured size; this asserts the data)
        assert image.dim() == 4 and tuple(image.shape[1:]) == (3, S, S), f"images must be [B, 3, {S}, {S}], got {tuple(image.shape)}"
        assert 0 < image.shape[0] <= self.max_batch, f"batch {image.shape[0]} outside 1..max_batch={self.max_batch}"

    def _check_features(self, feat: torch.Tensor):
        """The library is told only B: features of another width would make the copy read out of bounds."""
        E = self.shape.embed_dim
        assert feat.dim() == 2 and feat.shape[1] == E, f"features must be [B, {E}], got {tuple(feat.shape)}"
        assert 0 < feat.shape[0] <= self.max_batch, f"batch {feat.shape[0]} outside 1..max_batch={self.max_batch}"

    def _infer(self, x: torch.Tensor, width: int, call) -> torch.Tensor:
        """One inference call on a checked batch ``x``: moved to the device as fp32, ``call(x, B, out, stream)`` on the pointers, fp32
        [B, width] back.  The library then holds the raw image features of these B rows."""
        x = x.to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        out = torch.empty(B, width, dtype=torch.float32, device=self.device)
        call(capi.ptr(x), B, capi.ptr(out), self._stream())
        self._last_batch = B
        return out

    def image_features(self) -> torch.Tensor:
        """``mudpt_image_features``: the raw ``clip_model.visual(image)`` features [B, embed_dim] of the last inference forward (``forward``,
        ``forward_features``, ``encode_image``), B as that forward had it.  Before any, B = 0 and the library answers with its bad state."""
        B = self._last_batch
        feat = torch.empty(max(B, 1), self.shape.embed_dim, dtype=torch.float32, device=self.device)
        capi.check(self.lib.mudpt_image_features(self._h, B, capi.ptr(feat), self._stream()), "image_features")
        return feat[:B]

    @torch.no_grad()
    def predict(self, image: torch.Tensor, k: int = 5):
        """CLIP's zero-shot recipe ``logits.softmax(-1).topk(k)`` on ``forward``'s logits: ``(prob [B, k] fp32, index [B, k] int64)`` from one
        more launch (``metrics.topk``).  Ties are ranked by the evaluator's order (lower index first), so two runs agree."""
        from . import metrics
        index, prob = metrics.topk(self.forward(image), k, probabilities=True)
        return prob, index

    def debug_read(self, name: str, batch: int = 1) -> torch.Tensor:
        """Flat fp32 host copy of an internal activation of the last call, "image_features", "text_features" or "text_launches" (test
        hook, see include/mudpt.h)."""
        n = C.c_size_t()
        capi.check(self.lib.mudpt_debug_read(self._h, name.encode(), batch, None, 0, C.byref(n)), "debug_read")
        out = torch.empty(n.value, dtype=torch.float32)
        capi.check(self.lib.mudpt_debug_read(self._h, name.encode(), batch, capi.ptr(out), n.value, C.byref(n)), "debug_read")
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            self.lib.mudpt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ClipOutputs(NamedTuple):
    """What ``CustomCLIP.differentiable`` returns: the logits and the RAW (un-normalised) features of both towers, fp32 on the device."""
    logits: torch.Tensor
    image_features: torch.Tensor
    text_features: torch.Tensor


def _forward_train(model, image, keep: bool):
    """``mudpt_forward_train`` + ``mudpt_train_features`` on a checked device batch: (logits, image features, text features, token).  keep:
    the forward stays in flight for a backward and ``token`` is its number (``mudpt_train_token``); else it is released and the token is 0."""
    B, E = image.shape[0], model.shape.embed_dim
    logits = torch.empty(B, model.n_cls, dtype=torch.float32, device=model.device)
    img_f = torch.empty(B, E, dtype=torch.float32, device=model.device)
    txt_f = torch.empty(model.n_cls, E, dtype=torch.float32, device=model.device)
    capi.check(model.lib.mudpt_forward_train(model._h, capi.ptr(image), B, capi.ptr(logits), model._stream()), "forward_train")
    capi.check(model.lib.mudpt_train_features(model._h, B, capi.ptr(img_f), capi.ptr(txt_f), model._stream()), "train_features")
    model._text_version, model._last_batch = model.flat_params._version, 0  # as forward_backward: this version's text features are in the library
    token = C.c_int64(0)
    if keep:
        capi.check(model.lib.mudpt_train_token(model._h, 0, C.byref(token)), "train_token")
    else:
        capi.check(model.lib.mudpt_train_release(model._h), "train_release")
    return logits, img_f, txt_f, token.value


class _DifferentiableStep(torch.autograd.Function):
    """The library's training step as one autograd node.  The trainables are no inputs of it: autograd's accumulator may REPLACE a
    parameter's ``.grad``, and every ``.grad`` here must stay its view of the flat bucket (the optimizer, the all-reduce and the step
    consensus read that bucket).  The backward therefore accumulates into the bucket as a side effect and returns None for the anchor."""

    @staticmethod
    def forward(ctx, model, image, grad_scale, anchor):
        ctx.model, ctx.batch, ctx.grad_scale = model, image.shape[0], grad_scale
        ctx.set_materialize_grads(False)  # an output the loss does not read arrives as None, and goes to the library as null
        *out, ctx.token = _forward_train(model, image, keep=True)
        return tuple(out)

    @staticmethod
    def backward(ctx, d_logits, d_img, d_txt):
        model = ctx.model
        given = [None if g is None else g.to(model.device, torch.float32).contiguous() for g in (d_logits, d_img, d_txt)]
        if all(g is None for g in given):
            return None, None, None, None
        # THIS node's forward must be the one in flight: a later forward of the same batch size would otherwise take these gradients
        capi.check(model.lib.mudpt_train_token(model._h, ctx.token, None), "backward_logits")
        before = model.flat_grads.clone()  # the library zeroes the bucket and writes this step's gradient; torch accumulates, so add it back
        try:
            capi.check(model.lib.mudpt_backward_logits(model._h, *(capi.ptr(g) for g in given), ctx.batch, ctx.grad_scale, model._stream()), "backward_logits")
        except BaseException:
            model.flat_grads.copy_(before)  # zeroed or not: the bucket is what it was
            raise
        model.flat_grads.add_(before)
        return None, None, None, None


class _Holder(nn.Module):
    """Namespace module so parameters get the reference's dotted state-dict keys."""


class CustomCLIP(LibraryModel):
    def __init__(self, shape: ModelShape, clip_state: Dict[str, torch.Tensor], tokenized_prompts: torch.Tensor,
                 ctx_token_ids: Optional[Sequence[int]] = None, max_batch: int = 256, dtype: str = "bf16",
                 device: str = "cuda:0", seed: Optional[int] = None, variant: str = "mudpt", knobs: Optional[Dict[str, int]] = None,
                 class_shard: Optional[Sequence[int]] = None, group=None, class_token_position: str = "end",
                 name_lens: Optional[Sequence[int]] = None, prompt_shape: Optional[Sequence[int]] = None):
        # "cocoop": the same library runs trainers/cocoop.py's CustomCLIP (vanilla vision tower, meta_net, one text-tower pass
        # per (image, class) pair); the module then owns ctx + meta_net under the reference's names (prompt_learner.*)
        # "coop" / "coop_csc": trainers/coop.py's CustomCLIP (vanilla vision tower, forward only; one trainable, prompt_learner.ctx, shared
        # [n_ctx, d_t] or one per class [n_cls, n_ctx, d_t]); class_token_position / name_lens: TRAINER.COOP.CLASS_TOKEN_POSITION and
        # len(_tokenizer.encode(name)) per class (coop.py:80), needed for "middle" / "front"
        # "vpt" / "mpt": trainers/vpt.py's / mpt.py's CustomCLIP (independent deep prompts per tower, every "visual_ctx" a trainable of its
        # own under the reference's key); prompt_shape = (DEEP_TEXT_N_CTX, TEXT_PROMPT_DEPTH, DEEP_VISUAL_N_CTX, VISUAL_PROMPT_DEPTH) of
        # TRAINER.VPT / TRAINER.MPT (include/mudpt.h mudpt_prompt_shape); shape.n_ctx / depth are not used.  MPT's ctx_token_ids: the
        # TEXT_CTX_INIT tokens that initialise text_prompt_learner.visual_ctx (trainers/mpt.py:55-62)
        # "umudpt": trainers/umudpt.py's CustomCLIP (MuDPT's towers; the vision prompts of every layer are generated from ctx / deep_prompts by a
        # trainable transformer block): 20 trainables under "umudpt_prompt_learner.*"; shape.n_ctx (1..16) / depth are TRAINER.UMUDPT.N_CTX /
        # DEEP_PROMPT_DEPTH
        # "uumudpt": trainers/uumudpt.py's CustomCLIP (UMuDPT plus the vision tower's own visual_ctx, visual_ctx_deep_prompts and a second
        # generator that turns those into an addend of the text deep prompts): 40 trainables, "uumudpt_prompt_learner.*" then
        # "image_encoder.visual_ctx*"; shape.n_ctx (1..16) / depth are TRAINER.UUMUDPT.N_CTX / DEEP_PROMPT_DEPTH
        # A ResNet ``shape`` (RN50, RN101, RN50x16, RN50x64): "coop" / "coop_csc" / "cocoop" only -- their image encoder is frozen and prompt-free
        # (trainers/coop.py:212-226, cocoop.py:178-198), so the tower runs forward only where the vanilla ViT would (mudpt_create_resnet).  Its
        # convolutions run fused (set_resnet_conv_path(1)) from construction on under MUDPT_RN_FUSED_CONV=1, or after that call at any time
        assert not shape.resnet or variant in ("coop", "coop_csc", "cocoop"), \
            "ResNet backbones run on the frozen handle only (ZeroshotCLIP, ZeroshotCLIP2, feature extraction)"
        if variant == "coop_csc" and ctx_token_ids is not None:
            variant = "coop"  # trainers/coop.py:52-61: the CTX_INIT path builds one shared context whatever CSC says
        assert (prompt_shape is not None) == (variant in ("vpt", "mpt")), "prompt_shape is the VPT / MPT setting, and they need it"
        prompt_shape = None if prompt_shape is None else tuple(int(v) for v in prompt_shape)

        def create(lib, cfg, h):
            if shape.resnet:
                capi.check(lib.mudpt_create_resnet(cfg, C.byref(capi.ResnetShape(*shape.v_stages, shape.v_width, shape.v_heads)), h), "create_resnet")
            elif prompt_shape is not None:
                capi.check(lib.mudpt_create_ex(cfg, C.byref(capi.PromptShape(*prompt_shape)), h), "create_ex")
            else:
                capi.check(lib.mudpt_create(cfg, h), "create")

        super().__init__(shape, tokenized_prompts.shape[0], max_batch, dtype, device, knobs, create, variant=variant)
        self.tokenized_prompts = tokenized_prompts.clone()
        self.variant, self.prompt_shape = variant, prompt_shape
        h = self._h
        for k, v in clip_state.items():  # the frozen weights; of the token embedding only the class prompts' rows go up (below)
            if k != "token_embedding.weight" and isinstance(v, torch.Tensor) and v.is_floating_point():  # not BatchNorm's num_batches_tracked
                self.set_weight(k, v)
        # class-parallel text tower (include/mudpt.h): this rank encodes classes [c0, c1) of the n_cls; ``group`` is the process group
        # of the two exchanges (None = the default group)
        self.class_shard, self.group = None, group
        if class_shard is not None and tuple(class_shard) != (0, self.n_cls):
            assert variant != "cocoop", "CoCoOp's text features depend on the image: shard the batch, not the classes"
            assert variant == "mudpt", "class-parallel CoOp is not implemented: shard the batch, not the classes"
            self.class_shard = (int(class_shard[0]), int(class_shard[1]))
            capi.check(self.lib.mudpt_set_class_shard(h, *self.class_shard), "set_class_shard")
        self.class_token_position = class_token_position
        if variant in ("coop", "coop_csc"):  # before the class prompts: they are reordered by it (trainers/coop.py:99-164)
            pos = {"end": capi.CLASS_TOKEN_END, "middle": capi.CLASS_TOKEN_MIDDLE, "front": capi.CLASS_TOKEN_FRONT}[class_token_position]
            lens = None if name_lens is None else torch.tensor([int(v) for v in name_lens], dtype=torch.int32)
            assert lens is None or lens.numel() == self.n_cls, f"name_lens has {lens.numel()} entries for {self.n_cls} classes"
            capi.check(self.lib.mudpt_set_class_token_position(h, pos, capi.ptr(lens)), "set_class_token_position")
        else:
            assert class_token_position == "end" and name_lens is None, "class_token_position / name_lens are CoOp settings"
        # class prompts: token_embedding(tokenized) and the EOT position (trainers/mudpt.py:85-90,154)
        emb_w = clip_state["token_embedding.weight"].detach().to("cpu", torch.float32)
        tok = tokenized_prompts.to("cpu").long()
        emb = emb_w[tok].contiguous()
        eot = tok.argmax(dim=-1).to(torch.int32).contiguous()
        capi.check(self.lib.mudpt_set_class_prompts(h, capi.ptr(emb), capi.ptr(eot)), "set_class_prompts")
        # the flat parameter / gradient buckets and the 10 named views
        total = self.lib.mudpt_param_numel(h)
        self.flat_params = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.flat_grads = torch.zeros(total, dtype=torch.float32, device=self.device)
        capi.check(self.lib.mudpt_bind_params(h, capi.ptr(self.flat_params), capi.ptr(self.flat_grads)), "bind_params")
        self.param_names = []
        for i in range(self.lib.mudpt_param_count(h)):
            name, off, numel, ndim, shp = C.c_char_p(), C.c_size_t(), C.c_size_t(), C.c_int32(), (C.c_int64 * 3)()
            capi.check(self.lib.mudpt_param_info(h, i, C.byref(name), C.byref(off), C.byref(numel), C.byref(ndim), C.byref(shp)))
            key = name.value.decode()
            view = self.flat_params[off.value:off.value + numel.value].view(*[int(shp[j]) for j in range(ndim.value)])
            p = nn.Parameter(view, requires_grad=True)
            p.grad = self.flat_grads[off.value:off.value + numel.value].view_as(view)
            mod = self
            *path, leaf = key.split(".")
            for part in path:  # namespace modules along the reference's dotted key
                if not hasattr(mod, part):
                    setattr(mod, part, _Holder())
                mod = getattr(mod, part)
            mod.register_parameter(leaf, p)
            self.param_names.append(key)
        self._init_trainables(emb_w, ctx_token_ids, seed)
        self._cp_feat = self._cp_dfeat = None
        if variant == "mudpt":  # the [n_cls, embed] text-feature table and its gradient (library-owned): operands of the class-parallel exchanges
            f, df, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
            capi.check(self.lib.mudpt_cp_buffers(h, C.byref(f), C.byref(df), C.byref(n)), "cp_buffers")
            self._cp_feat, self._cp_dfeat = (capi.device_view(q.value, n.value, self.device).view(self.n_cls, shape.embed_dim) for q in (f, df))
        self._loss = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._text_version = None  # flat_params._version the library's cached text features belong to
        self.loss_scale = 128.0    # the library's default (mudpt_set_loss_scale)

    # -- initialisation of the trainables, trainers/mudpt.py:57-81 and clip/model.py:512-519 ---------------------
    def _init_trainables(self, emb_w, ctx_token_ids, seed):
        sd = dict(self.named_parameters())
        if self.variant == "umudpt":
            s = self.shape
            with torch.random.fork_rng(devices=[], enabled=seed is not None):  # a seed: the reference's draws under torch.manual_seed(seed)
                if seed is not None:
                    torch.manual_seed(seed)
                init = umudpt_init_tensors(s.n_ctx, s.depth, s.t_width, s.v_width, None if ctx_token_ids is None else emb_w[list(ctx_token_ids)])
            with torch.no_grad():
                for k, v in init.items():
                    sd["umudpt_prompt_learner." + k].copy_(v)
            return
        if self.variant == "uumudpt":
            s = self.shape
            with torch.random.fork_rng(devices=[], enabled=seed is not None):
                init = uumudpt_init_tensors(s.n_ctx, s.depth, s.t_width, s.v_width, s.embed_dim, s.image_size, s.patch, seed,
                                            None if ctx_token_ids is None else emb_w[list(ctx_token_ids)])
            with torch.no_grad():
                for k, v in init.items():
                    sd[k].copy_(v)
            return
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        with torch.no_grad():
            for k, p in sd.items():
                if k.endswith(".weight") or k.endswith(".bias"):
                    fan_in = sd[k.rsplit(".", 1)[0] + ".weight"].shape[1]
                    v = (torch.rand(p.shape, generator=g) * 2 - 1) / math.sqrt(fan_in)  # nn.Linear default
                else:
                    v = 0.02 * torch.randn(p.shape, generator=g)  # nn.init.normal_(std=0.02)
                p.copy_(v)
            if ctx_token_ids is not None:  # CTX_INIT words -> their token embeddings
                sd[self.ctx_key].copy_(emb_w[list(ctx_token_ids)])

    @property
    def ctx_key(self) -> str:
        return {"mudpt": "mudpt_prompt_learner.ctx", "mpt": "text_prompt_learner.visual_ctx",
                "umudpt": "umudpt_prompt_learner.ctx", "uumudpt": "uumudpt_prompt_learner.ctx"}.get(self.variant, "prompt_learner.ctx")

    def set_params(self, tensors: Dict[str, torch.Tensor]):
        self._text_version = None
        with torch.no_grad():
            for k, p in self.named_parameters():
                if k in tensors:
                    p.copy_(tensors[k])

    def grads(self) -> Dict[str, torch.Tensor]:
        return {k: p.grad for k, p in self.named_parameters()}

    def invalidate_text_cache(self):
        """Parameters changed behind the bucket's version counter (``p.data`` writes, optimizers, the library's SGD): the next eval
        forward recomputes the text features."""
        self._text_version = None

    def load_state_dict(self, *args, **kwargs):
        self._text_version = None
        return super().load_state_dict(*args, **kwargs)

    def _text_reuse(self):
        """(reuse, version) of an eval forward: the text features only depend on the parameters, so they are recomputed only when the flat
        bucket's version counter moved (the reference re-runs the text tower for every test batch).  CoCoOp's depend on the image; VPT's on
        no trainable: the library keeps them itself (until a frozen weight changes)."""
        version = self.flat_params._version
        return (not self.training) and self._text_version == version and self.variant not in ("cocoop", "vpt"), version

    def forward_features(self, feat: torch.Tensor) -> torch.Tensor:
        """``forward`` behind ``clip_model.visual(image)`` (trainers/coop.py:214-223, cocoop.py:182-198), for the CoOp and CoCoOp variants:
        logits [B, n_cls] of the raw image features ``feat`` [B, embed_dim] -- what ``image_features()`` returns after a ``forward`` and what
        lpclip/feat_extractor.py:125-137 saves.  Bit for bit the logits of the image forward the features came from.  Any other variant:
        AssertionError (its trainable prompts run inside the vision tower)."""
        self._check_features(feat)
        reuse, version = self._text_reuse()
        logits = self._infer(feat, self.n_cls, lambda x, B, out, stream: capi.check(
            self.lib.mudpt_forward_features(self._h, x, B, out, 1 if reuse else 0, stream), "forward_features"))
        self._text_version = version
        return logits

    # -- trainers/mudpt.py:170-184 ---------------------------------------------------------------------------------
    def forward(self, image: torch.Tensor) -> torch.Tensor:
        self._check_images(image)
        reuse, version = self._text_reuse()

        def call(x, B, out, stream):
            if self.class_shard is not None:
                capi.check(self.lib.mudpt_cp_forward(self._h, x, B, 1 if reuse else 0, stream), "cp_forward")
                if not reuse:
                    self._exchange(self._cp_feat)
                capi.check(self.lib.mudpt_cp_head(self._h, None, B, 1.0, None, out, 1 if reuse else 0, stream), "cp_head")
            else:
                capi.check(self.lib.mudpt_forward_ex(self._h, x, B, out, 1 if reuse else 0, stream), "forward")

        logits = self._infer(image, self.n_cls, call)
        self._text_version = version
        return logits

    def _exchange(self, table: torch.Tensor, async_op: bool = False):
        """Sum of a [n_cls, embed] table over the ranks of the class-parallel group (rows of other ranks are zero in the feature table,
        so the sum is the gather, bit for bit, also for uneven shards)."""
        import torch.distributed as dist
        # only a class-SHARDED handle exchanges: on an unsharded one every rank holds the full table already, and summing world
        # identical copies would scale d(features) -- and with it every text-side gradient -- by world without any error
        if self.class_shard is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            return dist.all_reduce(table, group=self.group, async_op=async_op)
        return None

    def forward_backward_cp(self, image: torch.Tensor, label: torch.Tensor, grad_scale: float = 1.0, return_logits: bool = False):
        """The training step in class-parallel phases (include/mudpt.h): towers forward with this rank's classes -> sum of the feature
        table -> head over the local images and all classes -> sum of d(features), overlapped with the vision backward -> text backward
        over this rank's classes.  On an unsharded handle (every rank encodes all classes) the phases run without any exchange."""
        self._check_images(image)
        assert label.shape == (image.shape[0],), f"labels must be [B], got {tuple(label.shape)}"
        image = image.to(self.device, torch.float32).contiguous()
        label = label.to(self.device, torch.int64).contiguous()
        B = image.shape[0]
        logits = torch.empty(B, self.n_cls, dtype=torch.float32, device=self.device) if return_logits else None
        capi.check(self.lib.mudpt_cp_forward(self._h, capi.ptr(image), B, capi.FWD_TRAINING, self._stream()), "cp_forward")
        self._exchange(self._cp_feat)
        capi.check(self.lib.mudpt_cp_head(self._h, capi.ptr(label), B, grad_scale, capi.ptr(self._loss), capi.ptr(logits), 0, self._stream()), "cp_head")
        work = self._exchange(self._cp_dfeat, async_op=True)
        capi.check(self.lib.mudpt_cp_backward(self._h, capi.CP_VISION, self._stream()), "cp_backward(vision)")
        if work is not None:
            work.wait()  # the current stream waits for the collective; the host does not
        capi.check(self.lib.mudpt_cp_backward(self._h, capi.CP_TEXT, self._stream()), "cp_backward(text)")
        self._text_version, self._last_batch = self.flat_params._version, 0
        return (self._loss[0], logits) if return_logits else self._loss[0]

    # -- trainers/mudpt.py:249-251 minus the optimizer step: loss (device scalar) + .grad of the 10 tensors ---------------
    def forward_backward(self, image: torch.Tensor, label: torch.Tensor, grad_scale: float = 1.0,
                         return_logits: bool = False):
        if self.class_shard is not None:
            return self.forward_backward_cp(image, label, grad_scale, return_logits)
        self._check_images(image)
        assert label.shape == (image.shape[0],), f"labels must be [B], got {tuple(label.shape)}"
        image = image.to(self.device, torch.float32).contiguous()
        label = label.to(self.device, torch.int64).contiguous()
        B = image.shape[0]
        logits = torch.empty(B, self.n_cls, dtype=torch.float32, device=self.device) if return_logits else None
        capi.check(self.lib.mudpt_forward_backward(self._h, capi.ptr(image), capi.ptr(label), B, grad_scale,
                                                   capi.ptr(self._loss), capi.ptr(logits), self._stream()), "forward_backward")
        self._text_version, self._last_batch = self.flat_params._version, 0  # the step's forward left this version's text features in the library
        return (self._loss[0], logits) if return_logits else self._loss[0]

    # -- a loss of the caller's: the step split at the head (include/mudpt.h mudpt_forward_train / mudpt_backward_logits) -------------
    def differentiable(self, image: torch.Tensor, grad_scale: float = 1.0) -> "ClipOutputs":
        """The training forward as torch sees it: ``ClipOutputs(logits [B, n_cls], image_features [B, embed_dim], text_features [n_cls,
        embed_dim])`` -- the features RAW, as the towers leave them -- fp32 on the device, behind one ``torch.autograd.Function``.  Any torch
        loss of the three can be backpropagated with ``loss.backward()``: the library's backward then ADDS the gradient of ``grad_scale *
        loss`` to every trainable's ``.grad``, which stays the view of ``flat_grads`` it was.  One forward feeds one backward: a second
        ``backward`` through the same outputs, or one after another forward or step of this model, raises the library's bad-state error.
        Under ``torch.no_grad()`` the three tensors come back and nothing is armed for a backward.  CoCoOp, a class-sharded and a frozen
        handle are refused with the library's line."""
        self._check_images(image)
        image = image.to(self.device, torch.float32).contiguous()
        if not torch.is_grad_enabled():
            return ClipOutputs(*_forward_train(self, image, keep=False)[:3])
        if not hasattr(self, "_autograd_anchor"):  # what makes the outputs require grad; it never receives one (backward returns None for it)
            self._autograd_anchor = torch.zeros((), dtype=torch.float32, device=self.device, requires_grad=True)
        return ClipOutputs(*_DifferentiableStep.apply(self, image, float(grad_scale), self._autograd_anchor))

    def set_loss_scale(self, scale: float):
        """Static scale of the backward pass (include/mudpt.h mudpt_set_loss_scale; default 128 per sample); the trainer plugins move it
        like torch's GradScaler does (halve on overflow, grow back after a run of clean steps)."""
        capi.check(self.lib.mudpt_set_loss_scale(self._h, float(scale)), "set_loss_scale")
        self.loss_scale = float(scale)

    def sgd_step(self, lr: float, momentum: float = 0.9, weight_decay: float = 5e-4, dampening: float = 0.0, nesterov: bool = False):
        capi.check(self.lib.mudpt_sgd_step(self._h, lr, momentum, weight_decay, dampening, int(nesterov), self._stream()), "sgd_step")
        self._text_version = None  # the library wrote the parameters behind torch's version counter

    def profile(self, enable):
        """False / 0: off; True / 1: bracket the persistent GEMM launches only; an int > 1: bit mask of PROF_CLASSES (31 = all)."""
        capi.check(self.lib.mudpt_profile_enable(self._h, int(enable)), "profile_enable")

    def profile_read(self):
        """(summed GEMM ms, summed algorithmic GEMM FLOPs, launches) since the last enable / read."""
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        capi.check(self.lib.mudpt_profile_read(self._h, C.byref(ms), C.byref(fl), C.byref(n)), "profile_read")
        return ms.value, fl.value, n.value

    PROF_CLASSES = ("gemm_pp", "ln_fwd", "ln_bwd", "attn_fwd", "attn_bwd")

    def profile_read_classes(self):
        """({class: (ms, work, launches)}, executed MFMA FLOPs) since the last enable / read; work = algorithmic FLOPs for "gemm_pp",
        algorithmic HBM bytes for the LayerNorm / attention classes (vision tower launches only)."""
        ms, work, n, ex = (C.c_double * 5)(), (C.c_double * 5)(), (C.c_int64 * 5)(), C.c_double()
        capi.check(self.lib.mudpt_profile_read_classes(self._h, C.byref(ms), C.byref(work), C.byref(n), C.byref(ex)), "profile_read_classes")
        return {k: (ms[i], work[i], n[i]) for i, k in enumerate(self.PROF_CLASSES)}, ex.value
