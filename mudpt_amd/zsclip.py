"""Drop-in ``ZeroshotCLIP`` and ``ZeroshotCLIP2`` plugins -- the reference's ``trainers/zsclip.py:51-118`` -- and ``FrozenCLIP``, the module
they run on: CLIP as it was trained, nothing to learn, over a frozen handle of libmudpt_hip.so (``mudpt_create_frozen``).

The class prompts reach the library as token ids ``[T, C, ctx_len]``, one set per prompt template; the token embedding is looked up on the
device, the text tower runs once per template, and the text features -- ``f / |f|`` for one template (zsclip.py:67-71),
``normalise(mean_t normalise(f_t))`` for an ensemble (zsclip.py:107-117) -- are computed at the first forward and kept.  ``encode_image``
returns the raw ``visual(image)`` features the reference's linear-probe extractor reads (lpclip/feat_extractor.py:125; lpclip.py here).

The two template tables below restate the reference's data (trainers/zsclip.py:32-48, trainers/imagenet_templates.py:84-92), as
``dassl_lite.default_cfg`` restates train.py's defaults; tests/golden/zsclip_templates.json holds them to the reference's.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import nn

from . import capi, synth
from .model import ModelShape, check_features, read_image_features
from .trainer import TRAINER_REGISTRY, TrainerX, install_test_loader, load_clip_state_dict, precision_to_dtype, tokenize_prompts, warn_if_fp16_misses_the_bound

# trainers/zsclip.py:32-48: the per-dataset prompt, keyed by cfg.DATASET.NAME
CUSTOM_TEMPLATES = {
    "OxfordPets": "a photo of a {}, a type of pet.",
    "OxfordFlowers": "a photo of a {}, a type of flower.",
    "FGVCAircraft": "a photo of a {}, a type of aircraft.",
    "DescribableTextures": "{} texture.",
    "EuroSAT": "a centered satellite photo of {}.",
    "StanfordCars": "a photo of a {}.",
    "Food101": "a photo of {}, a type of food.",
    "SUN397": "a photo of a {}.",
    "Caltech101": "a photo of a {}.",
    "UCF101": "a photo of a person doing {}.",
    "ImageNet": "a photo of a {}.",
    "ImageNetSketch": "a photo of a {}.",
    "ImageNetV2": "a photo of a {}.",
    "ImageNetA": "a photo of a {}.",
    "ImageNetR": "a photo of a {}.",
}

# trainers/imagenet_templates.py:84-92: the seven templates ZeroshotCLIP2 ensembles (zsclip.py:87)
IMAGENET_TEMPLATES_SELECT = (
    "itap of a {}.",
    "a bad photo of the {}.",
    "a origami {}.",
    "a photo of the large {}.",
    "a {} in a video game.",
    "art of the {}.",
    "a photo of the small {}.",
)


def prompt_strings(template: str, classnames) -> List[str]:
    """zsclip.py:62,109: the template formatted with every class name, "_" replaced by a space."""
    return [template.format(c.replace("_", " ")) for c in classnames]


def ensemble_templates(dataset_name: str) -> List[str]:
    """zsclip.py:100-102: the seven selected ImageNet templates and, for every dataset but "ImageNet", the dataset's own."""
    templates = list(IMAGENET_TEMPLATES_SELECT)
    if dataset_name != "ImageNet":
        templates.append(CUSTOM_TEMPLATES[dataset_name])
    return templates


class FrozenCLIP(nn.Module):
    """Frozen CLIP over ``mudpt_create_frozen``: owns no parameter.  ``tokens`` [T, C, ctx_len] (or [C, ctx_len] for one template) are the
    tokenized prompts of every template and class; ``clip_state`` the OpenAI CLIP state dict ("token_embedding.weight" included: the
    library keeps it on the device)."""

    def __init__(self, shape: ModelShape, clip_state: Dict[str, torch.Tensor], tokens: torch.Tensor, max_batch: int = 100, dtype: str = "fp16",
                 device: str = "cuda:0", knobs: Optional[Dict[str, int]] = None):
        super().__init__()
        if not torch.cuda.is_available():
            raise capi.MudptError("mudpt_amd needs an MI355X (HIP device); there is no CPU path in the product")
        self.lib = capi.load()
        self.shape = shape
        self.device = torch.device(device)
        self.dtype_name = dtype
        tokens = torch.as_tensor(tokens)
        if tokens.dim() == 2:
            tokens = tokens[None]
        assert tokens.dim() == 3 and tokens.shape[2] == shape.ctx_len, f"tokens must be [T, C, {shape.ctx_len}], got {tuple(tokens.shape)}"
        self.tokens = tokens.to("cpu", torch.int32).contiguous()
        self.n_templates, self.n_cls = int(tokens.shape[0]), int(tokens.shape[1])
        self.max_batch = int(max_batch)
        cfg = capi.Config(shape.image_size, shape.patch, shape.v_width, shape.v_layers, shape.v_heads, shape.t_width, shape.t_layers,
                          shape.t_heads, shape.ctx_len, shape.embed_dim, 0, 1, self.n_cls, self.max_batch,
                          {"bf16": capi.BF16, "fp16": capi.F16, "fp32": capi.F32}[dtype], 0)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        capi.check(self.lib.mudpt_create_frozen(C.byref(cfg), C.byref(h)), "create_frozen")
        self._h = h
        for name, value in (knobs or {}).items():  # before the tokens: the layout knobs are read by mudpt_set_text_tokens
            self.set_knob(name, value)
        for k, v in clip_state.items():  # clip/model.py:919 load_state_dict
            if isinstance(v, torch.Tensor):
                self.set_weight(k, v)
        if tokens.numel():  # no tokens: encode_image alone (the linear-probe extractor)
            self.set_tokens(self.tokens)

    def set_weight(self, key: str, value: torch.Tensor):
        t = value.detach().to("cpu", torch.float32).contiguous()
        capi.check(self.lib.mudpt_set_weight(self._h, key.encode(), capi.ptr(t), t.numel()), f"set_weight({key})")

    def set_tokens(self, tokens: torch.Tensor):
        tokens = torch.as_tensor(tokens)
        tokens = (tokens[None] if tokens.dim() == 2 else tokens).to("cpu", torch.int32).contiguous()
        assert tokens.dim() == 3 and tuple(tokens.shape[1:]) == (self.n_cls, self.shape.ctx_len), \
            f"tokens must be [T, {self.n_cls}, {self.shape.ctx_len}], got {tuple(tokens.shape)}"
        capi.check(self.lib.mudpt_set_text_tokens(self._h, capi.ptr(tokens), int(tokens.shape[0])), "set_text_tokens")
        self.tokens, self.n_templates = tokens, int(tokens.shape[0])

    def set_knob(self, name: str, value: int):
        capi.check(self.lib.mudpt_model_set(self._h, name.encode(), int(value)), f"model_set({name})")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_images(self, image: torch.Tensor):
        S = self.shape.image_size
        # the library is told only B: a wrong-sized batch would make the patch gather read out of bounds
        assert image.dim() == 4 and tuple(image.shape[1:]) == (3, S, S), f"images must be [B, 3, {S}, {S}], got {tuple(image.shape)}"
        assert 0 < image.shape[0] <= self.max_batch, f"batch {image.shape[0]} outside 1..max_batch={self.max_batch}"

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """zsclip.py:74-79 model_inference: logits [B, n_cls]."""
        self._check_images(image)
        image = image.to(self.device, torch.float32).contiguous()
        logits = torch.empty(image.shape[0], self.n_cls, dtype=torch.float32, device=self.device)
        capi.check(self.lib.mudpt_forward(self._h, capi.ptr(image), image.shape[0], capi.ptr(logits), self._stream()), "forward")
        self._last_batch = image.shape[0]
        return logits

    def forward_features(self, feat: torch.Tensor) -> torch.Tensor:
        """model_inference behind ``clip_model.visual(image)`` (zsclip.py:76-79): logits [B, n_cls] of the raw image features ``feat``
        [B, embed_dim] -- ``encode_image`` / ``image_features()`` here, the rows lpclip/feat_extractor.py:125-137 saves.  Bit for bit the logits
        of the image forward the features came from; needs no ``visual.*`` weight."""
        check_features(feat, self.shape.embed_dim, self.max_batch)
        feat = feat.to(self.device, torch.float32).contiguous()
        logits = torch.empty(feat.shape[0], self.n_cls, dtype=torch.float32, device=self.device)
        capi.check(self.lib.mudpt_forward_features(self._h, capi.ptr(feat), feat.shape[0], capi.ptr(logits), 0, self._stream()), "forward_features")
        self._last_batch = feat.shape[0]
        return logits

    def image_features(self) -> torch.Tensor:
        """The raw ``clip_model.visual(image)`` features [B, embed_dim] of the last ``forward`` / ``forward_features`` / ``encode_image``."""
        return read_image_features(self)

    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        """clip/model.py:822: the raw (un-normalised) image features [B, embed_dim]."""
        self._check_images(image)
        image = image.to(self.device, torch.float32).contiguous()
        feat = torch.empty(image.shape[0], self.shape.embed_dim, dtype=torch.float32, device=self.device)
        capi.check(self.lib.mudpt_encode_image(self._h, capi.ptr(image), image.shape[0], capi.ptr(feat), self._stream()), "encode_image")
        self._last_batch = image.shape[0]
        return feat

    def text_features(self) -> torch.Tensor:
        """The ensembled, normalised text features [n_cls, embed_dim] (zsclip.py:71,117)."""
        feat = torch.empty(self.n_cls, self.shape.embed_dim, dtype=torch.float32, device=self.device)
        capi.check(self.lib.mudpt_text_features(self._h, capi.ptr(feat), self._stream()), "text_features")
        return feat

    def text_layout(self):
        """(token rows summed over the templates, largest bucket count of a template, longest kept length) (``mudpt_text_layout``)."""
        r, b, l = C.c_int32(), C.c_int32(), C.c_int32()
        capi.check(self.lib.mudpt_text_layout(self._h, C.byref(r), C.byref(b), C.byref(l)), "text_layout")
        return r.value, b.value, l.value

    def debug_read(self, name: str, batch: int = 1) -> torch.Tensor:
        """Flat fp32 host copy of "image_features", "text_features" or "text_launches" (test hook, see include/mudpt.h)."""
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


@TRAINER_REGISTRY.register()
class ZeroshotCLIP(TrainerX):
    """trainers/zsclip.py:51-79: one prompt per class from the dataset's template.  No optimizer, no registered model, no training step."""

    def templates_for(self, dataset_name: str) -> List[str]:
        return [CUSTOM_TEMPLATES[dataset_name]]  # an unknown dataset: KeyError, as zsclip.py:61

    def build_model(self):
        cfg = self.cfg
        classnames = self.dm.dataset.classnames
        print(f"Loading CLIP (backbone: {cfg.MODEL.BACKBONE.NAME})")
        state = load_clip_state_dict(cfg)
        if state is None:
            backbone = ModelShape()
            state = synth.random_clip_state(backbone, cfg.MODEL.BACKBONE.SYNTHETIC_SEED)
        else:
            backbone = ModelShape.from_state_dict(state, 0, 1)
        templates = self.templates_for(cfg.DATASET.NAME)
        if len(templates) > 1:
            print(f"Prompt ensembling (n={len(templates)})")  # zsclip.py:104-105
        node = getattr(cfg.TRAINER, "ZSCLIP", None)  # the reference has no such node: its GPU run is clip.load's fp16 model
        prec = node.PREC if node is not None and "PREC" in node else "fp16"
        warn_if_fp16_misses_the_bound(prec, state)
        near = cfg.MODEL.BACKBONE.PATH or None
        tokens = torch.stack([tokenize_prompts(prompt_strings(t, classnames), backbone.ctx_len, near=near) for t in templates])
        device = f"cuda:{self.device.index or 0}" if self.device.type == "cuda" else "cuda:0"
        self.templates = templates
        self.model = FrozenCLIP(backbone, state, tokens, max_batch=cfg.DATALOADER.TEST.BATCH_SIZE, dtype=precision_to_dtype(prec), device=device)

    def model_inference(self, image):
        return self.model(image)

    def test(self, split=None):
        from . import featcache
        install_test_loader(self, self.model.device.index or 0)  # the opt-in device-resident test pass (MUDPT_DEVICE_TEST=1 / device_test_store)
        return featcache.run_test(self, split, super().test)  # MUDPT_TEST_FEATURES=<dir> / trainer.test_features: from cached image features


@TRAINER_REGISTRY.register()
class ZeroshotCLIP2(ZeroshotCLIP):
    """Prompt ensembling (trainers/zsclip.py:82-118): the seven selected ImageNet templates plus, except for "ImageNet", the dataset's own.

    The reference appends the dataset's template to the CLASS-level list in place (zsclip.py:101-102), so a second ``build_model`` in one
    process ensembles 9 templates, a third 10.  Here the intended list -- 7 or 8 -- is built per instance, every time."""

    def templates_for(self, dataset_name: str) -> List[str]:
        return ensemble_templates(dataset_name)
