"""Drop-in ``ZeroshotCLIP`` and ``ZeroshotCLIP2`` plugins -- the reference's ``trainers/zsclip.py:51-118`` -- and ``FrozenCLIP``, the module
they run on: CLIP as it was trained, nothing to learn, over a frozen handle of libmudpt_hip.so (``mudpt_create_frozen``; with a ResNet image
tower -- RN50, RN101, RN50x16, RN50x64 -- ``mudpt_create_frozen_resnet``).

The class prompts reach the library as token ids ``[T, C, ctx_len]``, one set per prompt template; the token embedding is looked up on the
device, the text tower runs once per template, and the text features -- ``f / |f|`` for one template (zsclip.py:67-71),
``normalise(mean_t normalise(f_t))`` for an ensemble (zsclip.py:107-117) -- are computed at the first forward and kept.  ``encode_image``
returns the raw ``visual(image)`` features the reference's linear-probe extractor reads (lpclip/feat_extractor.py:125; lpclip.py here).

The two template tables below restate the reference's data (trainers/zsclip.py:32-48, trainers/imagenet_templates.py:84-92), as
``dassl_lite.default_cfg`` restates train.py's defaults; tests/golden/zsclip_templates.json holds them to the reference's.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, List, Optional

import torch

from . import capi
from .model import LibraryModel, ModelShape
from .trainer import TRAINER_REGISTRY, TrainerX, install_test_loader, open_backbone, precision_to_dtype, tokenize_prompts, warn_if_fp16_misses_the_bound

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


class FrozenCLIP(LibraryModel):
    """Frozen CLIP over ``mudpt_create_frozen``: owns no parameter.  ``tokens`` [T, C, ctx_len] (or [C, ctx_len] for one template) are the
    tokenized prompts of every template and class; ``clip_state`` the OpenAI CLIP state dict ("token_embedding.weight" included: the
    library keeps it on the device)."""

    def __init__(self, shape: ModelShape, clip_state: Dict[str, torch.Tensor], tokens: torch.Tensor, max_batch: int = 100, dtype: str = "fp16",
                 device: str = "cuda:0", knobs: Optional[Dict[str, int]] = None, rn_fused_conv: Optional[bool] = None):
        tokens = torch.as_tensor(tokens)
        if tokens.dim() == 2:
            tokens = tokens[None]
        assert tokens.dim() == 3 and tokens.shape[2] == shape.ctx_len, f"tokens must be [T, C, {shape.ctx_len}], got {tuple(tokens.shape)}"
        def create(lib, cfg, h):
            if shape.resnet:  # clip/model.py:686-694: a checkpoint without "visual.proj" carries the ResNet image tower
                rn = capi.ResnetShape(*shape.v_stages, shape.v_width, shape.v_heads)
                capi.check(lib.mudpt_create_frozen_resnet(cfg, C.byref(rn), h), "create_frozen_resnet")
            else:
                capi.check(lib.mudpt_create_frozen(cfg, h), "create_frozen")

        # the knobs go in before the tokens: the layout knobs are read by mudpt_set_text_tokens
        super().__init__(shape, tokens.shape[1], max_batch, dtype, device, knobs, create, rn_fused_conv=rn_fused_conv, frozen=True)
        self.tokens = tokens.to("cpu", torch.int32).contiguous()
        self.n_templates = int(tokens.shape[0])
        for k, v in clip_state.items():  # clip/model.py:919 load_state_dict
            if isinstance(v, torch.Tensor) and v.is_floating_point():  # not BatchNorm's num_batches_tracked, nor a JIT archive's integer attributes
                self.set_weight(k, v)
        if tokens.numel():  # no tokens: encode_image alone (the linear-probe extractor)
            self.set_tokens(self.tokens)

    def set_tokens(self, tokens: torch.Tensor):
        tokens = torch.as_tensor(tokens)
        tokens = (tokens[None] if tokens.dim() == 2 else tokens).to("cpu", torch.int32).contiguous()
        assert tokens.dim() == 3 and tuple(tokens.shape[1:]) == (self.n_cls, self.shape.ctx_len), \
            f"tokens must be [T, {self.n_cls}, {self.shape.ctx_len}], got {tuple(tokens.shape)}"
        capi.check(self.lib.mudpt_set_text_tokens(self._h, capi.ptr(tokens), int(tokens.shape[0])), "set_text_tokens")
        self.tokens, self.n_templates = tokens, int(tokens.shape[0])

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """zsclip.py:74-79 model_inference: logits [B, n_cls]."""
        self._check_images(image)
        return self._infer(image, self.n_cls, lambda x, B, out, stream: capi.check(self.lib.mudpt_forward(self._h, x, B, out, stream), "forward"))

    def forward_features(self, feat: torch.Tensor) -> torch.Tensor:
        """model_inference behind ``clip_model.visual(image)`` (zsclip.py:76-79): logits [B, n_cls] of the raw image features ``feat``
        [B, embed_dim] -- ``encode_image`` / ``image_features()`` here, the rows lpclip/feat_extractor.py:125-137 saves.  Bit for bit the logits
        of the image forward the features came from; needs no ``visual.*`` weight."""
        self._check_features(feat)
        return self._infer(feat, self.n_cls, lambda x, B, out, stream: capi.check(
            self.lib.mudpt_forward_features(self._h, x, B, out, 0, stream), "forward_features"))

    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        """clip/model.py:822: the raw (un-normalised) image features [B, embed_dim]."""
        self._check_images(image)
        return self._infer(image, self.shape.embed_dim, lambda x, B, out, stream: capi.check(
            self.lib.mudpt_encode_image(self._h, x, B, out, stream), "encode_image"))

    def text_features(self) -> torch.Tensor:
        """The ensembled, normalised text features [n_cls, embed_dim] (zsclip.py:71,117)."""
        feat = torch.empty(self.n_cls, self.shape.embed_dim, dtype=torch.float32, device=self.device)
        capi.check(self.lib.mudpt_text_features(self._h, capi.ptr(feat), self._stream()), "text_features")
        return feat


@TRAINER_REGISTRY.register()
class ZeroshotCLIP(TrainerX):
    """trainers/zsclip.py:51-79: one prompt per class from the dataset's template.  No optimizer, no registered model, no training step."""

    def templates_for(self, dataset_name: str) -> List[str]:
        return [CUSTOM_TEMPLATES[dataset_name]]  # an unknown dataset: KeyError, as zsclip.py:61

    def build_model(self):
        cfg = self.cfg
        classnames = self.dm.dataset.classnames
        backbone, state = open_backbone(cfg)
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
        self.model = FrozenCLIP(dataclasses.replace(backbone, n_ctx=0, depth=1), state, tokens, max_batch=cfg.DATALOADER.TEST.BATCH_SIZE, dtype=precision_to_dtype(prec), device=device)

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
