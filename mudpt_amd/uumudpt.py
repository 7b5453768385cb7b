"""Drop-in ``UUMuDPT`` trainer plugin: the reference's ``trainers/uumudpt.py:236-352`` surface over libmudpt_hip.so.

UMuDPT with the coupling in both directions: besides the prompt learner's generator (text prompts -> vision prompts) the vision tower owns
``visual_ctx``, ``visual_ctx_deep_prompts`` and a second generator that turns its deep prompts into an addend of the text tower's deep prompts
(``VisionTransformer_UUMuDPT``, clip/model.py:600-664).  The module owns the reference's 40 trainables -- every parameter whose name contains
"prompt_learner" or "visual_ctx" (uumudpt.py:255-261) -- under its keys ``uumudpt_prompt_learner.*`` and ``image_encoder.visual_ctx*``, and the
whole model is registered as "UnifiedMultimodalDeepPromptTuning" (uumudpt.py:276), the name UMuDPT's carries too.  MODEL.INIT_WEIGHTS: as in
UMuDPT the reference reads ``self.model.prompt_learner``, which its model does not have (uumudpt.py:269-270); here the file is loaded into the
module that owns the tensors.
"""
from __future__ import annotations

from .trainer import TRAINER_REGISTRY, PromptTrainer
from .umudpt import UMuDPT


@TRAINER_REGISTRY.register()
class UUMuDPT(PromptTrainer):
    CFG_NODE, MODEL_NAME = "UUMUDPT", "UnifiedMultimodalDeepPromptTuning"  # trainers/uumudpt.py:239,276
    DROP_KEYS = ("uumudpt_prompt_learner.token_prefix", "uumudpt_prompt_learner.token_suffix")  # trainers/uumudpt.py:342-347

    def build_model(self):
        assert self.cfg.TRAINER.UUMUDPT.DEEP_PROMPT_DEPTH > 0, "PROMPT_DEPTH should be > 0"  # trainers/uumudpt.py:92
        super().build_model()

    def prompt_setup(self, uc, names, ctx_len, near):
        # trainers/uumudpt.py:97-115,127-129 are umudpt.py's lines: the same ctx init words, prefix and class prompts
        n_ctx, depth, prompts, kwargs = UMuDPT.prompt_setup(self, uc, names, ctx_len, near)
        return n_ctx, depth, prompts, dict(kwargs, variant="uumudpt")
