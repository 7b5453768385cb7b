"""Drop-in ``UMuDPT`` trainer plugin: the reference's ``trainers/umudpt.py:233-346`` surface over libmudpt_hip.so.

Same class name, registry name, hooks and error behaviour: ``check_cfg``, ``build_model``, ``forward_backward`` (``{"loss"}``),
``parse_batch_train``, inherited ``model_inference`` and ``load_model``.  The towers are MuDPT's; the vision prompts of every layer are
generated from the text prompts of every layer by a trainable pre-LN transformer block (``UMuDPTPromptLearner``, umudpt.py:79-178), which the
library runs in fp32 (mudpt_amd/csrc/promptgen.hip).  The module owns the reference's 20 trainables -- every parameter whose name contains
"prompt_learner" (umudpt.py:252-255) -- under its keys ``umudpt_prompt_learner.*``, and the whole model is registered as
"UnifiedMultimodalDeepPromptTuning" (umudpt.py:270), so ``--model-dir`` layouts load.  MODEL.INIT_WEIGHTS: the reference reads
``self.model.prompt_learner``, an attribute its model does not have (umudpt.py:263-264); here the file is loaded into the module that owns the
prompt learner's tensors.
"""
from __future__ import annotations

from .trainer import TRAINER_REGISTRY, PromptTrainer, class_prompts, ctx_init_token_ids


@TRAINER_REGISTRY.register()
class UMuDPT(PromptTrainer):
    CFG_NODE, MODEL_NAME = "UMUDPT", "UnifiedMultimodalDeepPromptTuning"  # trainers/umudpt.py:236,270
    DROP_KEYS = ("umudpt_prompt_learner.token_prefix", "umudpt_prompt_learner.token_suffix")  # trainers/umudpt.py:336-341

    def build_model(self):
        assert self.cfg.TRAINER.UMUDPT.DEEP_PROMPT_DEPTH > 0, "PROMPT_DEPTH should be > 0"  # trainers/umudpt.py:91
        super().build_model()

    def prompt_setup(self, uc, names, ctx_len, near):
        # trainers/umudpt.py:96-114,126-128: ctx init words, prompt prefix, "<prefix> <classname>." prompts
        ctx_init, ctx_ids = uc.CTX_INIT, None
        if ctx_init:
            ctx_init = ctx_init.replace("_", " ")
            prompt_prefix = " ".join(ctx_init.split()[:uc.N_CTX])
            ctx_ids = ctx_init_token_ids(ctx_init, uc.N_CTX, ctx_len, near)
        else:
            print("Initializing A Generic Context")
            prompt_prefix = " ".join(["X"] * uc.N_CTX)
        print(f'Initial context: "{prompt_prefix}"')
        print(f"Number of context words (tokens): {uc.N_CTX}")
        print(f"Depth of deep prompt: {uc.DEEP_PROMPT_DEPTH}")
        return uc.N_CTX, uc.DEEP_PROMPT_DEPTH, class_prompts(prompt_prefix, names, ctx_len, near), dict(ctx_token_ids=ctx_ids, variant="umudpt")
