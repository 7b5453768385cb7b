"""Drop-in ``VPT`` and ``MPT`` trainer plugins: the reference's ``trainers/vpt.py:122-236`` and ``trainers/mpt.py:177-294`` surfaces over
libmudpt_hip.so.

Same class names, registry names, hooks and error behaviour: ``check_cfg``, ``build_model``, ``forward_backward`` (``{"loss", "acc"}``),
``parse_batch_train``, inherited ``model_inference`` and ``load_model``.  Both trainers prompt every block ``1 <= i < depth`` of a tower with
a ``visual_ctx`` of its own (``ResidualAttentionBlock_VPT``, clip/model.py:202-251): VPT in the vision tower only, MPT in both, each with
its own row count and depth (TRAINER.<NAME>.DEEP_TEXT_N_CTX / TEXT_PROMPT_DEPTH / DEEP_VISUAL_N_CTX / VISUAL_PROMPT_DEPTH).  The module
owns exactly the reference's trainables (the freeze rules of vpt.py:141-146 / mpt.py:195-202) under its keys, and the whole model is
registered under the reference's names ("VisualPromptLearner" / "MultiModalPromptLearner"), so ``--model-dir`` layouts load.
"""
from __future__ import annotations

from .trainer import TRAINER_REGISTRY, PromptTrainer, class_prompts, ctx_init_token_ids

# the shipped yamls' prompt shapes (configs/trainers/VPT|MPT/vit_b16_c2_ep5_batch4.yaml): (DEEP_TEXT_N_CTX, TEXT_PROMPT_DEPTH,
# DEEP_VISUAL_N_CTX, VISUAL_PROMPT_DEPTH)
YAML_PROMPTS = {"VPT": (0, 0, 8, 12), "MPT": (2, 12, 2, 12)}


def prompt_shape(node):
    return (int(node.DEEP_TEXT_N_CTX), int(node.TEXT_PROMPT_DEPTH), int(node.DEEP_VISUAL_N_CTX), int(node.VISUAL_PROMPT_DEPTH))


def _tower_prompts(self, node, names, ctx_len, near):
    """prompt_setup of both plugins: trainers/vpt.py:52-62, trainers/mpt.py:55-79."""
    t_n, t_depth, v_n, v_depth = prompt_shape(node)
    mpt = self.CFG_NODE == "MPT"
    ctx_init, ctx_ids = node.TEXT_CTX_INIT, None
    if not mpt or ctx_init:
        # VPT: the fixed prompt "<TEXT_CTX_INIT> <name>." (vpt.py:52-66); MPT: the WHOLE init string is the prefix, and rows 1..n_t of its
        # tokens initialise text_prompt_learner.visual_ctx (mpt.py:55-62)
        prompt_prefix = ctx_init.replace("_", " ")
        if mpt:
            ctx_ids = ctx_init_token_ids(prompt_prefix, t_n, ctx_len, near)
    else:
        print("Initializing a generic context")  # mpt.py:63-67
        prompt_prefix = " ".join(["X"] * t_n)
    print(f'Initial context: "{prompt_prefix}"')
    print(f"Number of context words (tokens) of deep visual prompt: {v_n}")
    print(f"Number of context words (tokens) of deep text prompt: {t_n}")
    print(f"Number of depth of deep visual prompt: {v_depth}")
    print(f"Number of depth of deep text prompt: {t_depth}")
    # ModelShape's n_ctx / depth are unused by these variants: CustomCLIP takes the prompt_shape
    return 4, 1, class_prompts(prompt_prefix, names, ctx_len, near), dict(ctx_token_ids=ctx_ids, variant=self.CFG_NODE.lower(),
                                                                          prompt_shape=(t_n, t_depth, v_n, v_depth))


@TRAINER_REGISTRY.register()
class VPT(PromptTrainer):
    CFG_NODE, MODEL_NAME, WITH_ACC = "VPT", "VisualPromptLearner", True  # trainers/vpt.py:124-125,159,168-200
    DROP_KEYS = ("text_prompt_learner.token_prefix", "text_prompt_learner.token_suffix")  # trainers/vpt.py:227-231
    prompt_setup = _tower_prompts


@TRAINER_REGISTRY.register()
class MPT(PromptTrainer):
    CFG_NODE, MODEL_NAME, WITH_ACC = "MPT", "MultiModalPromptLearner", True  # trainers/mpt.py:179-180,217,226-252
    DROP_KEYS = ("text_prompt_learner.token_prefix", "text_prompt_learner.token_suffix")  # trainers/mpt.py:285-289
    prompt_setup = _tower_prompts
