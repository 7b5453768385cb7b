"""Drop-in ``CoCoOp`` trainer plugin: the reference's ``trainers/cocoop.py:201-322`` surface over libmudpt_hip.so
(BASELINE configs[3]).

Same class name, registry name, hooks and error behaviour: ``check_cfg`` (:203), ``build_model`` (:206), ``forward_backward``
(:252), ``parse_batch_train`` (:283), inherited ``model_inference`` (``self.model(input)`` in eval mode returns logits, :198) and
``load_model`` (:290).  As in the reference only the ``prompt_learner`` sub-module is given to the optimizer and registered
(:239-241), so checkpoints hold ``ctx`` and ``meta_net.*`` under the same keys.  The per-image text-encoder loop of
``CustomCLIP.forward`` (:187-194) is one batched pass over all (image, class) prompts inside the library.
"""
from __future__ import annotations

from .trainer import TRAINER_REGISTRY, PromptTrainer, class_prompts, ctx_init_token_ids


@TRAINER_REGISTRY.register()
class CoCoOp(PromptTrainer):
    CFG_NODE, MODEL_NAME, PROMPT_LEARNER_ONLY = "COCOOP", "prompt_learner", True
    DROP_KEYS = ("token_prefix", "token_suffix")  # trainers/cocoop.py:314-318
    SKIPPED_NOTE = "Note that load_model() is skipped as no Pretrained model is given"  # :292

    def check_compute_loss(self):
        assert self.compute_loss is None, ("CoCoOp takes no compute_loss: its step is chunked over the images, so all logits exist only after "
                                           "every backward would have had to start")

    def prompt_setup(self, cc, names, ctx_len, near):
        n_ctx, ctx_init, ctx_ids = cc.N_CTX, cc.CTX_INIT, None
        if ctx_init:  # trainers/cocoop.py:79-87: n_ctx follows the init words
            ctx_init = ctx_init.replace("_", " ")
            n_ctx = len(ctx_init.split(" "))
            ctx_ids, prompt_prefix = ctx_init_token_ids(ctx_init, n_ctx, ctx_len, near), ctx_init
        else:
            prompt_prefix = " ".join(["X"] * n_ctx)  # random N(0, 0.02^2) context (:90-92)
        print(f'Initial context: "{prompt_prefix}"')
        print(f"Number of context words (tokens): {n_ctx}")
        return n_ctx, 1, class_prompts(prompt_prefix, names, ctx_len, near), dict(ctx_token_ids=ctx_ids, variant="cocoop")  # :110-112
