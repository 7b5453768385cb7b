"""Drop-in ``CoOp`` trainer plugin: the reference's ``trainers/coop.py:229-354`` surface over libmudpt_hip.so.

Same class name, registry name, hooks and error behaviour: ``check_cfg`` (:235), ``build_model`` (:238), ``forward_backward``
(:281), ``parse_batch_train`` (:307), inherited ``model_inference`` and ``load_model`` (:314).  As in the reference only the
``prompt_learner`` sub-module -- its one tensor ``ctx``, shared ``[n_ctx, d_t]`` or class-specific ``[n_cls, n_ctx, d_t]`` (CSC) -- is
given to the optimizer and registered (:268-270), so checkpoints hold ``ctx`` under the same key.  CLASS_TOKEN_POSITION ("end", "middle",
"front") moves the context rows inside every class prompt; the library reorders the frozen rows once and splices the context at run time.
"""
from __future__ import annotations

from . import synth
from .trainer import TRAINER_REGISTRY, PromptTrainer, class_prompts, ctx_init_token_ids


def name_lengths(classnames, near=None):
    """len(_tokenizer.encode(name)) per class (trainers/coop.py:80) by the native BPE tokenizer; None without a merge table."""
    from . import tokenizer
    try:
        tok = tokenizer.BPETokenizer(tokenizer.find_vocab(near=near))
    except RuntimeError as no_vocab:
        if "merge table" not in str(no_vocab):
            raise
        return None
    return [len(tok.encode(name)) for name in classnames]


@TRAINER_REGISTRY.register()
class CoOp(PromptTrainer):
    CFG_NODE, MODEL_NAME, PROMPT_LEARNER_ONLY, WITH_ACC = "COOP", "prompt_learner", True, True  # loss_summary {"loss", "acc"} (:297-300)
    DROP_KEYS = ("token_prefix", "token_suffix")  # trainers/coop.py:341-345

    def prompt_setup(self, cc, names, ctx_len, near):
        n_ctx, ctx_init, ctx_ids = cc.N_CTX, cc.CTX_INIT, None
        csc = bool(cc.CSC) and not ctx_init
        if ctx_init:  # trainers/coop.py:52-61: n_ctx follows the init words, and the context is shared whatever CSC says
            ctx_init = ctx_init.replace("_", " ")
            n_ctx = len(ctx_init.split(" "))
            ctx_ids, prompt_prefix = ctx_init_token_ids(ctx_init, n_ctx, ctx_len, near), ctx_init
        else:
            print("Initializing class-specific contexts" if csc else "Initializing a generic context")
            prompt_prefix = " ".join(["X"] * n_ctx)  # random N(0, 0.02^2) context (:63-72)
        print(f'Initial context: "{prompt_prefix}"')
        print(f"Number of context words (tokens): {n_ctx}")
        name_lens = name_lengths(names, near)  # :78-81
        if name_lens is not None:
            tokenized = class_prompts(prompt_prefix, names, ctx_len, near)
        elif not ctx_init and names == synth.BENCH_CLASSNAMES:  # no merge table: the benchmark names' recorded ids
            tokenized, name_lens = synth.bench_coop_prompts(n_ctx, ctx_len)
        else:
            raise RuntimeError("CoOp needs CLIP's BPE merge table for the class-name lengths (trainers/coop.py:80): set MUDPT_BPE_VOCAB")
        return n_ctx, 1, tokenized, dict(ctx_token_ids=ctx_ids, variant="coop_csc" if csc else "coop",
                                         class_token_position=cc.CLASS_TOKEN_POSITION, name_lens=name_lens)
