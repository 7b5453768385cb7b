"""Drop-in ``CoOp`` trainer plugin: the reference's ``trainers/coop.py:229-345`` surface over libmudpt_hip.so.

Same class name, registry name, hooks and error behaviour: ``check_cfg`` (:236), ``build_model`` (:239), ``forward_backward``
(:281), ``parse_batch_train`` (:302), inherited ``model_inference`` and ``load_model`` (:314).  As in the reference only the
``prompt_learner`` sub-module -- its one tensor ``ctx``, shared ``[n_ctx, d_t]`` or class-specific ``[n_cls, n_ctx, d_t]`` (CSC) -- is
given to the optimizer and registered (:255-259), so checkpoints hold ``ctx`` under the same key.  CLASS_TOKEN_POSITION ("end", "middle",
"front") moves the context rows inside every class prompt; the library reorders the frozen rows once and splices the context at run time.
"""
from __future__ import annotations

from . import parallel, synth
from .model import CustomCLIP, ModelShape
from .trainer import (TRAINER_REGISTRY, TrainerX, build_lr_scheduler, build_optimizer, data_parallel_step, install_loader, load_clip_state_dict,
                      load_plugin_checkpoint, load_pretrained_weights, parse_batch, precision_to_dtype, save_on_main, tokenize_prompts, warn_if_fp16_misses_the_bound)


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
class CoOp(TrainerX):
    def check_cfg(self, cfg):
        assert cfg.TRAINER.COOP.PREC in ["fp16", "fp32", "amp"]  # trainers/coop.py:237

    def build_model(self):
        cfg = self.cfg
        classnames = self.dm.dataset.classnames
        cc = cfg.TRAINER.COOP
        print(f"Loading CLIP (backbone: {cfg.MODEL.BACKBONE.NAME})")
        state = load_clip_state_dict(cfg)
        n_ctx = cc.N_CTX
        ctx_init = cc.CTX_INIT
        near = cfg.MODEL.BACKBONE.PATH or None
        if ctx_init:  # trainers/coop.py:52-61: n_ctx follows the init words, and the context is shared whatever CSC says
            ctx_init = ctx_init.replace("_", " ")
            n_ctx = len(ctx_init.split(" "))
        if state is None:
            shape = ModelShape(n_ctx=n_ctx, depth=1)
            state = synth.random_clip_state(shape, cfg.MODEL.BACKBONE.SYNTHETIC_SEED)
        else:
            shape = ModelShape.from_state_dict(state, n_ctx, 1)
        cfg_imsize = cfg.INPUT.SIZE[0]
        assert cfg_imsize == shape.image_size, f"cfg_imsize ({cfg_imsize}) must equal to clip_imsize ({shape.image_size})"  # :51
        # fp16 at logit scale 100 (pretrained checkpoints): this mode is ~4e-3 from the reference's fp32 logits; "fp32" is the parity mode
        warn_if_fp16_misses_the_bound(cc.PREC, state)
        csc = bool(cc.CSC) and not ctx_init
        if ctx_init:
            ctx_ids = [int(v) for v in tokenize_prompts([ctx_init], shape.ctx_len, near=near)[0, 1:1 + n_ctx]] \
                if ctx_init != "a photo of a" else synth.CTX_INIT_TOKENS[:n_ctx]
            prompt_prefix = ctx_init
        else:
            print("Initializing class-specific contexts" if csc else "Initializing a generic context")
            ctx_ids, prompt_prefix = None, " ".join(["X"] * n_ctx)  # random N(0, 0.02^2) context (:63-72)
        print(f'Initial context: "{prompt_prefix}"')
        print(f"Number of context words (tokens): {n_ctx}")
        names = [name.replace("_", " ") for name in classnames]  # :78
        prompts = [prompt_prefix + " " + name + "." for name in names]  # :81
        name_lens = name_lengths(names, near)
        if name_lens is not None:
            tokenized = tokenize_prompts(prompts, shape.ctx_len, near=near)
        elif not ctx_init and names == synth.BENCH_CLASSNAMES:  # no merge table: the benchmark names' recorded ids
            tokenized, name_lens = synth.bench_coop_prompts(n_ctx, shape.ctx_len)
        else:
            raise RuntimeError("CoOp needs CLIP's BPE merge table for the class-name lengths (trainers/coop.py:80): set MUDPT_BPE_VOCAB")

        print("Building custom CLIP")
        rank, world, local = parallel.init()
        max_batch = max(-(-cfg.DATALOADER.TRAIN_X.BATCH_SIZE // world), cfg.DATALOADER.TEST.BATCH_SIZE)
        self.model = CustomCLIP(shape, state, tokenized, ctx_token_ids=ctx_ids, max_batch=max_batch, dtype=precision_to_dtype(cc.PREC),
                                device=f"cuda:{local}", seed=cfg.SEED, variant="coop_csc" if csc else "coop",
                                class_token_position=cc.CLASS_TOKEN_POSITION, name_lens=name_lens)
        print("Turning off gradients in both the image and the text encoder")  # structural: the module owns ctx only
        print(f"Parameters to be updated: {set(self.model.param_names)}")
        if cfg.MODEL.INIT_WEIGHTS:  # :248-249
            load_pretrained_weights(self.model.prompt_learner, cfg.MODEL.INIT_WEIGHTS)
        # NOTE: only give prompt_learner to the optimizer (:251)
        self.optim = build_optimizer(self.model.prompt_learner, cfg.OPTIM)
        self.sched = build_lr_scheduler(self.optim, cfg.OPTIM)
        self.register_model("prompt_learner", self.model.prompt_learner, self.optim, self.sched)
        self.scaler = None  # loss scaling lives inside the library
        if parallel.world_size() > 1:  # nn.DataParallel (:261-264) becomes one process per GPU
            parallel.broadcast_params(self.model.flat_params)
        install_loader(self, local)

    def forward_backward(self, batch):
        # output = model(image); loss = F.cross_entropy(output, label); backward + step (:281-300); loss_summary {"loss", "acc"}
        return data_parallel_step(self, batch, with_acc=True)

    def parse_batch_train(self, batch):
        return parse_batch(self, batch)

    def save_model(self, *args, **kwargs):
        save_on_main(self, super().save_model, *args, **kwargs)

    def load_model(self, directory, epoch=None):
        load_plugin_checkpoint(self, directory, epoch, ("token_prefix", "token_suffix"),  # trainers/coop.py:337-341
                               "Note that load_model() is skipped as no pretrained model is given")
