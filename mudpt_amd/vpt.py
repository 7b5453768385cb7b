"""Drop-in ``VPT`` and ``MPT`` trainer plugins: the reference's ``trainers/vpt.py:127-235`` and ``trainers/mpt.py:185-270`` surfaces over
libmudpt_hip.so.

Same class names, registry names, hooks and error behaviour: ``check_cfg``, ``build_model``, ``forward_backward`` (``{"loss", "acc"}``),
``parse_batch_train``, inherited ``model_inference`` and ``load_model``.  Both trainers prompt every block ``1 <= i < depth`` of a tower with
a ``visual_ctx`` of its own (``ResidualAttentionBlock_VPT``, clip/model.py:202-251): VPT in the vision tower only, MPT in both, each with
its own row count and depth (TRAINER.<NAME>.DEEP_TEXT_N_CTX / TEXT_PROMPT_DEPTH / DEEP_VISUAL_N_CTX / VISUAL_PROMPT_DEPTH).  The module
owns exactly the reference's trainables (the freeze rules of vpt.py:141-146 / mpt.py:195-202) under its keys, and the whole model is
registered under the reference's names ("VisualPromptLearner" / "MultiModalPromptLearner"), so ``--model-dir`` layouts load.
"""
from __future__ import annotations

from . import parallel, synth
from .model import CustomCLIP, ModelShape
from .trainer import (TRAINER_REGISTRY, TrainerX, build_lr_scheduler, build_optimizer, data_parallel_step, install_loader, load_clip_state_dict,
                      load_plugin_checkpoint, load_pretrained_weights, parse_batch, precision_to_dtype, save_on_main, tokenize_prompts,
                      warn_if_fp16_misses_the_bound)

# the shipped yamls' prompt shapes (configs/trainers/VPT|MPT/vit_b16_c2_ep5_batch4.yaml): (DEEP_TEXT_N_CTX, TEXT_PROMPT_DEPTH,
# DEEP_VISUAL_N_CTX, VISUAL_PROMPT_DEPTH)
YAML_PROMPTS = {"VPT": (0, 0, 8, 12), "MPT": (2, 12, 2, 12)}


def prompt_shape(node):
    return (int(node.DEEP_TEXT_N_CTX), int(node.TEXT_PROMPT_DEPTH), int(node.DEEP_VISUAL_N_CTX), int(node.VISUAL_PROMPT_DEPTH))


def _build(trainer, name: str, model_name: str):
    """build_model of both plugins: trainers/vpt.py:131-166, trainers/mpt.py:189-222."""
    cfg = trainer.cfg
    classnames = trainer.dm.dataset.classnames
    node = getattr(cfg.TRAINER, name)
    print(f"Loading CLIP (backbone: {cfg.MODEL.BACKBONE.NAME})")
    state = load_clip_state_dict(cfg)
    if state is None:
        shape = ModelShape(depth=1)
        state = synth.random_clip_state(shape, cfg.MODEL.BACKBONE.SYNTHETIC_SEED)
    else:
        shape = ModelShape.from_state_dict(state, 4, 1)
    cfg_imsize = cfg.INPUT.SIZE[0]
    assert cfg_imsize == shape.image_size, f"cfg_imsize ({cfg_imsize}) must equal to clip_imsize ({shape.image_size})"  # vpt.py:48, mpt.py:52
    warn_if_fp16_misses_the_bound(node.PREC, state)
    t_n, t_depth, v_n, v_depth = prompt_shape(node)
    near = cfg.MODEL.BACKBONE.PATH or None
    ctx_init, ctx_ids = node.TEXT_CTX_INIT, None
    if name == "VPT" or ctx_init:
        # VPT: the fixed prompt "<TEXT_CTX_INIT> <name>." (vpt.py:52-66); MPT: the WHOLE init string is the prefix, and rows 1..n_t of its
        # tokens initialise text_prompt_learner.visual_ctx (mpt.py:55-62)
        prompt_prefix = ctx_init.replace("_", " ")
        if name == "MPT":
            ctx_ids = [int(v) for v in tokenize_prompts([prompt_prefix], shape.ctx_len, near=near)[0, 1:1 + t_n]] \
                if prompt_prefix != "a photo of a" or t_n > 4 else synth.CTX_INIT_TOKENS[:t_n]
    else:
        print("Initializing a generic context")  # mpt.py:63-67
        prompt_prefix = " ".join(["X"] * t_n)
    print(f'Initial context: "{prompt_prefix}"')
    print(f"Number of context words (tokens) of deep visual prompt: {v_n}")
    print(f"Number of context words (tokens) of deep text prompt: {t_n}")
    print(f"Number of depth of deep visual prompt: {v_depth}")
    print(f"Number of depth of deep text prompt: {t_depth}")
    names = [n.replace("_", " ") for n in classnames]
    prompts = [prompt_prefix + " " + n + "." for n in names]
    tokenized = tokenize_prompts(prompts, shape.ctx_len, near=near)

    print("Building custom CLIP")
    rank, world, local = parallel.init()
    max_batch = max(-(-cfg.DATALOADER.TRAIN_X.BATCH_SIZE // world), cfg.DATALOADER.TEST.BATCH_SIZE)
    trainer.model = CustomCLIP(shape, state, tokenized, ctx_token_ids=ctx_ids, max_batch=max_batch, dtype=precision_to_dtype(node.PREC),
                               device=f"cuda:{local}", seed=cfg.SEED, variant=name.lower(), prompt_shape=(t_n, t_depth, v_n, v_depth))
    print("Turning off gradients in both the image and the text encoder")  # structural: the module owns the prompts only
    print(f"Parameters to be updated: {set(trainer.model.param_names)}")
    if cfg.MODEL.INIT_WEIGHTS:
        # vpt.py:148-149 / mpt.py:209-210 pass self.model.prompt_learner, an attribute these models do not have (as trainers/mudpt.py,
        # SURVEY appendix A.3); the evident intent -- initialise the trainables from a checkpoint -- is applied to the module that owns them
        load_pretrained_weights(trainer.model, cfg.MODEL.INIT_WEIGHTS)
    trainer.optim = build_optimizer(trainer.model, cfg.OPTIM)
    trainer.sched = build_lr_scheduler(trainer.optim, cfg.OPTIM)
    trainer.register_model(model_name, trainer.model, trainer.optim, trainer.sched)
    trainer.scaler = None  # loss scaling lives inside the library
    if parallel.world_size() > 1:  # nn.DataParallel becomes one process per GPU
        parallel.broadcast_params(trainer.model.flat_params)
    install_loader(trainer, local)


@TRAINER_REGISTRY.register()
class VPT(TrainerX):
    def check_cfg(self, cfg):
        assert cfg.TRAINER.VPT.PREC in ["fp16", "fp32", "amp"]  # trainers/vpt.py:129

    def build_model(self):
        _build(self, "VPT", "VisualPromptLearner")  # trainers/vpt.py:159

    def forward_backward(self, batch):
        return data_parallel_step(self, batch, with_acc=True)  # trainers/vpt.py:168-200

    def parse_batch_train(self, batch):
        return parse_batch(self, batch)

    def save_model(self, *args, **kwargs):
        save_on_main(self, super().save_model, *args, **kwargs)

    def load_model(self, directory, epoch=None):
        load_plugin_checkpoint(self, directory, epoch, ("text_prompt_learner.token_prefix", "text_prompt_learner.token_suffix"),  # vpt.py:225-229
                               "Note that load_model() is skipped as no pretrained model is given")


@TRAINER_REGISTRY.register()
class MPT(TrainerX):
    def check_cfg(self, cfg):
        assert cfg.TRAINER.MPT.PREC in ["fp16", "fp32", "amp"]  # trainers/mpt.py:187

    def build_model(self):
        _build(self, "MPT", "MultiModalPromptLearner")  # trainers/mpt.py:217

    def forward_backward(self, batch):
        return data_parallel_step(self, batch, with_acc=True)  # trainers/mpt.py:224-256

    def parse_batch_train(self, batch):
        return parse_batch(self, batch)

    def save_model(self, *args, **kwargs):
        save_on_main(self, super().save_model, *args, **kwargs)

    def load_model(self, directory, epoch=None):
        load_plugin_checkpoint(self, directory, epoch, ("text_prompt_learner.token_prefix", "text_prompt_learner.token_suffix"),
                               "Note that load_model() is skipped as no pretrained model is given")
