"""Drop-in ``MuDPT`` trainer plugin: the reference's ``trainers/mudpt.py:187-302`` surface over libmudpt_hip.so.

Same class name, registry name, hooks and error behaviour as the reference plugin:
``check_cfg`` (:189), ``build_model`` (:192), ``forward_backward`` (:235), ``parse_batch_train`` (:263),
inherited ``model_inference`` (``self.model(input)``) and ``load_model`` (:270).  With Dassl installed it subclasses
``dassl.engine.TrainerX`` and registers in Dassl's ``TRAINER_REGISTRY`` so ``train.py --trainer MuDPT`` and
``scripts/mudpt/*.sh`` run unchanged; without Dassl it falls back to ``dassl_lite``.  Its hooks and ``build_model``
skeleton live in ``PromptTrainer``, which the CoCoOp, CoOp, VPT and MPT plugins (cocoop.py, coop.py, vpt.py) subclass as well.
"""
from __future__ import annotations

import dataclasses
import os
import os.path as osp

import torch

try:  # the real framework, when present
    from dassl.engine import TRAINER_REGISTRY, TrainerX
    from dassl.optim import build_optimizer, build_lr_scheduler
    from dassl.utils import load_checkpoint, load_pretrained_weights
    HAVE_DASSL = True
except ImportError:  # Dassl is not installed in the build image nor on the GPU box
    from .dassl_lite import TRAINER_REGISTRY, TrainerX, build_optimizer, build_lr_scheduler, load_checkpoint, load_pretrained_weights
    HAVE_DASSL = False

from . import evaluator, parallel, synth  # noqa: F401 -- evaluator: with Dassl, registers DeviceClassification in its EVALUATOR_REGISTRY
from .model import CustomCLIP, ModelShape

PREC_TO_DTYPE = {"fp16": "fp16", "fp32": "fp32", "amp": "bf16"}


def load_clip_state_dict(cfg):
    """trainers/mudpt.py:20-38 load_clip_to_cpu: a JIT archive or a plain state dict at MODEL.BACKBONE.PATH.
    The reference's name-based branch is a network download (and dead code); offline it is
    replaced by an explicit opt-in to seeded random weights (MODEL.BACKBONE.SYNTHETIC_SEED) for benchmarking."""
    path = cfg.MODEL.BACKBONE.PATH
    if path:
        print(f"Loading CLIP backbone: {cfg.MODEL.BACKBONE.NAME} from {path}")
        try:
            return torch.jit.load(path, map_location="cpu").eval().state_dict()
        except RuntimeError:
            return torch.load(path, map_location="cpu", weights_only=True)
    seed = cfg.MODEL.BACKBONE.get("SYNTHETIC_SEED", None) if hasattr(cfg.MODEL.BACKBONE, "get") else None
    if seed is None:
        raise RuntimeError("MODEL.BACKBONE.PATH is empty and no network is available to download "
                           f"{cfg.MODEL.BACKBONE.NAME}; set MODEL.BACKBONE.PATH to a local CLIP checkpoint")
    print(f"Building random-initialised CLIP {cfg.MODEL.BACKBONE.NAME} (seed {seed}) -- synthetic benchmark weights")
    return None


def open_backbone(cfg):
    """(ModelShape, CLIP state dict) of cfg.MODEL.BACKBONE: the checkpoint's, or the default ViT-B/16 shape with seeded random weights.  The
    shape's n_ctx / depth are placeholders: every plugin sets its own (dataclasses.replace)."""
    print(f"Loading CLIP (backbone: {cfg.MODEL.BACKBONE.NAME})")
    state = load_clip_state_dict(cfg)
    if state is None:  # a ResNet name of clip.load (clip/clip.py:32-36) selects that tower; every other name the default ViT-B/16, as before
        shape = ModelShape(**synth.RESNET_SHAPES.get(cfg.MODEL.BACKBONE.NAME, {}))
        return shape, synth.random_clip_state(shape, cfg.MODEL.BACKBONE.SYNTHETIC_SEED)
    return ModelShape.from_state_dict(state, 4, 1), state


def tokenize_prompts(prompts, ctx_len=77, near=None):
    """clip.tokenize (clip/clip.py:199-239) by the native BPE tokenizer (mudpt_amd/tokenizer.py); the merge table is looked for
    at $MUDPT_BPE_VOCAB, next to the checkpoint (``near``) and in an importable clip package.  Without a merge table only the
    benchmark prompts (recorded ids) can be served."""
    from . import tokenizer
    try:
        return tokenizer.tokenize(list(prompts), ctx_len, near=near)
    except RuntimeError as no_vocab:
        if "merge table" not in str(no_vocab):
            raise
        table = {f"a photo of a {n}.": i for i, n in enumerate(synth.BENCH_CLASSNAMES)}
        tok = synth.bench_tokenized_prompts(ctx_len)
        try:
            return torch.stack([tok[table[p]] for p in prompts])
        except KeyError as e:
            raise RuntimeError(f"no BPE merge table available for prompt {e}: {no_vocab}") from None


LOSS_SCALE_INIT, LOSS_SCALE_MIN, LOSS_SCALE_GROWTH_INTERVAL = 128.0, 1.0, 2000


def data_parallel_step(trainer, batch, with_acc: bool = False):
    """One training step of either plugin (trainers/mudpt.py:235-261, trainers/cocoop.py:246-276) in data-parallel form:
    forward + cross-entropy + backward in ONE library call on this rank's images (gradient of loss / world), ONE all-reduce of the
    flat bucket, the consensus on what every rank sees (parallel.step_consensus), then the optimizer step -- so replicas stay bitwise
    identical.  The logged loss is the GLOBAL-batch mean, as the reference's (nn.DataParallel gathers the logits before
    F.cross_entropy, trainers/mudpt.py:249-256).

    Loss scaling follows torch.cuda.amp.GradScaler (the reference's amp path, trainers/mudpt.py:228,239-246): the backward runs on
    per-sample gradients times a power-of-two scale inside the library; gradients that come back non-finite (an fp16 copy of a token
    gradient overflowed) make every rank SKIP the optimizer step and halve the scale; LOSS_SCALE_GROWTH_INTERVAL clean steps in a row
    double it again, up to the initial value.  A non-finite LOSS is an error, as in Dassl's model_backward_and_update.

    with_acc (the CoOp plugin, trainers/coop.py:297-300): the summary also has "acc", the top-1 accuracy of the GLOBAL batch in percent
    (dassl.metrics.compute_accuracy of the gathered logits): correct and total counts are summed over the ranks.

    A plugin that defines ``compute_loss(out, label)`` (PromptTrainer: None = not defined) replaces the ONE library call by
    ``model.differentiable`` (the training forward as a ``ClipOutputs`` of torch tensors), its own loss and ``loss.backward()`` into the
    zeroed bucket; everything behind the bucket -- all-reduce, consensus, loss-scale state machine, optimizer step -- is the same."""
    image, label = trainer.parse_batch_train(batch)
    model = trainer.model
    compute_loss = getattr(trainer, "compute_loss", None)
    if compute_loss is not None:  # a plugin with a loss of its own: the step split at the head, autograd in between
        model.flat_grads.zero_()  # differentiable() accumulates, as torch does
        out = model.differentiable(image, grad_scale=parallel.grad_scale())
        loss = compute_loss(out, label.to(out.logits.device))
        loss.backward()
        loss, logits = loss.detach(), out.logits
    elif with_acc:
        loss, logits = model.forward_backward(image, label, grad_scale=parallel.grad_scale(), return_logits=True)
    else:
        loss = model.forward_backward(image, label, grad_scale=parallel.grad_scale())
    if with_acc:
        counts = torch.stack([(logits.argmax(dim=1) == label.to(logits.device)).sum().float(),
                              torch.tensor(float(label.shape[0]), device=logits.device)])
        if parallel.world_size() > 1:
            torch.distributed.all_reduce(counts, op=torch.distributed.ReduceOp.SUM)
    parallel.allreduce_grads(model.flat_grads)
    loss_ok, grads_ok, global_loss = parallel.step_consensus(loss, model.flat_grads)
    if not loss_ok:
        raise FloatingPointError("Loss is infinite or NaN!")
    state = trainer.__dict__.setdefault("_loss_scale_state", {"scale": getattr(model, "loss_scale", LOSS_SCALE_INIT), "clean": 0, "skipped": 0})
    if grads_ok:
        trainer.optim.step()
        model.invalidate_text_cache()  # the optimizer wrote through .data views of the bucket
        state["clean"] += 1
        if state["clean"] >= LOSS_SCALE_GROWTH_INTERVAL and state["scale"] < LOSS_SCALE_INIT and hasattr(model, "set_loss_scale"):
            state["scale"], state["clean"] = state["scale"] * 2.0, 0
            model.set_loss_scale(state["scale"])
    else:
        if state["scale"] <= LOSS_SCALE_MIN or not hasattr(model, "set_loss_scale"):
            raise FloatingPointError("Gradients are infinite or NaN at the smallest loss scale!")
        state["scale"], state["clean"], state["skipped"] = state["scale"] * 0.5, 0, state["skipped"] + 1
        model.set_loss_scale(state["scale"])
        print(f"Gradient overflow: step skipped, loss scale halved to {state['scale']:g}")
    loss_summary = {"loss": global_loss}
    if with_acc:
        loss_summary["acc"] = (counts[0] * 100.0 / counts[1]).item()
    if (trainer.batch_idx + 1) == trainer.num_batches:
        trainer.update_lr()
    return loss_summary


DEVICE_DATA_TRANSFORMS = {"random_resized_crop", "random_flip", "normalize"}  # INPUT.TRANSFORMS of every yaml the reference ships


def _device_store(trainer, loader, local: int, attr: str, dm_method: str, noun: str, set_name: str, runs: str):
    """The DeviceImageStore a device-resident loader runs on, announced and kept as ``trainer.<attr>``: the one handed over there, else the set
    decoded once from the ``impath`` / ``label`` items of Dassl's data_source, else dassl_lite's synthetic uint8 set (``trainer.dm.<dm_method>``).
    None, after a one-line note, when no image list is found or the store would take more than a quarter of the free device memory."""
    from .augment import DeviceImageStore, StoreTooLarge
    device = f"cuda:{local}"
    budget = torch.cuda.mem_get_info(device)[0] // 4
    store = getattr(trainer, attr, None)
    if store is None:
        source = getattr(getattr(loader, "dataset", None), "data_source", None)
        try:
            if source is not None and len(source) > 0 and all(hasattr(item, "impath") and hasattr(item, "label") for item in source):
                store = DeviceImageStore.from_paths([item.impath for item in source], [item.label for item in source], device=device, max_bytes=budget)
            elif hasattr(getattr(trainer, "dm", None), dm_method):
                store = getattr(trainer.dm, dm_method)(device, max_bytes=budget)
            else:
                print(f"Device-resident {noun} refused: the {set_name} exposes no impath / label items; using the host loader")
                return None
        except StoreTooLarge as too_large:
            print(f"Device-resident {noun} refused: {too_large}, a quarter of the free device memory; using the host loader")
            return None
    setattr(trainer, attr, store)
    print(f"Device-resident {noun}: {len(store)} images, {store.nbytes / 2 ** 20:.1f} MiB of uint8 on {device}; {runs}")
    return store


def device_data_loader(trainer, loader, local: int):
    """The opt-in device-resident input path (mudpt_amd/augment.py; MUDPT_DEVICE_DATA=1 or trainer.device_store): a DeviceAugmentLoader over
    a DeviceImageStore -- trainer.device_store if one was handed over, else the training set decoded once from the ``impath`` / ``label``
    items of Dassl's data_source, else dassl_lite's synthetic uint8 set.  None, after a one-line note, when the configuration is not the one
    the kernel reproduces (exactly the three transforms above with INTERPOLATION "bicubic"), when no image list is found, or when the store
    would take more than a quarter of the free device memory: install_loader then goes on as without the opt-in."""
    from .augment import CLIP_MEAN, CLIP_STD, DeviceAugmentLoader
    inp = trainer.cfg.INPUT
    transforms, interpolation = set(getattr(inp, "TRANSFORMS", ()) or ()), getattr(inp, "INTERPOLATION", None)
    if transforms != DEVICE_DATA_TRANSFORMS or interpolation != "bicubic":
        print(f"Device-resident data refused: INPUT.TRANSFORMS {sorted(transforms)} / INTERPOLATION {interpolation!r} is not "
              f"{sorted(DEVICE_DATA_TRANSFORMS)} / 'bicubic'; using the host loader")
        return None
    store = _device_store(trainer, loader, local, "device_store", "uint8_store", "data", "training set",
                          "crop, flip and normalize run in one HIP launch per step")
    if store is None:
        return None
    return DeviceAugmentLoader(store, trainer.cfg.DATALOADER.TRAIN_X.BATCH_SIZE, inp.SIZE[0], getattr(inp, "PIXEL_MEAN", CLIP_MEAN), getattr(inp, "PIXEL_STD", CLIP_STD),
                               getattr(inp, "RRC_SCALE", (0.08, 1.0)), seed=trainer.cfg.SEED)


def install_loader(trainer, local: int):
    """Rank-aware, prefetched training loader (called at the end of build_model).  world > 1: ``train_loader_x`` is rebuilt over the same
    dataset with its batch sampler wrapped in parallel.ShardedBatchSampler, so each rank loads and decodes 1/world of every global
    batch (the reference's nn.DataParallel scatters ONE loaded batch, trainers/mudpt.py:230-233; here nothing is loaded N times);
    loaders that cannot be rebuilt (list-like synthetic ones) keep the slice-after-load fallback (parallel.shard_batch).  Then the
    DevicePrefetcher overlaps the next batch's host -> device copy with the current step.  With the opt-in of device_data_loader the
    images never leave the device and its loader takes the place of both."""
    from .prefetch import DevicePrefetcher
    loader = getattr(trainer, "train_loader_x", None)
    trainer._loader_sharded = False
    if loader is None or isinstance(loader, DevicePrefetcher):
        return
    if os.environ.get("MUDPT_DEVICE_DATA") == "1" or getattr(trainer, "device_store", None) is not None:
        device_loader = device_data_loader(trainer, loader, local)
        if device_loader is not None:
            trainer.train_loader_x = device_loader
            return
    if parallel.world_size() > 1:
        sharded = parallel.shard_loader(loader)  # unchanged if the loader is rank-aware already (MUDPT_DATA_SHARDED=1, DistributedSampler)
        if sharded is not None:
            loader, trainer._loader_sharded = sharded, True
    trainer.train_loader_x = DevicePrefetcher(loader, device=f"cuda:{local}", shard=not trainer._loader_sharded)


def device_test_loader(trainer, loader, local: int):
    """The opt-in device-resident test pass (MUDPT_DEVICE_TEST=1 or trainer.device_test_store; its own switch, MUDPT_DEVICE_DATA does not
    take it): a DeviceEvalLoader over a DeviceImageStore -- trainer.device_test_store if one was handed over, else the test set decoded once
    from the ``impath`` / ``label`` items of Dassl's data_source, else dassl_lite's synthetic uint8 test set.  Dassl's test transform is
    Resize(max(INPUT.SIZE)) + CenterCrop(INPUT.SIZE) + ToTensor and, if INPUT.TRANSFORMS names it, normalize, with INTERPOLATION: the
    kernel reproduces it for a square size, "normalize" and "bicubic".  None, after a one-line note, under the conditions
    device_data_loader refuses: another transform, no image list, a store over a quarter of the free device memory."""
    from .augment import CLIP_MEAN, CLIP_STD, DeviceEvalLoader
    inp = trainer.cfg.INPUT
    transforms, interpolation, size = set(getattr(inp, "TRANSFORMS", ()) or ()), getattr(inp, "INTERPOLATION", None), tuple(inp.SIZE)
    if "normalize" not in transforms or interpolation != "bicubic" or len(set(size)) != 1:
        print(f"Device-resident test data refused: INPUT.SIZE {size} / TRANSFORMS {sorted(transforms)} / INTERPOLATION {interpolation!r} is not "
              "a square size with 'normalize' / 'bicubic'; using the host loader")
        return None
    store = _device_store(trainer, loader, local, "device_test_store", "uint8_test_store", "test data", "test set",
                          "resize, center crop and normalize run in one HIP launch per batch")
    if store is None:
        return None
    return DeviceEvalLoader(store, trainer.cfg.DATALOADER.TEST.BATCH_SIZE, size[0], getattr(inp, "PIXEL_MEAN", CLIP_MEAN), getattr(inp, "PIXEL_STD", CLIP_STD))


def install_test_loader(trainer, local: int):
    """Under the opt-in of device_test_loader, ``test_loader`` becomes the DeviceEvalLoader; otherwise nothing changes."""
    from .augment import DeviceEvalLoader
    loader = getattr(trainer, "test_loader", None)
    if loader is None or isinstance(loader, DeviceEvalLoader):
        return
    if os.environ.get("MUDPT_DEVICE_TEST") == "1" or getattr(trainer, "device_test_store", None) is not None:
        device_loader = device_test_loader(trainer, loader, local)
        if device_loader is not None:
            trainer.test_loader = device_loader


def fused_optimizer(model, optim):
    """The opt-in fused optimizer step (mudpt_amd/optim.py; MUDPT_FUSED_OPTIM=1): a torch.optim.SGD / Adam / AdamW / RMSprop over exactly the
    tensors of the model's bucket becomes the BucketOptimizer of the same hyper-parameters, whose step is ONE HIP launch; its state_dict is
    torch's, so checkpoints move between the two.  Anything else -- another class, parameter groups that differ, maximize, only a part of
    the bucket -- is refused with a one-line note and ``optim`` is returned as it came."""
    from .optim import BucketOptimizer
    try:
        fused = BucketOptimizer.from_torch(optim, model=model, backend="hip")
    except ValueError as why:
        print(f"Fused optimizer step refused: {why}; stepping through torch.optim.{type(optim).__name__}")
        return optim
    print(f"Fused optimizer step: {fused.algo_name} over the bucket's {model.flat_params.numel()} elements in one HIP launch per step")
    return fused


def parse_batch(trainer, batch):
    """parse_batch_train of both plugins (trainers/mudpt.py:263-268, trainers/cocoop.py:278-283).  N > 1: this rank's share of the global
    batch -- already the whole batch when the loader is rank-aware or the batch came through the DevicePrefetcher (sliced, on the
    device: the two .to(device) are then no-ops), else the contiguous slice nn.DataParallel's scatter would give this GPU, taken on the
    host so that only 1/world of the images crosses PCIe."""
    input, label = batch["img"], batch["label"]
    if not batch.get("_mudpt_sharded", False) and not getattr(trainer, "_loader_sharded", False):
        input, label = parallel.shard_batch(input, label)
    return input.to(trainer.device), label.to(trainer.device)


def save_on_main(trainer, save, *args, **kwargs):
    """Replicas are identical: rank 0 alone writes OUTPUT_DIR; the others wait until the file is complete, so that a load_model that
    follows (Dassl's after_train with TEST.FINAL_MODEL = best_val, a resume) never reads a missing or half-written checkpoint.  The wait
    is an exchange of rank 0's success flag, not a bare barrier: if the save raised, EVERY rank raises (the others would otherwise walk
    on into the next collective, or into reading the missing file, while rank 0 unwinds)."""
    err = None
    if parallel.is_main():
        try:
            save(*args, **kwargs)
        except Exception as e:  # noqa: BLE001 -- re-raised below, after the other ranks have been told
            err = e
    if not parallel.all_ok(err is None):
        if err is not None:
            raise err
        raise RuntimeError("rank 0 failed to write the checkpoint (its traceback is on rank 0's stderr)")


def load_plugin_checkpoint(trainer, directory, epoch, drop_keys, skipped_note):
    """load_model of both plugins (trainers/mudpt.py:270-302, trainers/cocoop.py:285-307): {directory}/{name}/model.pth.tar-{epoch} or
    model-best.pth.tar, keys state_dict / epoch, the fixed token buffers dropped, strict=False (the frozen backbone entries of a
    reference checkpoint are ignored)."""
    if not directory:
        print(skipped_note)
        return
    names = trainer.get_model_names()
    model_file = "model-best.pth.tar"  # by default, the best model is loaded
    if epoch is not None:
        model_file = "model.pth.tar-" + str(epoch)
    for name in names:
        model_path = osp.join(directory, name, model_file)
        if not osp.exists(model_path):
            raise FileNotFoundError('Model not found at "{}"'.format(model_path))
        checkpoint = load_checkpoint(model_path)
        state_dict = checkpoint["state_dict"]
        epoch = checkpoint["epoch"]
        for k in drop_keys:  # ignore fixed token vectors
            state_dict.pop(k, None)
        print("Loading weights to {} " 'from "{}" (epoch = {})'.format(name, model_path, epoch))
        trainer._models[name].load_state_dict(state_dict, strict=False)


def class_parallel_shard(n_cls: int, setting=None):
    """This rank's class range for the class-parallel text tower, or None (every rank encodes all classes, as the reference does).
    ``setting``: cfg.TRAINER.MUDPT.CLASS_PARALLEL if the config defines it, else the environment variable MUDPT_CLASS_PARALLEL:
    "1" / True = on, "0" / False = off, unset / "auto" = on when there is more than one rank and at least 256 classes (ImageNet: the
    replicated text tower is 39 % of the step's FLOPs; at 11 classes it hides behind the vision tower and the two extra
    exchanges would only cost).  Every rank must then run the same sequence of forward calls (training steps, test batches)."""
    world = parallel.world_size()
    if setting is None:
        setting = os.environ.get("MUDPT_CLASS_PARALLEL", "auto")
    if isinstance(setting, str):
        setting = {"1": True, "true": True, "on": True, "0": False, "false": False, "off": False}.get(setting.lower(), "auto")
    on = (world > 1 and n_cls >= 256) if setting == "auto" else bool(setting)
    if not on or world <= 1 or world > n_cls:
        return None
    return parallel.class_range(n_cls)


def precision_to_dtype(prec: str) -> str:
    """TRAINER.*.PREC -> library mode.  The reference's model is fp32 on its CPU path whatever PREC says (clip/clip.py:142-143 floats it;
    trainers/mudpt.py:199-200).  "fp32" selects the library's parity mode (include/mudpt.h MUDPT_F32: split forward GEMM operands -- fp16
    pairs + fp32 attention in the text tower, fp16 + e4m3 remainders on the fp8 matrix pipe in the vision tower): logits within 3.5e-4 of the
    reference at the logit scale pretrained checkpoints carry (100), at 1.27x the bf16 step.  "fp16" is the fast mode that holds 1e-3 at the
    INIT logit scale 14.29 only (4e-3 at 100: see warn_if_fp16_misses_the_bound), "amp" the bf16 throughput mode."""
    return PREC_TO_DTYPE[prec]


_warned_fp16_scale = False


def warn_if_fp16_misses_the_bound(prec: str, state) -> bool:
    """PREC = "fp16" (the reference yamls' default) on a REAL checkpoint: every released CLIP carries exp(logit_scale) = 100
    (clip/model.py:777 initialises ln(1 / 0.07) = 14.29, training drives it to the clamp at 100), and at that scale the fp16 mode's logits
    are ~4e-3 from the reference's fp32 CPU path (trainers/mudpt.py:178-182) -- outside north_star's 1e-3.  Say so once, and which setting
    holds the bound.  Returns whether it warned."""
    global _warned_fp16_scale
    if prec != "fp16" or state is None or "logit_scale" not in state:
        return False
    scale = float(torch.as_tensor(state["logit_scale"]).float().exp())
    if abs(scale - 100.0) >= 1.0:
        return False
    if not _warned_fp16_scale:
        print(f'NOTE: PREC "fp16" with exp(logit_scale) = {scale:.1f}: this mode rounds GEMM operands to fp16 and is ~4e-3 from the reference\'s '
              'fp32 logits at this scale (1e-3 is only held at the init scale 14.29).  PREC "fp32" selects the parity mode (<= 3.5e-4 at '
              'scale 100, ~1.2x the step time of "fp16"); "amp" is the bf16 throughput mode.')
        _warned_fp16_scale = True
    return True


def ctx_init_token_ids(text: str, n: int, ctx_len: int, near=None):
    """clip.tokenize(CTX_INIT)[0, 1:1 + n] (trainers/mudpt.py:60-63, cocoop.py:83-86, coop.py:57-60, mpt.py:59-62): the ids whose token
    embeddings initialise the context.  The benchmark's "a photo of a" comes from the recorded ids as far as they go, anything else from
    the BPE tokenizer."""
    if text == "a photo of a" and n <= len(synth.CTX_INIT_TOKENS):
        return synth.CTX_INIT_TOKENS[:n]
    return [int(v) for v in tokenize_prompts([text], ctx_len, near=near)[0, 1:1 + n]]


def class_prompts(prefix: str, names, ctx_len: int, near=None):
    """The tokenized "<prefix> <classname>." prompt of every class (trainers/mudpt.py:84-85, cocoop.py:110, coop.py:81, vpt.py:61, mpt.py:79)."""
    return tokenize_prompts([prefix + " " + name + "." for name in names], ctx_len, near=near)


class PromptTrainer(TrainerX):
    """The plugin layer every trainer of this package shares; not registered itself.  A plugin names its cfg node, its registered model
    and the fixed token buffers its load_model drops, and implements ``prompt_setup``; ``build_model`` is the reference plugins' common
    skeleton: backbone, CustomCLIP, optimizer / scheduler / register_model on the module that owns the trainables."""
    CFG_NODE = ""                  # cfg.TRAINER.<CFG_NODE>
    MODEL_NAME = ""                # register_model name: the checkpoint sub-directory
    DROP_KEYS = ()                 # fixed token buffers a checkpoint may hold; load_model ignores them
    SKIPPED_NOTE = "Note that load_model() is skipped as no pretrained model is given"
    WITH_ACC = False               # the step's summary also has "acc" (compute_accuracy of the logits)
    PROMPT_LEARNER_ONLY = False    # optimise, register and initialise model.prompt_learner, not the whole model
    FREEZE_NOTE = True             # print the reference's "Turning off gradients ..." line
    # compute_loss(self, out, label) -> scalar loss tensor; out: model.ClipOutputs(logits, image_features, text_features), label [B] on the
    # device.  None: not defined -- the step is the library's fused forward + cross-entropy + backward.  A subclass that defines it trains
    # on that loss instead (data_parallel_step; INTEGRATION.md has worked examples)
    compute_loss = None

    def check_cfg(self, cfg):
        assert getattr(cfg.TRAINER, self.CFG_NODE).PREC in ["fp16", "fp32", "amp"]  # trainers/mudpt.py:190, cocoop.py:204, coop.py:236, ...

    def prompt_setup(self, node, names, ctx_len: int, near):
        """Print the prompt settings; return (n_ctx, depth) of the ModelShape, the tokenized class prompts and the plugin's own CustomCLIP
        keyword arguments (ctx_token_ids, variant, ...).  ``names``: the class names with "_" replaced by " "."""
        raise NotImplementedError

    def build_model(self):
        cfg = self.cfg
        node = getattr(cfg.TRAINER, self.CFG_NODE)
        self.check_compute_loss()
        backbone, state = open_backbone(cfg)  # the prompt's n_ctx / depth come from prompt_setup
        cfg_imsize = cfg.INPUT.SIZE[0]
        assert cfg_imsize == backbone.image_size, f"cfg_imsize ({cfg_imsize}) must equal to clip_imsize ({backbone.image_size})"  # mudpt.py:55
        warn_if_fp16_misses_the_bound(node.PREC, state)
        names = [name.replace("_", " ") for name in self.dm.dataset.classnames]
        n_ctx, depth, tokenized, kwargs = self.prompt_setup(node, names, backbone.ctx_len, cfg.MODEL.BACKBONE.PATH or None)

        print("Building custom CLIP")
        # one process per GPU (the reference: nn.DataParallel in one process): join the process group torch.distributed.run set up
        # BEFORE the model exists, so grad_scale = 1 / world and the parameter broadcast below are in effect from step one
        rank, world, local = parallel.init()
        max_batch = max(-(-cfg.DATALOADER.TRAIN_X.BATCH_SIZE // world), cfg.DATALOADER.TEST.BATCH_SIZE)
        self.model = CustomCLIP(dataclasses.replace(backbone, n_ctx=n_ctx, depth=depth), state, tokenized, max_batch=max_batch,
                                dtype=precision_to_dtype(node.PREC), device=f"cuda:{local}", seed=cfg.SEED, **kwargs)
        if self.model.class_shard is not None:  # MuDPT only: CustomCLIP shards no other variant
            print(f"Class-parallel text tower: this rank encodes classes {self.model.class_shard[0]}..{self.model.class_shard[1] - 1} of {len(names)}")
        if self.FREEZE_NOTE:
            print("Turning off gradients in both the image and the text encoder")
        # the freeze rules (trainers/mudpt.py:205-218, cocoop.py:220-232, ...) are structural here: the module only owns the trainables
        print(f"Parameters to be updated: {set(self.model.param_names)}")
        # CoCoOp / CoOp give only prompt_learner to the optimizer (cocoop.py:239, coop.py:268).  MuDPT, VPT and MPT initialise
        # self.model.prompt_learner, an attribute their models do not have (mudpt.py:220-221, vpt.py:152-153, mpt.py:210-211, SURVEY
        # appendix A.3); the evident intent -- initialise the trainables from a checkpoint -- is applied to the module that owns them
        trained = self.model.prompt_learner if self.PROMPT_LEARNER_ONLY else self.model
        if cfg.MODEL.INIT_WEIGHTS:
            load_pretrained_weights(trained, cfg.MODEL.INIT_WEIGHTS)
        self.optim = build_optimizer(trained, cfg.OPTIM)
        if os.environ.get("MUDPT_FUSED_OPTIM") == "1":
            self.optim = fused_optimizer(self.model, self.optim)
        self.sched = build_lr_scheduler(self.optim, cfg.OPTIM)
        self.register_model(self.MODEL_NAME, trained, self.optim, self.sched)
        self.scaler = None  # loss scaling lives inside the library (mudpt_set_loss_scale)
        # the reference wraps in nn.DataParallel when device_count > 1 (mudpt.py:230-233); here: one process per GPU
        if parallel.world_size() > 1:
            parallel.broadcast_params(self.model.flat_params)
        install_loader(self, local)  # rank-aware (world > 1) and prefetched training loader
        self._local = local

    def check_compute_loss(self):
        """A plugin whose step cannot be split at the head refuses a defined ``compute_loss`` here, before anything is built."""

    def test(self, split=None):
        from . import featcache
        install_test_loader(self, self._local)  # the opt-in may be taken after construction (trainer.device_test_store)
        # MUDPT_TEST_FEATURES=<dir> / trainer.test_features: CoOp and CoCoOp may run from cached image features; without it, the pass as it was
        return featcache.run_test(self, split, super().test)

    def forward_backward(self, batch):
        return data_parallel_step(self, batch, with_acc=self.WITH_ACC)

    def parse_batch_train(self, batch):
        return parse_batch(self, batch)

    def save_model(self, *args, **kwargs):
        save_on_main(self, super().save_model, *args, **kwargs)

    def load_model(self, directory, epoch=None):
        load_plugin_checkpoint(self, directory, epoch, self.DROP_KEYS, self.SKIPPED_NOTE)


@TRAINER_REGISTRY.register()
class MuDPT(PromptTrainer):
    CFG_NODE, MODEL_NAME = "MUDPT", "MultimodalDeepPromptTuning"  # trainers/mudpt.py:190,227
    DROP_KEYS = ("mudpt_prompt_learner.token_prefix", "mudpt_prompt_learner.token_suffix")  # trainers/mudpt.py:293-298
    FREEZE_NOTE = False

    def build_model(self):
        assert self.cfg.TRAINER.MUDPT.DEEP_PROMPT_DEPTH > 0, "PROMPT_DEPTH should be > 0"  # trainers/mudpt.py:52
        super().build_model()

    def prompt_setup(self, mc, names, ctx_len, near):
        # trainers/mudpt.py:57-75,83-85: ctx init words, prompt prefix, "<prefix> <classname>." prompts
        ctx_init, ctx_ids = mc.CTX_INIT, None
        if ctx_init:
            ctx_init = ctx_init.replace("_", " ")
            prompt_prefix = " ".join(ctx_init.split()[:mc.N_CTX])
            ctx_ids = ctx_init_token_ids(ctx_init, mc.N_CTX, ctx_len, near)
        else:
            print("Initializing A Generic Context")
            prompt_prefix = " ".join(["X"] * mc.N_CTX)
        print(f'Initial context: "{prompt_prefix}"')
        print(f"Number of context words (tokens): {mc.N_CTX}")
        print(f"Depth of deep prompt: {mc.DEEP_PROMPT_DEPTH}")
        return mc.N_CTX, mc.DEEP_PROMPT_DEPTH, class_prompts(prompt_prefix, names, ctx_len, near), dict(
            ctx_token_ids=ctx_ids, variant="mudpt", class_shard=class_parallel_shard(len(names), getattr(mc, "CLASS_PARALLEL", None)))
