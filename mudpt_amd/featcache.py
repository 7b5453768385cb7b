"""The test pass from cached image features.

ZeroshotCLIP / ZeroshotCLIP2 (trainers/zsclip.py:74-79), CoOp (trainers/coop.py:212-223) and CoCoOp (trainers/cocoop.py:178-188) all begin
``model_inference`` with the frozen, prompt-free ``clip_model.visual(image)`` and read nothing else of the image.  Per image that is a
constant, and the reference already names the file that holds it: lpclip/feat_extractor.py:125-137 writes ``clip_model.visual(data)`` of a
whole split to ``{dir}/{dataset}/{split}.npz`` (``lpclip.save_features`` here).  With such a file a test pass is one
``model.forward_features`` launch chain per batch on rows of a table -- no decode, no transform, no vision tower -- and the file outlives
the process: the ``base2new`` / ``xd_test`` / ``run_zsclip`` scripts re-run the same pass per checkpoint, seed, shot count and class split.
On a ResNet backbone (RN50, RN101, RN50x16, RN50x64) the tower of a CoOp / CoCoOp handle is the frozen handle's bit for bit, so the file is the
one ``lpclip``'s extractor writes for the zero-shot and linear-probe baselines of the same table.

MuDPT, VPT, MPT, UMuDPT and UUMuDPT carry trainable prompts inside the vision tower: their features are no constants and are refused.

``decide_test_pass`` is the one place that decides what a pass does; ``run_test`` is what the plugins' ``test()`` call.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

from . import lpclip

FEATURE_TRAINERS = ("ZeroshotCLIP", "ZeroshotCLIP2", "CoOp", "CoCoOp")  # clip_model.visual(image) is frozen and prompt-free
PROMPT_IN_VISION_TRAINERS = ("MuDPT", "VPT", "MPT", "UMuDPT", "UUMuDPT")  # trainable prompts inside the vision tower
ENV = "MUDPT_TEST_FEATURES"


class FeatureStore:
    """fp32 [N, E] image features and int64 [N] labels of one split, in loader order, on any device.  ``name`` is the file they came from
    (or what stands for it in messages).  ValueError, naming it: features not 2-D / labels not 1-D, unequal lengths, an empty set, and --
    with ``width`` -- a feature width that is not the model's."""

    def __init__(self, features, labels, name: str = "<memory>", width=None, device=None):
        features, labels = torch.as_tensor(features), torch.as_tensor(labels)
        if features.dim() != 2 or labels.dim() != 1:
            raise ValueError(f"{name}: features must be [N, E] and labels [N], got {tuple(features.shape)} and {tuple(labels.shape)}")
        if features.shape[0] != labels.shape[0]:
            raise ValueError(f"{name}: {features.shape[0]} feature rows for {labels.shape[0]} labels")
        if features.shape[0] == 0 or features.shape[1] == 0:
            raise ValueError(f"{name}: an empty feature set {tuple(features.shape)}")
        if width is not None and features.shape[1] != width:
            raise ValueError(f"{name}: features of width {features.shape[1]}, the model's embed_dim is {width}")
        if labels.is_floating_point() or labels.dtype == torch.bool:
            raise ValueError(f"{name}: labels must be integers, got {labels.dtype}")
        device = features.device if device is None else torch.device(device)
        self.features = features.to(device=device, dtype=torch.float32).contiguous()
        self.labels = labels.to(device=device, dtype=torch.int64).contiguous()
        self.name = name

    def __len__(self):
        return self.features.shape[0]

    @property
    def width(self) -> int:
        return self.features.shape[1]

    @property
    def device(self):
        return self.features.device

    def to(self, device) -> "FeatureStore":
        return self if torch.device(device) == self.device else FeatureStore(self.features, self.labels, self.name, device=device)

    @classmethod
    def from_npz(cls, path, width=None, device=None) -> "FeatureStore":
        """``{dir}/{dataset}/{split}.npz`` with ``feature_list`` and ``label_list``: the reference's file (feat_extractor.py:119-137: Python
        lists of floats and ints, so float64 [N, E] and int64 [N] arrays) or the one ``save`` / ``lpclip.save_features`` writes."""
        path = os.fspath(path)
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("feature_list", "label_list") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: no array {' / '.join(missing)} (found {sorted(z.files)})")
            features, labels = z["feature_list"], z["label_list"]
        if not (np.issubdtype(features.dtype, np.floating) and np.issubdtype(labels.dtype, np.integer)):
            raise ValueError(f"{path}: feature_list must hold floats and label_list integers, got {features.dtype} and {labels.dtype}")
        return cls(torch.from_numpy(np.asarray(features, dtype=np.float32)), torch.from_numpy(np.asarray(labels, dtype=np.int64)), name=path,
                   width=width, device=device)

    @classmethod
    def from_loader(cls, model, loader, name: str = "<loader>") -> "FeatureStore":
        """feat_extractor.py:118-129 over ``loader`` with ``model.encode_image`` (a ``zsclip.FrozenCLIP``); the rows stay on the device."""
        features, labels = lpclip.extract_features(model, loader, on_device=True)
        return cls(features, labels, name=name, width=model.shape.embed_dim)

    def save(self, output_dir, dataset_name, split) -> str:
        """``lpclip.save_features``' file of this store."""
        return lpclip.save_features(output_dir, dataset_name, split, self.features, self.labels)


class FeatureLoader:
    """The test loader over a FeatureStore: every row once, in index order, the last batch short.  A batch is two slices of the store's
    tensors, {"feat", "label"}: no copy and no synchronisation per batch."""

    def __init__(self, store: FeatureStore, batch_size: int):
        self.store, self.batch_size = store, int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"a test batch of {batch_size} feature rows")

    def __len__(self):
        return -(-len(self.store) // self.batch_size)

    def __iter__(self):
        for lo in range(0, len(self.store), self.batch_size):
            yield {"feat": self.store.features[lo:lo + self.batch_size], "label": self.store.labels[lo:lo + self.batch_size]}


def _label_list(labels):
    return None if labels is None else [int(v) for v in torch.as_tensor(labels).reshape(-1).cpu().tolist()]


def decide_test_pass(trainer_name, model_width, store_n=None, store_labels=None, store_width=None, test_n=None, test_labels=None):
    """What a test pass under the opt-in does: ("use" | "write" | "refuse", reason).  Pure: names, sizes and labels in, a decision out.

    trainer_name / model_width: the plugin's registry name and its model's embed_dim.  store_n / store_labels / store_width: the cached
    set's rows, labels and feature width; store_n None = there is no file yet.  test_n / test_labels: the test set's, where the loader
    exposes them (None: not known, not checked).

      refuse   one of the five trainers with prompts inside the vision tower, or a name that is none of the nine; a feature width that
               is not the model's; another number of rows than the test set; any differing label -- the guard against a file extracted
               under another DATASET.SUBSAMPLE_CLASSES, which relabels the classes from 0
      write    no file yet: the pass runs on the images and saves their features
      use      everything known agrees
    """
    if trainer_name in PROMPT_IN_VISION_TRAINERS:
        return "refuse", f"{trainer_name} carries trainable prompts inside the vision tower, so its image features are no constants"
    if trainer_name not in FEATURE_TRAINERS:
        return "refuse", f"{trainer_name} is none of {', '.join(FEATURE_TRAINERS)}"
    if store_n is None:
        return "write", "no feature file yet"
    if store_width != model_width:
        return "refuse", f"features of width {store_width}, the model's embed_dim is {model_width}"
    if test_n is not None and store_n != test_n:
        return "refuse", f"{store_n} feature rows for a test set of {test_n} images"
    have, want = _label_list(store_labels), _label_list(test_labels)
    if want is not None:
        if have is None or len(have) != len(want):
            return "refuse", f"{0 if have is None else len(have)} cached labels for {len(want)} test labels"
        differ = [i for i, (a, b) in enumerate(zip(have, want)) if a != b]
        if differ:
            i = differ[0]
            return "refuse", (f"{len(differ)} of {len(want)} labels differ from the test set's (first: row {i}, cached {have[i]}, test set {want[i]}): "
                              "extracted under another class split?")
    return "use", f"{store_n} rows of width {store_width}" + ("" if want is not None else "; the loader exposes no labels to check them against")


def loader_labels(loader):
    """The labels of a test loader in its order, without loading an image: Dassl's ``dataset.data_source`` items, a device-resident
    loader's store, or a list of ready batches (dassl_lite's synthetic loader).  None where the loader exposes none of these."""
    source = getattr(getattr(loader, "dataset", None), "data_source", None)
    if source is not None and len(source) > 0 and all(hasattr(item, "label") for item in source):
        return torch.tensor([int(item.label) for item in source], dtype=torch.int64)
    store = getattr(loader, "store", None)
    if store is not None and hasattr(store, "labels"):
        return torch.as_tensor(store.labels).to("cpu", torch.int64)
    if isinstance(loader, (list, tuple)) and loader and all(isinstance(b, dict) and "label" in b for b in loader):
        return torch.cat([torch.as_tensor(b["label"]).reshape(-1).to("cpu", torch.int64) for b in loader])
    return None


def _split_loader(trainer, split):
    """Dassl's SimpleTrainer.test(): split None -> cfg.TEST.SPLIT; "val" with a val_loader -> that loader, anything else the test set."""
    if split is None:
        split = getattr(getattr(trainer.cfg, "TEST", None), "SPLIT", "test")
    if split == "val" and getattr(trainer, "val_loader", None) is not None:
        return "val", "val_loader"
    return "test", "test_loader"


@contextlib.contextmanager
def _swapped(trainer, **attrs):
    """The trainer's attributes replaced for one pass, then put back (an instance attribute that was not there is removed)."""
    missing = object()
    before = {k: trainer.__dict__.get(k, missing) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(trainer, k, v)
        yield
    finally:
        for k, v in before.items():
            if v is missing:
                trainer.__dict__.pop(k, None)
            else:
                setattr(trainer, k, v)


def run_test(trainer, split, image_test):
    """``test()`` of every plugin.  ``image_test(split=...)`` is the framework's own pass over images.  Without the opt-in -- the
    environment's MUDPT_TEST_FEATURES=<feature_dir> or ``trainer.test_features = FeatureStore(...)`` -- that is all that runs.  With it,
    by ``decide_test_pass``:

      use     the same pass with the loader replaced by a FeatureLoader and ``model_inference`` by ``model.forward_features``: each batch
              drives ``evaluator.process(model.forward_features(feat), label)``
      write   the pass on images; ``model.image_features()`` is collected per batch and rank 0 writes
              ``{feature_dir}/{DATASET.NAME}/{split}.npz`` at the end (every rank evaluates the whole set, as without the switch)
      refuse  a one-line note, then the pass on images
    """
    from . import parallel
    store, feature_dir = getattr(trainer, "test_features", None), os.environ.get(ENV)
    if store is None and not feature_dir:
        return image_test(split=split)
    name = type(trainer).__name__
    split_name, loader_attr = _split_loader(trainer, split)
    loader = getattr(trainer, loader_attr)
    model = trainer.model
    width = getattr(getattr(model, "shape", None), "embed_dim", None)
    path = None
    if name in FEATURE_TRAINERS and store is None:
        path = os.path.join(feature_dir, trainer.cfg.DATASET.NAME, f"{split_name}.npz")
        if os.path.exists(path):
            try:
                store = FeatureStore.from_npz(path, device=model.device)
            except ValueError as bad:
                print(f"Cached test features refused: {bad}; running on the images")
                return image_test(split=split)
    labels = loader_labels(loader)
    if store is None:
        action, reason = decide_test_pass(name, width)
    else:
        action, reason = decide_test_pass(name, width, len(store), store.labels, store.width, None if labels is None else len(labels), labels)
    if action == "refuse":
        print(f"Cached test features refused: {reason}; running on the images")
        return image_test(split=split)
    if action == "use":
        store = store.to(model.device)
        print(f"Cached test features: {len(store)} rows of {store.name}; the vision tower does not run")
        feature_loader = FeatureLoader(store, trainer.cfg.DATALOADER.TEST.BATCH_SIZE)
        with _swapped(trainer, **{loader_attr: feature_loader, "parse_batch_test": lambda batch: (batch["feat"], batch["label"]),
                                  "model_inference": model.forward_features}):
            return image_test(split=split)
    # write: the pass on images, keeping what the vision tower computed anyway
    features, kept_labels = [], []
    parse, infer = trainer.parse_batch_test, trainer.model_inference

    def parse_and_keep(batch):
        x, y = parse(batch)
        kept_labels.append(torch.as_tensor(y).reshape(-1).to(model.device, torch.int64))
        return x, y

    def infer_and_keep(x):
        out = infer(x)
        features.append(model.image_features())
        return out

    with _swapped(trainer, parse_batch_test=parse_and_keep, model_inference=infer_and_keep):
        result = image_test(split=split)
    if parallel.is_main():
        written = FeatureStore(torch.cat(features), torch.cat(kept_labels), name=path, width=width).save(feature_dir, trainer.cfg.DATASET.NAME, split_name)
        print(f"Cached test features: wrote {sum(f.shape[0] for f in features)} rows to {written}")
    return result
