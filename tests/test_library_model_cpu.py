"""The host plumbing that exists once, pinned on the CPU: the library's config struct (``model.library_config``), the handle base class
(``model.LibraryModel``), the store block of the two device-resident loaders, ``trainer.open_backbone`` and the writer of the feature file.

The expected values are literals: the sixteen integers and the printed lines are what ``CustomCLIP`` / ``FrozenCLIP`` and the two loaders
produced while each had its own copy."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mudpt_amd import capi, dassl_lite, featcache, lpclip, model, synth, trainer, zsclip
from mudpt_amd.model import LibraryModel, ModelShape, library_config

FIELDS = [name for name, _ in capi.Config._fields_]
SHAPE = ModelShape(image_size=32, patch=16, v_width=192, v_layers=3, v_heads=4, t_width=128, t_layers=2, t_heads=5, ctx_len=77, embed_dim=64,
                   n_ctx=6, depth=7)
BACKBONE = [32, 16, 192, 3, 4, 128, 2, 5, 77, 64]  # the first ten fields, in include/mudpt.h's order
DTYPE_CODES = {"bf16": 0, "fp16": 1, "fp32": 2}  # MUDPT_BF16 / MUDPT_F16 / MUDPT_F32
VARIANT_CODES = {"mudpt": 0, "cocoop": 1, "coop": 2, "coop_csc": 3, "vpt": 4, "mpt": 5, "umudpt": 6, "uumudpt": 7}  # MUDPT_VARIANT_*


def integers(cfg):
    assert isinstance(cfg, capi.Config)
    return [getattr(cfg, f) for f in FIELDS]


def test_fields_are_the_headers_sixteen():
    assert FIELDS == ["image_size", "patch", "v_width", "v_layers", "v_heads", "t_width", "t_layers", "t_heads", "ctx_len", "embed_dim", "n_ctx",
                      "depth", "n_cls", "max_batch", "dtype", "variant"]


@pytest.mark.parametrize("dtype", sorted(DTYPE_CODES))
@pytest.mark.parametrize("variant", sorted(VARIANT_CODES))
def test_library_config_of_a_trainable_handle(variant, dtype):
    want = BACKBONE + [6, 7, 11, 9, DTYPE_CODES[dtype], VARIANT_CODES[variant]]
    assert integers(library_config(SHAPE, 11, 9, dtype, variant)) == want
    assert integers(library_config(SHAPE, 11, 9, dtype, variant=variant, frozen=False)) == want


@pytest.mark.parametrize("dtype", sorted(DTYPE_CODES))
def test_library_config_of_a_frozen_handle(dtype):
    """n_ctx 0, depth 1, variant 0 whatever the shape says."""
    assert integers(library_config(SHAPE, 11, 9, dtype, frozen=True)) == BACKBONE + [0, 1, 11, 9, DTYPE_CODES[dtype], 0]


def test_library_config_defaults_and_unknown_names():
    assert integers(library_config(SHAPE, 11, 9, "bf16")) == BACKBONE + [6, 7, 11, 9, 0, 0]  # variant: "mudpt"
    with pytest.raises(KeyError):
        library_config(SHAPE, 11, 9, "fp64")
    with pytest.raises(KeyError):
        library_config(SHAPE, 11, 9, "fp64", frozen=True)
    with pytest.raises(KeyError):
        library_config(SHAPE, 11, 9, "bf16", "maple")


def test_one_base_owns_the_handle():
    assert issubclass(model.CustomCLIP, LibraryModel) and issubclass(zsclip.FrozenCLIP, LibraryModel) and issubclass(LibraryModel, torch.nn.Module)
    shared = ("close", "__del__", "_stream", "_check_images", "set_knob", "text_layout", "debug_read", "image_features")
    for name in shared:
        assert name in LibraryModel.__dict__, name
        for cls in (model.CustomCLIP, zsclip.FrozenCLIP):
            assert name not in cls.__dict__, (cls.__name__, name)


# ---- the two device-resident loaders ------------------------------------------------------------------------------------------------------

THREE = ["normalize", "random_flip", "random_resized_crop"]


def stub_trainer(interpolation):
    inp = SimpleNamespace(TRANSFORMS=("random_resized_crop", "random_flip", "normalize"), INTERPOLATION=interpolation, SIZE=(224, 224))
    return SimpleNamespace(cfg=SimpleNamespace(INPUT=inp))


def test_loaders_refuse_another_interpolation(capsys, monkeypatch):
    def no_cuda(*a, **k):
        raise AssertionError("a refused configuration must return before any CUDA call")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_cuda)
    t = stub_trainer("bilinear")
    assert trainer.device_data_loader(t, object(), 0) is None
    assert capsys.readouterr().out == (f"Device-resident data refused: INPUT.TRANSFORMS {THREE} / INTERPOLATION 'bilinear' is not "
                                       f"{THREE} / 'bicubic'; using the host loader\n")
    assert trainer.device_test_loader(t, object(), 0) is None
    assert capsys.readouterr().out == (f"Device-resident test data refused: INPUT.SIZE (224, 224) / TRANSFORMS {THREE} / INTERPOLATION 'bilinear' is not "
                                       "a square size with 'normalize' / 'bicubic'; using the host loader\n")
    assert not hasattr(t, "device_store") and not hasattr(t, "device_test_store")


def test_loaders_refuse_a_set_without_an_image_list(capsys, monkeypatch):
    asked = []
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: asked.append(device) or (1 << 30, 1 << 31))
    t = stub_trainer("bicubic")  # no dm; the loader has no dataset.data_source
    assert trainer.device_data_loader(t, object(), 0) is None
    assert capsys.readouterr().out == "Device-resident data refused: the training set exposes no impath / label items; using the host loader\n"
    assert trainer.device_test_loader(t, object(), 1) is None
    assert capsys.readouterr().out == "Device-resident test data refused: the test set exposes no impath / label items; using the host loader\n"
    assert asked == ["cuda:0", "cuda:1"]
    assert not hasattr(t, "device_store") and not hasattr(t, "device_test_store")


# ---- the backbone -------------------------------------------------------------------------------------------------------------------------

def test_open_backbone_synthetic(capsys, monkeypatch):
    """The state is ``synth.random_clip_state(ModelShape(), seed)``: drawn once (ViT-B/16 takes a second), so the call is recorded."""
    draw, drawn = synth.random_clip_state, []
    monkeypatch.setattr(synth, "random_clip_state", lambda *a, **k: drawn.append((a, k, draw(*a, **k))) or drawn[-1][2])
    cfg = dassl_lite.default_cfg()
    cfg.MODEL.BACKBONE.SYNTHETIC_SEED = 5
    shape, state = trainer.open_backbone(cfg)
    assert shape == ModelShape()
    assert [(a, k) for a, k, _ in drawn] == [((ModelShape(), 5), {})] and state is drawn[0][2]
    assert list(state) == [key for key, _, _ in synth.clip_state_table(ModelShape())] + ["logit_scale"]
    assert capsys.readouterr().out.splitlines() == ["Loading CLIP (backbone: ViT-B/16)",
                                                    "Building random-initialised CLIP ViT-B/16 (seed 5) -- synthetic benchmark weights"]


def test_open_backbone_needs_a_path_or_a_seed():
    cfg = dassl_lite.default_cfg()
    cfg.MODEL.BACKBONE.SYNTHETIC_SEED = None
    with pytest.raises(RuntimeError, match="MODEL.BACKBONE.PATH is empty and no network is available to download ViT-B/16; "
                                           "set MODEL.BACKBONE.PATH to a local CLIP checkpoint"):
        trainer.open_backbone(cfg)


# ---- the feature file ---------------------------------------------------------------------------------------------------------------------

def test_one_writer_of_the_feature_file(tmp_path):
    g = torch.Generator().manual_seed(2)
    features, labels = torch.randn(5, 8, generator=g, dtype=torch.float64), torch.tensor([3, 0, 2, 2, 1], dtype=torch.int32)
    loaded = []
    for save in (lambda: lpclip.save_features(str(tmp_path), "Pets", "test", features, labels),
                 lambda: featcache.FeatureStore(features, labels).save(str(tmp_path), "Pets", "test")):
        path = save()
        assert path == os.path.join(str(tmp_path), "Pets", "test.npz")
        assert os.listdir(tmp_path / "Pets") == ["test.npz"]  # and no temporary file
        with np.load(path) as z:
            assert sorted(z.files) == ["feature_list", "label_list"]
            loaded.append((z["feature_list"], z["label_list"]))
        os.remove(path)
    for f, y in loaded:
        assert f.dtype == np.float32 and y.dtype == np.int64
        assert np.array_equal(f, features.to(torch.float32).numpy()) and np.array_equal(y, labels.to(torch.int64).numpy())
    assert np.array_equal(loaded[0][0], loaded[1][0]) and np.array_equal(loaded[0][1], loaded[1][1])
