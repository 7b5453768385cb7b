"""No-GPU checks of the test pass from cached image features (mudpt_amd/featcache.py): the two new exports are declared and exported, the
feature file is read in both of its forms and written whole, the loader keeps the order, and the one function that decides what a pass
does decides it for every trainer and every mismatch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mudpt_amd import build, capi, featcache, lpclip
from mudpt_amd.featcache import FeatureLoader, FeatureStore, decide_test_pass


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


def test_new_exports_are_declared_and_exported(lib):
    i32, vp = C.c_int32, C.c_void_p
    assert capi.SIGNATURES["mudpt_forward_features"] == (i32, [vp, vp, i32, vp, i32, vp])
    assert capi.SIGNATURES["mudpt_image_features"] == (i32, [vp, i32, vp, vp])
    assert [n for n, _ in capi.DECLARATIONS["mudpt_forward_features"][1]] == ["m", "features_dev", "batch", "logits_dev", "flags", "stream"]
    assert [n for n, _ in capi.DECLARATIONS["mudpt_image_features"][1]] == ["m", "batch", "features_dev", "stream"]
    for name in ("mudpt_forward_features", "mudpt_image_features"):
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
    assert capi.ABI_VERSION == 7 and lib.mudpt_abi_version() == 7  # additions only
    # a null handle: refused before anything else is read
    assert lib.mudpt_forward_features(None, None, 1, None, 0, None) == 1 and b"null model" in lib.mudpt_last_error()
    assert lib.mudpt_image_features(None, 1, None, None) == 1 and b"null model" in lib.mudpt_last_error()


def table(n=7, e=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, e, generator=g), torch.randint(0, 4, (n,), generator=g)


def test_from_npz_reads_the_reference_file_and_its_own(tmp_path):
    f, y = table()
    # feat_extractor.py:119-137: Python lists of floats / ints handed to np.savez -> float64 [N, E] and int64 [N]
    ref = tmp_path / "reference.npz"
    np.savez(ref, feature_list=[row.tolist() for row in f], label_list=y.tolist())
    with np.load(ref) as z:
        assert z["feature_list"].dtype == np.float64 and z["label_list"].dtype == np.int64
    a = FeatureStore.from_npz(ref, width=5)
    assert a.features.dtype == torch.float32 and a.labels.dtype == torch.int64 and a.name == str(ref) and len(a) == 7 and a.width == 5
    assert torch.equal(a.features, f) and torch.equal(a.labels, y)  # fp32 -> float64 -> fp32 is exact
    own = lpclip.save_features(str(tmp_path / "feat"), "Caltech101", "test", f, y)
    b = FeatureStore.from_npz(own)
    assert torch.equal(b.features, f) and torch.equal(b.labels, y)
    # save: save_features' path and arrays, no temporary file left, and a round trip that is equal
    written = a.save(str(tmp_path / "feat2"), "Caltech101", "test")
    assert written == str(tmp_path / "feat2" / "Caltech101" / "test.npz") and os.listdir(tmp_path / "feat2" / "Caltech101") == ["test.npz"]
    with np.load(written) as z, np.load(own) as z0:
        assert sorted(z.files) == sorted(z0.files) == ["feature_list", "label_list"]
        for k in z.files:
            assert z[k].dtype == z0[k].dtype and np.array_equal(z[k], z0[k])
    c = FeatureStore.from_npz(written, width=5)
    assert torch.equal(c.features, a.features) and torch.equal(c.labels, a.labels)
    a.save(str(tmp_path / "feat2"), "Caltech101", "test")  # over an existing file: replaced, still alone
    assert os.listdir(tmp_path / "feat2" / "Caltech101") == ["test.npz"]
    # what lpclip's probe reads is the same file
    f2, y2 = lpclip._load(written)
    assert np.array_equal(f2, f.numpy()) and np.array_equal(y2, y.numpy())


def test_from_loader_is_extract_features_on_the_device():
    class Encoder:
        class shape:
            embed_dim = 5

        def encode_image(self, img):
            return img.reshape(img.shape[0], -1)[:, :5] * 2

    f, y = table(6)
    loader = [{"img": f[i:i + 4], "label": y[i:i + 4]} for i in range(0, 6, 4)]
    s = FeatureStore.from_loader(Encoder(), loader)
    assert torch.equal(s.features, f * 2) and torch.equal(s.labels, y) and s.name == "<loader>"


def test_every_malformed_set_is_a_value_error_that_names_the_file(tmp_path):
    f, y = table()
    cases = {
        "features_1d": (f[:, 0], y, r"must be \[N, E\]"), "features_3d": (f[None], y, r"must be \[N, E\]"), "labels_2d": (f, y[:, None], r"labels \[N\]"),
        "labels_0d": (f, y[0], r"labels \[N\]"), "unequal": (f, y[:-1], "7 feature rows for 6 labels"), "empty": (f[:0], y[:0], "empty"),
        "no_columns": (f[:, :0], y, "empty"),
    }
    for name, (ff, yy, word) in cases.items():
        path = tmp_path / f"{name}.npz"
        np.savez(path, feature_list=ff.numpy(), label_list=yy.numpy())
        with pytest.raises(ValueError, match=word) as info:
            FeatureStore.from_npz(path)
        assert str(path) in str(info.value), name
    good = tmp_path / "good.npz"
    np.savez(good, feature_list=f.numpy(), label_list=y.numpy())
    with pytest.raises(ValueError, match="width 5, the model's embed_dim is 512") as info:
        FeatureStore.from_npz(good, width=512)
    assert str(good) in str(info.value)
    for name, arrays, word in (("no_labels", {"feature_list": f.numpy()}, "no array label_list"),
                               ("float_labels", {"feature_list": f.numpy(), "label_list": y.double().numpy()}, "integers"),
                               ("int_features", {"feature_list": f.long().numpy(), "label_list": y.numpy()}, "floats")):
        path = tmp_path / f"{name}.npz"
        np.savez(path, **arrays)
        with pytest.raises(ValueError, match=word) as info:
            FeatureStore.from_npz(path)
        assert str(path) in str(info.value), name
    # the same checks on tensors handed over directly, named as the caller names them
    with pytest.raises(ValueError, match="mine: 7 feature rows for 3 labels"):
        FeatureStore(f, y[:3], name="mine")
    with pytest.raises(ValueError, match="<memory>: an empty"):
        FeatureStore(f[:0], y[:0])


def test_feature_loader_keeps_the_order_and_yields_a_short_last_batch():
    f, y = table(7)
    s = FeatureStore(f, y)
    for bs, sizes in ((3, [3, 3, 1]), (7, [7]), (8, [7]), (1, [1] * 7)):
        loader = FeatureLoader(s, bs)
        batches = list(loader)
        assert len(loader) == len(batches) and [b["feat"].shape[0] for b in batches] == sizes and all(sorted(b) == ["feat", "label"] for b in batches)
        assert torch.equal(torch.cat([b["feat"] for b in batches]), f) and torch.equal(torch.cat([b["label"] for b in batches]), y)
        assert all(torch.equal(a["feat"], b["feat"]) and torch.equal(a["label"], b["label"]) for a, b in zip(batches, loader))  # a second pass: the same
        # slices of the store's own tensors: no copy
        assert all(b["feat"].data_ptr() == s.features[i * bs:].data_ptr() and b["label"].data_ptr() == s.labels[i * bs:].data_ptr() for i, b in enumerate(batches))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="test batch"):
            FeatureLoader(s, bad)


NINE = ("MuDPT", "CoCoOp", "CoOp", "VPT", "MPT", "UMuDPT", "UUMuDPT", "ZeroshotCLIP", "ZeroshotCLIP2")


def test_the_decision_for_every_trainer_and_every_mismatch():
    from mudpt_amd import dassl_lite, cocoop, coop, trainer, umudpt, uumudpt, vpt, zsclip  # noqa: F401 -- the plugins register themselves
    registered = set(trainer.TRAINER_REGISTRY.registered_names()) if hasattr(trainer.TRAINER_REGISTRY, "registered_names") else set(NINE)
    assert set(NINE) <= registered and set(featcache.FEATURE_TRAINERS) | set(featcache.PROMPT_IN_VISION_TRAINERS) == set(NINE)
    y = [0, 1, 2, 1, 0]
    for name in NINE:
        constant = name in ("ZeroshotCLIP", "ZeroshotCLIP2", "CoOp", "CoCoOp")
        # a matching store; no file; labels as a tensor, on either side
        use = decide_test_pass(name, 512, 5, y, 512, 5, torch.tensor(y))
        write = decide_test_pass(name, 512)
        if constant:
            assert use[0] == "use" and write[0] == "write", name
        else:
            for action, reason in (use, write):
                assert action == "refuse" and name in reason and "vision tower" in reason, (name, reason)
    for name in ("ZeroshotCLIP", "ZeroshotCLIP2", "CoOp", "CoCoOp"):
        action, reason = decide_test_pass(name, 512, 5, y, 768, 5, y)
        assert action == "refuse" and "768" in reason and "512" in reason
        action, reason = decide_test_pass(name, 512, 5, y, 512, 6, y + [0])
        assert action == "refuse" and "5 feature rows" in reason and "6" in reason
        action, reason = decide_test_pass(name, 512, 5, y, 512, 4, y[:4])
        assert action == "refuse"
        for i in range(5):  # any one label
            other = list(y)
            other[i] = 3
            action, reason = decide_test_pass(name, 512, 5, other, 512, 5, y)
            assert action == "refuse" and "1 of 5 labels differ" in reason and f"row {i}" in reason, reason
        # a relabelled half (SUBSAMPLE_CLASSES "new" read as "base"): the same count, other labels
        action, reason = decide_test_pass(name, 512, 5, [v + 3 for v in y], 512, 5, y)
        assert action == "refuse" and "5 of 5" in reason
        # a loader that exposes nothing: not checked, and the reason says so; N alone is still checked when it is known
        action, reason = decide_test_pass(name, 512, 5, y, 512)
        assert action == "use" and "no labels" in reason
        assert decide_test_pass(name, 512, 5, y, 512, 7, None)[0] == "refuse"
    action, reason = decide_test_pass("LinearProbe", 512, 5, y, 512, 5, y)
    assert action == "refuse" and "LinearProbe" in reason


def test_loader_labels_from_what_a_loader_exposes():
    class Item:
        def __init__(self, label):
            self.label, self.impath = label, "x.jpg"

    class Dataset:
        data_source = [Item(2), Item(0), Item(1)]

    class Loader:
        dataset = Dataset()

    class StoreLoader:
        class store:
            labels = torch.tensor([1, 1, 0])

    assert featcache.loader_labels(Loader()).tolist() == [2, 0, 1]
    assert featcache.loader_labels(StoreLoader()).tolist() == [1, 1, 0]
    assert featcache.loader_labels([{"img": None, "label": torch.tensor([3, 1])}, {"img": None, "label": torch.tensor([2])}]).tolist() == [3, 1, 2]
    assert featcache.loader_labels(iter(())) is None and featcache.loader_labels([]) is None
