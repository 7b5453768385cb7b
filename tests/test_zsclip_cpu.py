"""No-GPU checks of the zero-shot trainers (trainers/zsclip.py): the registry, the restated template tables, the prompt strings, the native
tokenizer against the recorded ids, the CPU restatement against the fixtures of the reference's own classes, the host-side refusals of the
frozen handle's entry points, and the linear-probe feature file."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mudpt_amd import build, capi
from tests import zsclip_reference as R


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


@pytest.fixture(scope="module")
def cases():
    return {name: R.ZsCase(name) for name in R.FIXTURES}


def test_both_trainers_are_registered():
    from mudpt_amd import zsclip
    from mudpt_amd.trainer import TRAINER_REGISTRY, TrainerX
    assert TRAINER_REGISTRY.get("ZeroshotCLIP") is zsclip.ZeroshotCLIP and TRAINER_REGISTRY.get("ZeroshotCLIP2") is zsclip.ZeroshotCLIP2
    assert zsclip.ZeroshotCLIP.__bases__ == (TrainerX,)  # zsclip.py:52: TrainerX directly, no prompt-trainer layer
    assert issubclass(zsclip.ZeroshotCLIP2, zsclip.ZeroshotCLIP)  # zsclip.py:83
    for cls in (zsclip.ZeroshotCLIP, zsclip.ZeroshotCLIP2):
        assert "forward_backward" not in cls.__dict__ and "check_cfg" not in cls.__dict__
    assert not [k for k in vars(capi) if k.startswith("VARIANT_") and getattr(capi, k) > 7]  # a constructor, not a variant


def test_template_tables_are_the_references():
    from mudpt_amd import zsclip
    spec = json.load(open(os.path.join(R.GOLDEN, "zsclip_templates.json"), encoding="utf-8"))
    assert zsclip.CUSTOM_TEMPLATES == spec["CUSTOM_TEMPLATES"]
    assert list(zsclip.CUSTOM_TEMPLATES) == list(spec["CUSTOM_TEMPLATES"])
    assert list(zsclip.IMAGENET_TEMPLATES_SELECT) == spec["IMAGENET_TEMPLATES_SELECT"] and len(zsclip.IMAGENET_TEMPLATES_SELECT) == 7


def test_prompt_strings_replace_underscores():
    from mudpt_amd import zsclip
    names = ["face", "crocodile_head", "water_lily"]
    assert zsclip.prompt_strings(zsclip.CUSTOM_TEMPLATES["OxfordPets"], names) == [
        "a photo of a face, a type of pet.", "a photo of a crocodile head, a type of pet.", "a photo of a water lily, a type of pet."]
    assert zsclip.prompt_strings(zsclip.CUSTOM_TEMPLATES["DescribableTextures"], names)[1] == "crocodile head texture."
    with pytest.raises(KeyError):
        zsclip.ZeroshotCLIP.templates_for(None, "Synthetic")  # zsclip.py:61: an unknown dataset is a KeyError


def test_ensemble_has_7_templates_for_imagenet_and_8_otherwise_every_time():
    from mudpt_amd import zsclip
    for _ in range(2):  # the reference grows its class-level list on every build_model (zsclip.py:101-102)
        assert zsclip.ensemble_templates("ImageNet") == list(zsclip.IMAGENET_TEMPLATES_SELECT)
        t = zsclip.ZeroshotCLIP2.templates_for(None, "Caltech101")
        assert len(t) == 8 and t[:7] == list(zsclip.IMAGENET_TEMPLATES_SELECT) and t[7] == zsclip.CUSTOM_TEMPLATES["Caltech101"]
    assert len(zsclip.IMAGENET_TEMPLATES_SELECT) == 7
    # ImageNetSketch etc. are not "ImageNet": they get their own template appended, as in the reference
    assert len(zsclip.ensemble_templates("ImageNetSketch")) == 8


def test_fixture_templates_are_the_products(cases):
    from mudpt_amd import zsclip
    for case in cases.values():
        want = zsclip.ensemble_templates(case.dataset) if case.trainer == "ZeroshotCLIP2" else [zsclip.CUSTOM_TEMPLATES[case.dataset]]
        assert case.templates == want, case.name
        assert tuple(case.tokens.shape) == (len(want), len(case.classnames), 77) and case.tokens.dtype == torch.int32


def test_native_tokenizer_gives_the_recorded_ids(cases, tmp_path):
    from mudpt_amd import tokenizer, zsclip
    tok = tokenizer.BPETokenizer(R.merge_table_file(tmp_path))
    for case in cases.values():
        got = torch.stack([tok(zsclip.prompt_strings(t, case.classnames), 77) for t in case.templates])
        assert torch.equal(got, case.tokens), case.name
    assert any("_" in n for n in cases["zsclip_tiny"].classnames)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_the_reference(cases, name):
    """fp32 against fp32 on the same CPU: logits to 2e-5, text features to 2e-6."""
    case = cases[name]
    with torch.no_grad():
        txt = R.text_features(case.cfg, case.frozen, case.tokens)
        logits = R.forward(case.cfg, case.frozen, case.tokens, case.images)
        raw = R.image_features(case.cfg, case.frozen, case.images)
    e_txt, e_log = (txt - case.text_features).abs().max().item(), (logits - case.logits).abs().max().item()
    e_img = ((raw - case.image_features).norm(dim=-1) / case.image_features.norm(dim=-1)).max().item()
    print(f"{name}: text features {e_txt:.2e}, logits {e_log:.2e}, raw image features (relative) {e_img:.2e}")
    assert e_txt <= 2e-6 and e_log <= 2e-5
    assert e_img <= 1e-5
    assert (case.text_features.norm(dim=-1) - 1).abs().max().item() <= 1e-6


def test_ensemble_differs_from_the_single_template(cases):
    a, b = cases["zsclip_tiny"], cases["zsclip2_tiny"]
    assert a.classnames == b.classnames and (a.text_features - b.text_features).abs().max().item() > 1e-3


TINY = (32, 16, 192, 3, 3, 128, 3, 2, 77, 128)  # oracle TINY's shape fields


def test_frozen_constructor_refusals_do_not_touch_the_gpu(lib):
    h = C.c_void_p()
    assert lib.mudpt_create_frozen(None, C.byref(h)) == 1 and b"null" in lib.mudpt_last_error()
    cfg = capi.Config(*TINY, 0, 1, 6, 1, capi.F16, 0)
    assert lib.mudpt_create_frozen(C.byref(cfg), None) == 1
    bad_head = capi.Config(32, 16, 192, 3, 2, 128, 3, 2, 77, 128, 0, 1, 6, 1, capi.F16, 0)  # 192 / 2 heads: head dim 96
    assert lib.mudpt_create_frozen(C.byref(bad_head), C.byref(h)) == 1 and b"head dim must be 64" in lib.mudpt_last_error()
    bad_dtype = capi.Config(*TINY, 0, 1, 6, 1, 7, 0)
    assert lib.mudpt_create_frozen(C.byref(bad_dtype), C.byref(h)) == 1 and b"dtype" in lib.mudpt_last_error()
    no_classes = capi.Config(*TINY, 0, 1, 0, 1, capi.F16, 0)
    assert lib.mudpt_create_frozen(C.byref(no_classes), C.byref(h)) == 1
    # variant, n_ctx and depth are not read: values mudpt_create refuses pass the argument checks here
    for dtype in (capi.BF16, capi.F16, capi.F32):
        ok = capi.Config(*TINY, -3, 0, 6, 1, dtype, 8)
        rc = lib.mudpt_create_frozen(C.byref(ok), C.byref(h))
        if torch.cuda.is_available():
            assert rc == 0, lib.mudpt_last_error()
            assert lib.mudpt_param_count(h) == 0 and lib.mudpt_param_numel(h) == 0
            lib.mudpt_destroy(h)
        else:
            assert rc == 2, (rc, lib.mudpt_last_error())  # MUDPT_ERR_HIP: past the argument checks, no device to allocate on
    # mudpt_create is as it was: 8 is no variant
    v8 = capi.Config(*TINY, 2, 2, 6, 1, capi.F16, 8)
    assert lib.mudpt_create(C.byref(v8), C.byref(h)) == 1 and b"unknown variant 8" in lib.mudpt_last_error()


def test_frozen_entry_points_refuse_null_and_bad_sizes_on_the_host(lib):
    tok = (C.c_int32 * 8)()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    ti = C.cast(tok, C.c_void_p)
    assert lib.mudpt_set_text_tokens(None, ti, 1) == 1 and b"null" in lib.mudpt_last_error()
    assert lib.mudpt_text_features(None, p, None) == 1
    assert lib.mudpt_encode_image(None, p, 1, p, None) == 1
    # the kernel exports: null pointers, sizes below 1, d % 4 -- refused before any launch (the pointers are never read)
    assert lib.mudpt_embed_tokens(None, 8, ti, ti, p, p, 1, 4, None) == 1 and b"null" in lib.mudpt_last_error()
    assert lib.mudpt_embed_tokens(p, 8, None, ti, p, p, 1, 4, None) == 1
    assert lib.mudpt_embed_tokens(p, 8, ti, None, p, p, 1, 4, None) == 1
    assert lib.mudpt_embed_tokens(p, 8, ti, ti, None, p, 1, 4, None) == 1
    assert lib.mudpt_embed_tokens(p, 8, ti, ti, p, None, 1, 4, None) == 1
    for vocab, rows, d in ((0, 1, 4), (8, 0, 4), (8, -1, 4), (8, 1, 0), (8, 1, 6), (8, 1, 2)):
        assert lib.mudpt_embed_tokens(p, vocab, ti, ti, p, p, rows, d, None) == 1, (vocab, rows, d)
        assert b"embed_tokens" in lib.mudpt_last_error()
    q, r = C.cast((C.c_float * 8)(), C.c_void_p), C.cast((C.c_float * 8)(), C.c_void_p)
    assert lib.mudpt_feature_ensemble(None, q, r, 1, 4, 1, 1, 1, None) == 1 and b"null" in lib.mudpt_last_error()
    assert lib.mudpt_feature_ensemble(p, None, r, 1, 4, 1, 1, 1, None) == 1
    assert lib.mudpt_feature_ensemble(p, q, None, 1, 4, 1, 1, 1, None) == 1
    for Cn, e, T in ((0, 4, 1), (1, 0, 1), (1, 6, 1), (1, 4, 0)):
        assert lib.mudpt_feature_ensemble(p, q, r, Cn, e, 1, 1, T, None) == 1, (Cn, e, T)
    assert lib.mudpt_feature_ensemble(p, q, r, 1, 4, 1, 0, 1, None) == 1  # one template is the first and the last
    assert lib.mudpt_feature_ensemble(p, q, r, 1, 4, 1, 1, 2, None) == 1
    assert lib.mudpt_feature_ensemble(p, p, r, 1, 4, 1, 0, 2, None) == 1  # three different tables


def test_default_cfg_has_the_zero_shot_precision():
    from mudpt_amd import dassl_lite
    assert dassl_lite.default_cfg().TRAINER.ZSCLIP.PREC == "fp16"


def test_save_features_writes_the_linear_probes_file(tmp_path):
    """lpclip/feat_extractor.py:130-137: {output_dir}/{dataset}/{split}.npz with feature_list / label_list; the model is a stub."""
    from mudpt_amd import lpclip

    class Stub:
        shape = type("S", (), {"embed_dim": 4})()
        calls = 0

        def encode_image(self, img):
            self.calls += 1
            return img.reshape(img.shape[0], -1)[:, :4].double() * 2  # a dtype the extractor must bring to float32

    loader = [{"img": torch.arange(24.).reshape(2, 3, 2, 2), "label": torch.tensor([3, 1])},
              {"img": torch.arange(12.).reshape(1, 3, 2, 2) + 100, "label": torch.tensor([2], dtype=torch.int32)}]
    stub = Stub()
    feats, labels = lpclip.extract_features(stub, loader)
    assert stub.calls == 2 and feats.dtype == torch.float32 and labels.dtype == torch.int64
    assert tuple(feats.shape) == (3, 4) and labels.tolist() == [3, 1, 2]
    assert torch.equal(feats[2], torch.tensor([200., 202., 204., 206.]))
    path = lpclip.save_features(str(tmp_path / "out"), "Caltech101", "train", feats, labels)
    assert path == str(tmp_path / "out" / "Caltech101" / "train.npz")
    z = np.load(path)
    assert sorted(z.files) == ["feature_list", "label_list"]
    assert z["feature_list"].dtype == np.float32 and z["label_list"].dtype == np.int64
    assert np.array_equal(z["feature_list"], feats.numpy()) and np.array_equal(z["label_list"], labels.numpy())
    empty_f, empty_l = lpclip.extract_features(stub, [])
    assert tuple(empty_f.shape) == (0, 4) and empty_l.numel() == 0
