"""CoOp (trainers/coop.py) without a GPU: the test-local restatement against the fixtures of the reference's own modules, the native
tokenizer's name lengths, the config defaults and the new C ABI entries' argument checks."""
import gzip
import json
import os

import pytest
import torch

from tests import coop_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=R.FIXTURES)
def case(request):
    return R.CoopCase(request.param)


def test_fixture_shapes_and_recipe(case):
    img = case.images.double()
    assert abs(img.sum().item() - float(case.z["images_checksum"][0])) <= 1e-9 * img.abs().sum().item()
    C, n, d = len(case.classnames), case.cfg.n_ctx, case.cfg.t_width
    assert tuple(case.ctx.shape) == ((C,) if case.csc else ()) + (n, d)
    assert case.dctx.shape == case.ctx.shape
    # every context row lies before the EOT row (what mudpt_set_class_prompts checks)
    assert all(1 + n + nl <= int(e) for nl, e in zip(case.name_lens, case.eot))


def test_restatement_reproduces_the_reference(case):
    with torch.no_grad():
        logits = R.forward(case.cfg, case.frozen, case.ctx, case.class_embedding, case.eot, case.name_lens, case.position, case.images)
    assert (logits - case.logits).abs().max().item() <= 1e-4
    loss, _, dctx = R.forward_backward(case.cfg, case.frozen, case.ctx, case.class_embedding, case.eot, case.name_lens, case.position,
                                       case.images, case.labels)
    assert abs(loss.item() - case.loss) <= 1e-5
    assert (dctx - case.dctx).abs().max().item() <= 1e-4 * case.dctx.abs().max().item() + 1e-9


def test_prompt_rows_move_with_the_position():
    """construct_prompts keeps rows from 1 + n + name_len on in place and puts the context where ctx_rows says."""
    C, L, d, n = 3, 12, 4, 5
    emb = torch.arange(C * L * d, dtype=torch.float32).view(C, L, d)
    ctx = -torch.arange(1, C * n * d + 1, dtype=torch.float32).view(C, n, d)
    lens = [1, 2, 3]
    for pos in ("end", "middle", "front"):
        p = R.construct_prompts(ctx, emb, n, lens, pos)
        assert p.shape == emb.shape
        for c in range(C):
            for j, r in enumerate(R.ctx_rows(n, lens[c], pos)):
                assert torch.equal(p[c, r], ctx[c, j])
            assert torch.equal(p[c, 1 + n + lens[c]:], emb[c, 1 + n + lens[c]:])
            assert torch.equal(p[c, 0], emb[c, 0])


def test_native_tokenizer_name_lengths_match_the_reference(tmp_path):
    """name_lens = len(_tokenizer.encode(name)) (coop.py:80) by the native BPE tokenizer, on the merge-table rows the names use
    (tests/golden/coop_name_merges.json; the other ranks are pairs no byte string can form, as in tests/test_tokenizer_cpu.py)."""
    from mudpt_amd import tokenizer
    vocab = os.environ.get("MUDPT_BPE_VOCAB")
    if not vocab:
        spec = json.load(open(os.path.join(HERE, "golden", "coop_name_merges.json"), encoding="utf-8"))
        lines = ["#version: 0.2"] + [spec["merges"].get(str(r), f"一{r} 丁") for r in range(spec["n_merges"])]
        vocab = str(tmp_path / tokenizer.VOCAB_FILE)
        with gzip.open(vocab, "wt", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    tok = tokenizer.BPETokenizer(vocab)
    for name in R.FIXTURES:
        c = R.CoopCase(name)
        assert [len(tok.encode(n.replace("_", " "))) for n in c.classnames] == c.name_lens, name


def test_default_cfg_has_the_coop_node():
    from mudpt_amd import dassl_lite
    cc = dassl_lite.default_cfg().TRAINER.COOP
    assert (cc.N_CTX, cc.CTX_INIT, cc.PREC, cc.CSC, cc.CLASS_TOKEN_POSITION) == (16, "", "fp16", False, "end")  # train.py:83-88


def test_abi_entries_reject_a_null_handle():
    import ctypes as C
    from mudpt_amd import capi
    lib = capi.load()
    assert lib.mudpt_abi_version() == capi.ABI_VERSION == 7
    lens = (C.c_int32 * 2)(1, 2)
    assert lib.mudpt_set_class_token_position(None, capi.CLASS_TOKEN_MIDDLE, lens) == 1
    assert lib.mudpt_coop_dctx(0, None, None, None, None, 4, 2, 64, 0, 1.0, None) == 1
    assert b"coop_dctx" in lib.mudpt_last_error()
