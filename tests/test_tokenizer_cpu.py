"""The native BPE tokenizer (mudpt_amd/tokenizer.py) against token ids recorded from the reference's own tokenizer
(tests/golden/tokenizer_cases.json, written by tests/golden/gen_golden.py --tokenizer-only).

The merge table is data that ships with CLIP, not with this repository.  The tests build one from
tests/golden/tokenizer_merges.json: the rows of CLIP's table that these strings use, at their ranks, every other rank a pair no
byte string can form (why that merges exactly as the full table: gen_golden.py run_tokenizer_merges).  MUDPT_BPE_VOCAB, if set,
names a full table to test against instead."""
import gzip
import json
import os

import pytest
import torch

from mudpt_amd import tokenizer

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    if os.environ.get("MUDPT_BPE_VOCAB"):
        return os.environ["MUDPT_BPE_VOCAB"]
    spec = json.load(open(os.path.join(HERE, "golden", "tokenizer_merges.json"), encoding="utf-8"))
    merges = spec["merges"]
    lines = ["#version: 0.2"] + [merges.get(str(r), f"\u4e00{r} \u4e01") for r in range(spec["n_merges"])]  # U+4E00: never a byte symbol
    path = tmp_path_factory.mktemp("bpe") / tokenizer.VOCAB_FILE
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


def test_ids_match_the_reference_tokenizer(vocab):
    tok = tokenizer.BPETokenizer(vocab)
    spec = json.load(open(os.path.join(HERE, "golden", "tokenizer_cases.json"), encoding="utf-8"))
    assert len(spec["cases"]) >= 25
    for c in spec["cases"]:
        row = tok([c["text"]], spec["context_length"], truncate=spec["truncate"])[0]
        n = len(c["ids"])
        assert row[:n].tolist() == c["ids"], c["text"]
        assert (row[n:] == 0).all()
        assert int(row[n - 1]) == 49407
    assert tok.sot_id == 49406 and tok.eot_id == 49407


def test_too_long_prompt_raises_like_clip_tokenize(vocab):
    tok = tokenizer.BPETokenizer(vocab)
    with pytest.raises(RuntimeError, match="too long for context length"):  # clip/clip.py:235
        tok(["word " * 100])
    out = tok(["word " * 100], truncate=True)
    assert out.shape == (1, 77) and out[0, -1] == 49407


def test_missing_vocab_is_an_explicit_error(tmp_path, monkeypatch):
    import importlib.util
    if importlib.util.find_spec("clip") is not None:
        pytest.skip("a clip package with its merge table is importable here")
    monkeypatch.delenv("MUDPT_BPE_VOCAB", raising=False)
    with pytest.raises(RuntimeError, match="merge table"):
        tokenizer.find_vocab(str(tmp_path / "nope.gz"), near=str(tmp_path / "ViT-B-16.pt"))


def test_benchmark_prompts_agree_with_the_recorded_ids(vocab):
    from mudpt_amd import synth
    tok = tokenizer.BPETokenizer(vocab)
    prompts = [f"a photo of a {n}." for n in synth.BENCH_CLASSNAMES]
    assert torch.equal(tok(prompts), synth.bench_tokenized_prompts())
