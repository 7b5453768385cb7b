"""No-GPU checks of the text tower's sequence layout rule (plan_text_layout in model.cpp, exported as mudpt_text_layout_plan): what
mudpt_set_class_prompts and mudpt_set_text_tokens plan for a set of EOT positions, against an independent statement of the rule."""
import ctypes as C
import itertools
import os

import pytest

from mudpt_amd import build, capi

CTX = 77


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


def plan(lib, eot, ctx_len=CTX, n_prompt=0, heads=8, trim=1, buckets=3, cost=1024, allow=1):
    """-> cls, first_row, bucket_len (lists of n_cls), buckets, rows, max_len."""
    n = len(eot)
    outs = [(C.c_int32 * k)(*([-7] * k)) for k in (n, n, n, 1, 1, 1)]
    ptr = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    rc = lib.mudpt_text_layout_plan(ptr((C.c_int32 * n)(*eot)), n, ctx_len, n_prompt, heads, trim, buckets, cost, allow, *[ptr(a) for a in outs])
    assert rc == 0, lib.mudpt_last_error()
    return list(outs[0]), list(outs[1]), list(outs[2]), outs[3][0], outs[4][0], outs[5][0]


def search(lens, max_buckets, cost):
    """The cheapest way to cut the sorted distinct lengths into k <= max_buckets contiguous groups, each run to its longest member, by trying
    every set of cuts: {k: fewest rows with exactly k buckets}."""
    distinct = sorted(set(lens))
    count = [lens.count(v) for v in distinct]
    nd, rows = len(distinct), {}
    for k in range(1, min(max_buckets, nd) + 1):
        rows[k] = min(sum(sum(count[a:b]) * distinct[b - 1] for a, b in zip((0,) + cuts, cuts + (nd,)))
                      for cuts in itertools.combinations(range(1, nd), k - 1))
    return rows


# 64 classes with EOT positions 4 .. 31 in a scrambled order (every value at least twice, so the sort has ties to keep stable): 64 x 32 rows are
# exactly the threshold of 2048; one class fewer, 63 x 32 = 2016, is below it
SPREAD = [4 + (i * 37 % 64) * 28 // 64 for i in range(64)]
# 96 classes in three clusters of lengths, interleaved; EOT 1 and 2 are short enough for the n_prompt + 2 floor to bind at n_prompt = 4
CLUSTERS = [v for i in range(32) for v in ((1, 2, 7, 8, 9)[i % 5], (19, 20, 21)[i % 3], (44, 45)[i % 2])]
EQUAL = [30] * 96
CASES = {"spread64": (SPREAD, (1, 2, 3)), "spread63": (SPREAD[:63], (1, 2, 3)), "clusters96": (CLUSTERS, (1, 2, 3, 12)), "equal96": (EQUAL, (1, 2, 3, 12))}


def test_the_cases_are_what_they_claim():
    assert sorted(set(SPREAD)) == list(range(4, 32)) and min(SPREAD.count(v) for v in set(SPREAD)) >= 2 and SPREAD != sorted(SPREAD)
    assert len(SPREAD) * (max(SPREAD) + 1) == 2048 and len(SPREAD[:63]) * (max(SPREAD[:63]) + 1) == 2016
    assert len(CLUSTERS) == 96 and set(CLUSTERS) == {1, 2, 7, 8, 9, 19, 20, 21, 44, 45} and len(set(max(e + 1, 6) for e in CLUSTERS)) < len(set(CLUSTERS))
    assert all(len(set(max(e + 1, n + 2) for e in eot)) < 12 for eot, b in CASES.values() if 12 in b for n in (0, 4))  # 12 buckets: more than distinct lengths


@pytest.mark.parametrize("n_prompt", (0, 4))
@pytest.mark.parametrize("cost", (0, 1024))
@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_matches_the_rule(lib, case, cost, n_prompt):
    eot, bucket_counts = CASES[case]
    n = len(eot)
    lens = [max(e + 1, n_prompt + 2) for e in eot]
    Le = max(lens)
    for max_buckets, trim, allow in [(b, 1, 1) for b in bucket_counts] + [(3, 0, 1), (3, 1, 0)]:
        cls, first, blen, k, rows, max_len = plan(lib, eot, n_prompt=n_prompt, trim=trim, buckets=max_buckets, cost=cost, allow=allow)
        what = (case, cost, n_prompt, max_buckets, trim, allow)
        may_bucket = allow and trim and max_buckets > 1 and n * Le >= 2048
        if may_bucket:
            by_k = search(lens, max_buckets, cost)
            best = min(r + j * cost for j, r in by_k.items())
            want_k = min(j for j, r in by_k.items() if r + j * cost == best)  # among bucket counts of equal cost the smallest
        else:
            by_k, best, want_k = None, n * (Le if trim else CTX) + cost, 1
        assert k == want_k and rows + k * cost == best, what
        assert max_len == (Le if trim else CTX) == max(blen), what
        assert sorted(cls) == list(range(n)), what
        if k > 1:
            assert cls == sorted(range(n), key=lambda c: lens[c]), what  # the stable sort by kept length
            assert len(set(blen)) == k and blen == sorted(blen), what
            for L in set(blen):  # a bucket runs to its longest member
                assert L == max(lens[c] for c, b in zip(cls, blen) if b == L), what
        else:
            assert cls == list(range(n)) and set(blen) == {max_len}, what  # one bucket: the caller's order
        assert all(b >= lens[c] for c, b in zip(cls, blen)), what
        assert first[0] == 0 and all(first[q + 1] == first[q] + blen[q] for q in range(n - 1)) and rows == first[-1] + blen[-1] == sum(blen), what


def test_threshold_and_knobs_decide_as_documented(lib):
    """The cases above reach both sides of every switch: at the 2048-row threshold free buckets are taken and one class fewer they are not; a
    bucket's price of 1024 rows keeps the 64 spread prompts in one bucket and the clusters in several; more buckets than distinct lengths gives
    one per length when they are free."""
    assert plan(lib, SPREAD, cost=0)[3] == 3 and plan(lib, SPREAD[:63], cost=0)[3] == 1
    assert plan(lib, SPREAD, cost=1024)[3] == 1 and plan(lib, SPREAD, cost=0, buckets=2)[3] == 2
    assert plan(lib, CLUSTERS, cost=1024)[3] > 1 and plan(lib, CLUSTERS, cost=0, buckets=12)[3] == len(set(CLUSTERS))
    assert plan(lib, CLUSTERS, cost=0, buckets=12, n_prompt=4)[3] == len(set(CLUSTERS)) - 1  # EOT 1 and 2 both keep the floor's 6 rows
    assert plan(lib, EQUAL, cost=0, buckets=12)[3:] == (1, 96 * 31, 31)
    assert plan(lib, [1, 5], n_prompt=4)[2:] == ([6, 6], 1, 12, 6) and plan(lib, [1, 5], n_prompt=0)[2:] == ([6, 6], 1, 12, 6)
    assert plan(lib, [1, 2], n_prompt=4)[2:] == ([6, 6], 1, 12, 6) and plan(lib, [1, 2], n_prompt=0)[2:] == ([3, 3], 1, 6, 3)  # the floor binds
    assert plan(lib, [0], n_prompt=0)[2:] == ([2], 1, 2, 2)


def test_plan_refuses_bad_arguments_before_writing(lib):
    n = 4
    eot = (C.c_int32 * n)(5, 6, 7, 8)
    outs = [(C.c_int32 * n)(*([-7] * n)) for _ in range(6)]
    ptr = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    good = [ptr(eot), n, CTX, 0, 8, 1, 3, 1024, 1] + [ptr(a) for a in outs]
    assert lib.mudpt_text_layout_plan(*good) == 0
    for a in outs:
        a[:] = [-7] * n
    bad = {"null": [dict([(i, None)]) for i in (0, 9, 10, 11, 12, 13, 14)], "n_cls": [{1: 0}, {1: -3}], "heads": [{4: 0}], "n_prompt": [{3: -1}, {3: CTX - 1}]}
    for word, changes in bad.items():
        for change in changes:
            args = [change.get(i, v) for i, v in enumerate(good)]
            assert lib.mudpt_text_layout_plan(*args) == 1, (word, change)
            assert word.encode() in lib.mudpt_last_error(), (word, lib.mudpt_last_error())
            assert all(list(a) == [-7] * n for a in outs), (word, change)
    for value in (-1, CTX):
        eot[2] = value
        assert lib.mudpt_text_layout_plan(*good) == 1 and b"eot[2]" in lib.mudpt_last_error()
        assert all(list(a) == [-7] * n for a in outs)
