"""No-GPU checks of the C-ABI library: it loads, and exports every function include/mudpt.h declares."""
import ctypes as C
import os

import pytest

from mudpt_amd import capi, build


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


def test_header_functions_are_exported_and_bound(lib):
    declared = capi.declared_functions()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mudpt.h but not exported"
        assert name in capi.SIGNATURES, f"{name} has no ctypes signature in mudpt_amd/capi.py"
    assert sorted(capi.SIGNATURES) == declared


def test_abi_version(lib):
    assert lib.mudpt_abi_version() == capi.ABI_VERSION


def test_padded_len_is_host_only(lib):
    assert [lib.mudpt_attention_padded_len(L) for L in (1, 32, 33, 77, 201, 224)] == [32, 32, 64, 96, 224, 224]


def test_argument_errors_do_not_touch_the_gpu(lib):
    assert lib.mudpt_create(None, None) == 1
    assert b"null" in lib.mudpt_last_error()
    cfg = capi.Config(224, 16, 768, 12, 12, 512, 12, 8, 77, 512, 4, 0, 11, 4, 0)  # DEEP_PROMPT_DEPTH 0
    h = C.c_void_p()
    assert lib.mudpt_create(C.byref(cfg), C.byref(h)) == 1
    assert b"PROMPT_DEPTH should be > 0" in lib.mudpt_last_error()  # trainers/mudpt.py:52
    cfg = capi.Config(224, 16, 768, 12, 12, 512, 12, 8, 77, 512, 4, 12, 11, 4, 7)  # unknown dtype
    assert lib.mudpt_create(C.byref(cfg), C.byref(h)) == 1
    with pytest.raises(AssertionError):
        capi.check(1, "create")


def test_allreduce_entry_point_validates_before_touching_rccl(lib):
    assert lib.mudpt_allreduce_grads(None, None, None) == 1 and b"null model" in lib.mudpt_last_error()


def test_product_does_not_import_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, "mudpt_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.replace("no oracle", ""), f"{f} mentions the oracle: product must not depend on it"


def test_host_e4m3_conversion_matches_torch():
    """mudpt_e4m3_from_f32 (the conversion mudpt_set_weight applies to the frozen weights for the e4m3 second pass of the parity mode's
    vision tower) is OCP e4m3fn with round-to-nearest-even and saturation at +-448: bit for bit torch's float8_e4m3fn on in-range values."""
    import ctypes as C
    import torch
    from mudpt_amd import capi
    lib = capi.load()
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(20000, generator=g) * s for s in (1e-3, 0.02, 0.5, 4.0, 100.0)] +
                  [torch.tensor([0.0, -0.0, 448.0, -448.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 3 * 2.0 ** -10, 0.0625 + 2.0 ** -8, 17.0, 18.0, 19.0, 463.9, 240.0, 232.0])])
    for shift in (0, 3, -2):
        out = torch.zeros(x.numel(), dtype=torch.uint8)
        assert lib.mudpt_e4m3_from_f32(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.numel(), shift) == 0
        ref = (x * 2.0 ** shift).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        keep = ~((ref & 0x7f) == 0) | (out & 0x7f == 0)  # +-0: the sign of a value that rounds to zero is kept either way
        assert torch.equal(out[keep], ref[keep]), (out != ref).nonzero()[:5]
        assert (((out & 0x7f) == 0) == ((ref & 0x7f) == 0)).all()
    big = torch.tensor([464.0, 480.0, 1e6, -1e6, float("inf")])
    out = torch.zeros(5, dtype=torch.uint8)
    lib.mudpt_e4m3_from_f32(C.c_void_p(big.data_ptr()), C.c_void_p(out.data_ptr()), 5, 0)
    assert out.tolist() == [0x7e, 0x7e, 0x7e, 0xfe, 0x7e]  # saturates, never the NaN code


# Launchers that no single-kernel export calls by name, and why that is not a gap.  Keep it short: a launcher belongs here only if a
# direct float64 test reaches it some other way.
LAUNCHERS_WITHOUT_AN_EXPORT = {
    "launch_gemm_pp": "a form launch_gemm dispatches to (gemm_uses_pp); mudpt_gemm reaches it at the large shapes of test_gemm_pingpong_epilogues",
    "launch_attn_fwd_resident": "the FWD_RESIDENT form of launch_attn_fwd; test_attention_gpu_cases_reach_every_form holds mudpt_attention_fwd's cases to it",
    "launch_attn_bwd_resident": "the BWD_RESIDENT form of launch_attn_bwd; test_attention_gpu_cases_reach_every_form holds mudpt_attention_bwd's cases to it",
    "launch_sgd": "exported above the single-kernel section as mudpt_sgd_step, which test_model_gpu.py::test_sgd_step_matches_torch holds to torch.optim.SGD",
}


def test_every_launcher_is_called_from_a_test_export():
    """Every `int launch_*` kernels.h declares must be called from one of the single-kernel exports of model.cpp (the surface the float64 parity
    tests of tests/test_kernels_gpu.py, test_exact_gpu.py and test_movers_gpu.py drive), or stand in the allowlist above with its reason.  A new
    launcher that only the whole-model tests reach fails here."""
    import re
    csrc = os.path.join(os.path.dirname(capi.HERE), "mudpt_amd", "csrc")
    header = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "kernels.h")).read())
    launchers = sorted(set(re.findall(r"^\s*int\s+(launch_[a-z0-9_]+)\s*\(", header, flags=re.M)))
    assert len(launchers) >= 30, launchers
    model = open(os.path.join(csrc, "model.cpp")).read()
    marker = "// ---- single kernels "
    assert model.count(marker) == 1
    section = re.sub(r"//[^\n]*", "", model[model.index(marker):])
    exports = re.findall(r'extern "C" int (mudpt_[a-z0-9_]+)\s*\(', section)
    assert len(exports) >= 35 and set(exports) <= set(capi.SIGNATURES), exports
    called = set(re.findall(r"\b(launch_[a-z0-9_]+)\s*\(", section))
    missing = [f for f in launchers if f not in called and f not in LAUNCHERS_WITHOUT_AN_EXPORT]
    assert not missing, f"launchers no test export calls (add an export and a float64 test, or an allowlist entry with its reason): {missing}"
    stale = [f for f in LAUNCHERS_WITHOUT_AN_EXPORT if f not in launchers or f in called]
    assert not stale, f"allowlist entries that are no longer needed: {stale}"
    assert all(len(reason) > 20 for reason in LAUNCHERS_WITHOUT_AN_EXPORT.values())


W = (1 << 8) | (4 << 20)  # the window form: 4 rows from row 1 on
# (bwd, L, flags, sel) -> form of mudpt_attention_fwd / _bwd / _bwd_sel, as measured on the dispatch this table replaced
ATTN_FORM_TABLE = [
    (0, 201, 0, 0, "FWD_PERSISTENT"), (0, 224, 2, 0, "FWD_PERSISTENT"), (0, 77, 1, 0, "FWD_PAIR"), (0, 225, 0, 0, "FWD_RESIDENT"),
    (0, 581, 1, 0, "FWD_RESIDENT"), (0, 640, 0, 0, "FWD_RESIDENT"), (0, 581, 2, 0, "FWD_STAGED"), (0, 641, 0, 0, "FWD_STAGED"),
    (0, 4096, 1, 0, "FWD_STAGED"),
    (1, 77, 1, 0, "BWD_FUSED_W2"), (1, 77, 1 | 16, 0, "BWD_FUSED_W2"),
    (1, 96, 0, 0, "BWD_FUSED_W2"), (1, 96, 16, 0, "BWD_SWEEP"),
    (1, 97, 0, 0, "BWD_SWEEP"),
    (1, 128, 1, 0, "BWD_TWO"), (1, 128, 1 | 16, 0, "BWD_TWO"),
    (1, 201, 0, 0, "BWD_SWEEP"), (1, 201, 2, 0, "BWD_TWO"), (1, 201, 4, 0, "BWD_FUSED_W1"), (1, 201, 8, 0, "BWD_FUSED_W2"),
    (1, 201, 24, 0, "BWD_FUSED_W2"), (1, 201, W, 0, "BWD_TWO"), (1, 201, W | 8, 0, "BWD_TWO"), (1, 201, 0, 1, "BWD_TWO"),
    (1, 77, 1, 1, "BWD_TWO"),
    (1, 225, 0, 0, "BWD_RESIDENT"), (1, 225, 1, 0, "BWD_RESIDENT"),
    (1, 581, 0, 0, "BWD_RESIDENT"), (1, 581, 4, 0, "BWD_RESIDENT"), (1, 581, 8, 0, "BWD_RESIDENT"), (1, 581, 16, 0, "BWD_RESIDENT"),
    (1, 581, 2, 0, "BWD_STAGED"), (1, 581, W, 0, "BWD_STAGED"), (1, 581, 0, 1, "BWD_STAGED"),
    (1, 608, 1, 0, "BWD_RESIDENT"),
] + [(1, 609, c | f, s, "BWD_STAGED") for c in (0, 1) for f in (0, 2, 4, 8, 16, W) for s in (0, 1)]


def test_attention_form_table(lib):
    """Which kernels a launch runs is host arithmetic (attn_form, exported as mudpt_attention_form): every form computes the same numbers,
    so only this table notices a wrong edit to the dispatch before the benchmark does."""
    header = open(capi.HEADER_PATH).read()
    for code, name in enumerate(capi.ATTN_FORMS):
        assert f"#define MUDPT_ATTN_{name} {code} " in header, name
    for bwd, L, flags, sel, want in ATTN_FORM_TABLE:
        got = lib.mudpt_attention_form(bwd, L, flags, sel)
        assert got == capi.ATTN_FORMS.index(want), (bwd, L, flags, sel, want, capi.ATTN_FORMS[got] if got >= 0 else got)
    assert [lib.mudpt_attention_form(b, L, 0, 0) for b in (0, 1) for L in (0, 4097)] == [-1] * 4


def test_attention_gpu_cases_reach_every_form(lib):
    """The (case, flags) pairs the attention tests of test_kernels_gpu.py run reach all ten forms, the two resident launchers among them."""
    from tests.helpers import attention_test_launches
    reached = {lib.mudpt_attention_form(*call) for call in attention_test_launches()}
    assert reached == set(range(len(capi.ATTN_FORMS))), sorted(capi.ATTN_FORMS[i] for i in set(range(10)) - reached)


def test_patchify_cases_wrap_every_grid_stride_loop():
    """Arithmetic only, from the launchers' formulas: among the shapes test_movers_gpu.py runs, at least one per patchify kernel has more
    work than its capped grid holds in one pass (B = 64 vector form, B = 16 at p = 14, B = 128 split form at p = 16)."""
    from tests.helpers import PATCH_CASES, PATCH_SPLIT_CASES, patchify_threads
    vector = lambda p, ldk: p % 8 == 0 and ldk == 3 * p * p  # noqa: E731
    over = lambda form, case: patchify_threads(form, *case)[0] > patchify_threads(form, *case)[1]  # noqa: E731
    assert any(vector(c[2], c[3]) and over("vector", c) for c in PATCH_CASES)
    assert any(not vector(c[2], c[3]) and over("any", c) for c in PATCH_CASES)
    assert any(over("split", c) for c in PATCH_SPLIT_CASES)
