"""No-GPU checks of the C-ABI library: it loads, and exports every function include/mudpt.h declares."""
import ctypes as C
import os
import re

import pytest

from mudpt_amd import capi, build


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


def test_header_functions_are_exported_and_bound(lib):
    """capi.py binds from include/mudpt.h itself: every declaration is exported by the library and bound with the header's types and order."""
    declared = capi.declared_functions()
    loose = re.findall(r"\b(mudpt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(capi.HEADER_PATH).read(), flags=re.S))  # an independent, looser scan
    assert len(declared) >= 20 and declared == sorted(set(loose)), "a declaration the parser did not read"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mudpt.h but not exported"
        fn, (res, params) = getattr(lib, name), capi.DECLARATIONS[name]
        assert fn.restype is res and list(fn.argtypes) == [t for _, t in params] == capi.SIGNATURES[name][1], name


def test_header_parser_vocabulary():
    """One declaration per type the header may use -> its ctypes; comments and preprocessor lines are no declarations; an unknown type raises."""
    text = """/* int mudpt_in_a_comment(int x); */
    #define MUDPT_NOT_A_FUNCTION(x) 1
    typedef struct mudpt_model mudpt_model;
    int mudpt_a(void);
    const char* mudpt_b(int i, int32_t j, int64_t k, float f, size_t n);
    size_t mudpt_c(const mudpt_model* m, const char* key, const char** name, mudpt_model** out,
                   int64_t shape[3], const float* x, uint8_t* bytes, void* stream);"""
    i32, vp = C.c_int32, C.c_void_p
    assert capi.parse_header(text) == {
        "mudpt_a": (i32, []), "mudpt_b": (C.c_char_p, [("i", i32), ("j", i32), ("k", C.c_int64), ("f", C.c_float), ("n", C.c_size_t)]),
        "mudpt_c": (C.c_size_t, [("m", vp), ("key", C.c_char_p), ("name", vp), ("out", vp), ("shape", vp), ("x", vp), ("bytes", vp), ("stream", vp)])}
    for declaration, word in (("int mudpt_x(double v);", "double v"), ("int mudpt_x(unsigned n);", "unsigned n"), ("double mudpt_x(void);", "double"),
                              ("int mudpt_x(mudpt_config cfg);", "mudpt_config cfg"), ("int mudpt_x(const unsigned char* p);", "unsigned char"),
                              ("int mudpt_ok(void);\nint mudpt_x(void (*cb)(int));", "not read")):  # a form the parser cannot consume is no silent gap
        with pytest.raises(capi.MudptError, match="mudpt_x.*" + word):
            capi.parse_header(declaration)
    assert capi.parse_defines("#define MUDPT_X_B 1  /* one */\n#define MUDPT_X_A 0\n#define MUDPT_Y 7\n", "MUDPT_X_") == {"B": 1, "A": 0}
    assert (capi.BF16, capi.F16, capi.F32, capi.VARIANT_UUMUDPT, capi.CLASS_TOKEN_FRONT, capi.CP_TEXT, capi.FWD_TRAINING) == (0, 1, 2, 7, 2, 2, 2)
    assert capi.ATTN_FORMS[:2] == ("FWD_PAIR", "FWD_PERSISTENT") and capi.GEMM_FORMS[::9] == ("PP", "SPLITK_K64") and len(capi.ATTN_FORMS) == len(capi.GEMM_FORMS) == 10


def test_call_by_name_refuses_an_unknown_keyword(lib):
    import torch
    for kw, word in (({"Lp": 33}, "Lp"), ({"L": torch.zeros(1)}, "L")):  # a keyword the export does not have; a tensor for a scalar parameter
        with pytest.raises(TypeError, match="mudpt_attention_padded_len.*" + word):
            capi.call("mudpt_attention_padded_len", **kw)
    assert (capi.call("mudpt_attention_padded_len", L=33), capi.call("mudpt_attention_padded_len")) == (64, lib.mudpt_attention_padded_len(0))  # omitted scalar: 0
    assert capi.call("mudpt_create") == 1 and b"null" in lib.mudpt_last_error()  # omitted pointers are null


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
    import torch
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


def model_set_names(source):
    """The knob names mudpt_model_set compares its argument against: `strcmp(name, "x")` as it stands, `strcmp(k, "x")` behind the tower
    prefix ("vis_" / "txt_"; only "txt_" where the comparison is guarded by `t == &m->txt`)."""
    body = source[source.index('extern "C" int mudpt_model_set('):]
    body = re.sub(r"//[^\n]*", "", body[:body.index("unknown knob")])
    names = set(re.findall(r'strcmp\(name, "(\w+)"\)', body))
    for txt_only, k in re.findall(r'(t == &m->txt && )?!strcmp\(k, "(\w+)"\)', body):
        names |= {"txt_" + k} | (set() if txt_only else {"vis_" + k})
    return names


def header_knob_table(header):
    """The names in the first column of the knob table above mudpt_model_set's declaration."""
    table = header[header.index(" *   knob               default"):header.index("int mudpt_model_set(")]
    return set(re.findall(r"^ \*   ([a-z][a-z0-9_]*) ", table, flags=re.M)) - {"knob"}


def test_every_model_knob_is_documented_and_held_by_a_test():
    """Every name mudpt_model_set accepts has a row in MODEL_KNOBS (tests/helpers.py) that names the test holding it, or says why none does,
    and a row in the knob table of include/mudpt.h; neither table lists a name the library does not accept.  A new knob fails here until
    it has its settings, its test and its line of documentation."""
    from tests.helpers import KNOB_DEFAULTS, MODEL_KNOBS, knob_settings
    root = os.path.dirname(capi.HERE)
    accepted = model_set_names(open(os.path.join(root, "mudpt_amd", "csrc", "model.cpp")).read())
    assert len(accepted) >= 22 and {"gemm_variant", "gelu_q8", "txt_split", "vis_lo", "txt_exact_attn"} <= accepted, sorted(accepted)
    assert "vis_split" not in accepted  # "split" is the text tower's older name for "lo" alone
    documented = header_knob_table(open(capi.HEADER_PATH).read())
    assert not accepted - set(MODEL_KNOBS), f"knobs without a row in MODEL_KNOBS: {sorted(accepted - set(MODEL_KNOBS))}"
    assert not set(MODEL_KNOBS) - accepted, f"MODEL_KNOBS rows the library does not accept: {sorted(set(MODEL_KNOBS) - accepted)}"
    assert not accepted - documented, f"knobs missing from the table in include/mudpt.h: {sorted(accepted - documented)}"
    assert not documented - accepted, f"rows of the header's table the library does not accept: {sorted(documented - accepted)}"
    for name, (settings, held_by, why_not) in MODEL_KNOBS.items():
        assert bool(held_by) != bool(why_not) and (held_by or len(why_not) > 20), name
        for held in held_by.split(", ") if held_by else ():  # every test it names exists
            path, _, test = held.partition("::")
            assert f"\ndef {test}(" in open(os.path.join(root, path)).read(), (name, held)
        for s in settings:  # a setting moves its own knob off the dtype's default, and whatever it moves can be set back
            assert s.sets[0][0] == name and (s.construct or all(k in KNOB_DEFAULTS[s.dtype] for k, _ in s.sets)), s
            assert s.sets[0][1] != KNOB_DEFAULTS[s.dtype].get(name, 1 if name == "txt_split" else None), s
            assert "test_knobs_gpu.py" in held_by, (name, "settings are run by test_knobs_gpu.py")
    # the settings the GPU module runs: both attention forms, the window, three kernel choices and the streams in both dtypes; the fp16 text tower's split
    assert {s.sets[0] for s in knob_settings(dtype="bf16")} == {("gemm_variant", 12), ("gemm_variant", 1), ("gemm_variant", 10), ("attn_window", 0),
                                                                ("attn_two_kernels", 1), ("attn_fused_w1", 1), ("lp_grad", 0), ("lp_upd", 0), ("gelu_q8", 0)}
    assert {s.sets[0] for s in knob_settings(dtype="fp16")} == {("gemm_variant", 12), ("gemm_variant", 1), ("gemm_variant", 10), ("attn_window", 0),
                                                                ("attn_two_kernels", 1), ("attn_fused_w1", 1), ("lp_grad", 1), ("lp_upd", 1), ("gelu_q8", 1),
                                                                ("txt_split", 0), ("txt_lo", 0), ("txt_sites", 5)}
    # the parity mode's own knobs on a dtype "fp32" handle: pairs in the vision tower, its fp32 attention, both (round 3's exact mode), fewer
    # split sites, the text tower's attention back in fp16
    assert [s.sets for s in knob_settings(dtype="fp32")] == [(("vis_lo", 1),), (("vis_sites", 12),), (("vis_exact_attn", 1),),
                                                             (("vis_exact_attn", 1), ("vis_lo", 1)), (("txt_exact_attn", 0),)]
    assert set(KNOB_DEFAULTS) == {"fp16", "bf16", "fp32"} and all(KNOB_DEFAULTS["fp32"][k] == v for k, v in KNOB_DEFAULTS["fp16"].items() if k != "lp_grad")
    assert all(s.lowers == (s.dtype == "fp16" and s.sets[0][0] in ("lp_grad", "lp_upd", "gelu_q8", "txt_split", "txt_lo", "txt_sites")) for s in knob_settings())


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


def test_attention_gpu_cases_reach_every_instantiation(lib):
    """A form is not a kernel: for L <= 224 every whole-pair form is instantiated per NC = padded length / 32 and per mask.  The cases of
    test_attention_forms_gpu.py take the form their tables name, and the (form, NC, mask) they reach are all 9 x 7 = 63; the multi-pair cases
    hold more pairs than their persistent kernel has resident workgroups at 256 units, with a ragged last round."""
    from tests import helpers as h
    reached = set()
    for bwd, L, flags, sel, want in h.attention_form_launches():
        got = lib.mudpt_attention_form(bwd, L, flags, sel)
        assert got == capi.ATTN_FORMS.index(want), (bwd, L, flags, sel, want, capi.ATTN_FORMS[got] if got >= 0 else got)
        if L <= 224:
            reached.add((want, lib.mudpt_attention_padded_len(L) // 32, flags & 1))
    whole_pair = [("FWD_PERSISTENT", 0), ("FWD_PAIR", 1), ("BWD_SWEEP", 0)] + [(f, m) for f in ("BWD_TWO", "BWD_FUSED_W2", "BWD_FUSED_W1") for m in (0, 1)]
    want = {(f, NC, m) for f, m in whole_pair for NC in h.ATTN_NCS}
    assert len(want) == 63 and reached == want, sorted(want - reached) + sorted(reached - want)
    # every instance length is there, L = 1 and the lengths around an all-padding last tile among them
    assert {L for _, L, _, _ in h.ATTN_INSTANCE_CASES} >= {1, 16, 17, 32, 33, 208, 209, 224}
    assert [h.attn_fwd_cap(NC, 256) for NC in h.ATTN_NCS] == [2304, 1024, 768, 512, 256, 256, 256]
    for W2 in (2, 1):
        assert [h.attn_fused_cap(NC, W2, 256) for NC in h.ATTN_NCS] == [1024, 1024, 768, 512, 256, 256, 256]
    kernels = set()
    for c in h.ATTN_MULTI_PAIR_CASES:
        assert lib.mudpt_attention_padded_len(c.L) // 32 == c.NC
        for ncu in (256, 304, 64):
            pairs, cap = c.batch(ncu) * c.H, c.cap(ncu)
            assert cap < pairs <= 1.5 * cap and pairs % cap != 0, (c, ncu, pairs, cap)
        kernels.add((c.kernel, c.NC))
    assert kernels == {(k, NC) for k in ("fwd", "fused_w2", "fused_w1") for NC in h.ATTN_NCS}
    assert {(L, causal) for _, L, _, causal in h.ATTN_LONG_CASES} >= {(4096, False), (1025, True)}


def test_attention_float64_reference_is_the_gradient_of_attn64():
    """helpers.attn64_fwd_bwd (explicit sums, so that 4096 rows need no autograd graph) against autograd through attn64; with round_to it moves
    by roundings of T only."""
    import torch
    from tests.helpers import attn64, attn64_fwd_bwd
    g = torch.Generator().manual_seed(5)
    for L, H, causal in ((1, 2, True), (17, 2, False), (49, 3, True)):
        qkv = torch.randn(2, L, 3 * H * 64, generator=g).double().requires_grad_(True)
        dout = torch.randn(2, L, H * 64, generator=g).double()
        ref = attn64(qkv, H, causal)
        (dref,) = torch.autograd.grad(ref, qkv, dout)
        out, lse, dqkv = attn64_fwd_bwd(qkv.detach(), dout, H, causal)
        torch.testing.assert_close(out, ref.detach(), atol=1e-13, rtol=1e-12)
        torch.testing.assert_close(dqkv, dref, atol=1e-12, rtol=1e-11)
        assert lse.shape == (2, H, L)
        _, _, emu = attn64_fwd_bwd(qkv.detach(), dout, H, causal, round_to=torch.float16)
        assert 0 < (emu - dref).abs().max().item() <= 16 * 2.0 ** -11 * dref.abs().max().item()


def test_patchify_cases_wrap_every_grid_stride_loop():
    """Arithmetic only, from the launchers' formulas: among the shapes test_movers_gpu.py runs, at least one per patchify kernel has more
    work than its capped grid holds in one pass (B = 64 vector form, B = 16 at p = 14, B = 128 split form at p = 16)."""
    from tests.helpers import PATCH_CASES, PATCH_SPLIT_CASES, patchify_threads
    vector = lambda p, ldk: p % 8 == 0 and ldk == 3 * p * p  # noqa: E731
    over = lambda form, case: patchify_threads(form, *case)[0] > patchify_threads(form, *case)[1]  # noqa: E731
    assert any(vector(c[2], c[3]) and over("vector", c) for c in PATCH_CASES)
    assert any(not vector(c[2], c[3]) and over("any", c) for c in PATCH_CASES)
    assert any(over("split", c) for c in PATCH_SPLIT_CASES)


def _g(epi, M, N, K, want, slices=1, variant=0, ldo0=None, ldo1=None, ldaux=None, lo_mode=0, ncu=256):
    """One row of GEMM_FORM_TABLE: mudpt_gemm_form's arguments (contiguous outputs unless a stride is given) and the form it must name."""
    return (epi, M, N, K, N if ldo0 is None else ldo0, N if ldo1 is None else ldo1, N if ldaux is None else ldaux, lo_mode, variant, ncu), (want, slices)


S16 = 0x10000  # bit 16 of mudpt_gemm's variant: scratch for split K is available
# Worked out by hand from the dispatch this table replaced (gemm_uses_pp -> split_k_slices -> launch_epi, with small_tiles and deep_k_tiles), at
# 256 compute units unless a row says otherwise.  t64 / t128 / t256 = tiles of 64 x 64 / 128 x 128 / 256 x 256 (ragged edges count as tiles).
GEMM_FORM_TABLE = [
    # M * N against 256 * 128 * 512 = 16 777 216 (epilogue 2 never takes the persistent kernel); below it t64 = 4096 and t128 = 1024 leave 128 x 128
    _g(2, 16384, 1024, 192, "T256x256"), _g(2, 16383, 1024, 192, "T128x128"), _g(2, 16384, 1024, 192, "T128x256", variant=2),
    _g(2, 16384, 1024, 192, "T256x128", variant=4), _g(2, 16383, 1024, 192, "T128x128", variant=2),
    # small_tiles: t64 = 1280 | 1281 (= 61 x 21) at K > 512, and t64 = 2560 | 2561 (= 197 x 13) with K = 512 | 576
    _g(2, 5120, 1024, 576, "T64x64"), _g(2, 3904, 1344, 576, "T128x128"),
    _g(2, 10240, 1024, 512, "T64x64"), _g(2, 10240, 1024, 576, "T128x128"), _g(2, 12608, 832, 512, "T128x128"),
    # deep_k_tiles: t64 = 512 | 513 (= 27 x 19) against 2 ncu, K % 128, a split operand, knob 12
    _g(2, 2048, 1024, 128, "T64x64_K128"), _g(2, 2048, 1024, 192, "T64x64"), _g(2, 1728, 1216, 128, "T64x64"),
    _g(2, 2048, 1024, 128, "T64x64", lo_mode=1), _g(2, 2048, 1024, 128, "T64x64", variant=12),
    # t128 = 128 | 129 (= 43 x 3) decides ring against 128 x 128 once small_tiles is out of the way (knob 1 below the large-problem size)
    _g(5, 2048, 1024, 576, "T128x64_RING4", variant=1), _g(5, 5504, 384, 576, "T128x128", variant=1), _g(5, 2048, 1024, 576, "T128x128", variant=5),
    # the persistent kernel: t256 = 127 | 128; knob 3: 255 | 256 (128 is not enough); epilogues 2 and 4 never
    _g(0, 32512, 256, 64, "T64x64"), _g(0, 32768, 256, 64, "PP"), _g(0, 65280, 256, 64, "T128x128", variant=3), _g(0, 65536, 256, 64, "PP", variant=3),
    _g(0, 32768, 256, 64, "T128x128", variant=3), _g(2, 32768, 256, 64, "T64x64"), _g(4, 32768, 256, 64, "T64x64"),
    # ... and its stride conditions: ldo0 always, ldo1 under epilogue 1 only, ldaux under epilogue 3 only (8003 x 1008: t256 = 128, t64 = 2016)
    _g(0, 8003, 1008, 64, "T64x64", ldo0=1012), _g(0, 8003, 1008, 64, "PP", ldo0=1016), _g(5, 8003, 1008, 64, "T64x64", ldo0=1012),
    _g(1, 8003, 1008, 64, "T64x64", ldo1=1012), _g(1, 8003, 1008, 64, "PP", ldo1=1016),
    _g(3, 8003, 1008, 64, "T64x64", ldaux=1012), _g(3, 8003, 1008, 64, "PP", ldaux=1016),
    _g(0, 8003, 1008, 64, "PP", ldo1=1012, ldaux=1012), _g(3, 8003, 1008, 64, "PP", ldo1=1012),
    # split K (804 x 784: t64 = 169): K = 1472 | 1536; no scratch, another epilogue, a split operand, a knob other than 0 | 12: never;
    # knob 12 takes the 64-deep slices (1280 / 169 = 7 -> 4) where knob 0 takes three 128-deep ones (512 / 169 = 3)
    _g(0, 804, 784, 1472, "T64x64", variant=S16), _g(0, 804, 784, 1536, "SPLITK_K128", 3, variant=S16),
    _g(5, 804, 784, 3072, "SPLITK_K128", 3, variant=S16), _g(5, 804, 784, 1728, "SPLITK_K64", 3, variant=S16),
    _g(5, 804, 784, 3072, "T64x64_K128"), _g(2, 804, 784, 3072, "T64x64_K128", variant=S16), _g(5, 804, 784, 3072, "T64x64", variant=S16, lo_mode=1),
    _g(5, 804, 784, 3072, "SPLITK_K64", 4, variant=S16 | 12), _g(5, 804, 784, 3072, "T64x64", variant=S16 | 9),
    # ... slice counts around t64 * slices = 512: t64 = 128 -> 4 deep slices, 130 -> 3, 171 (= 9 x 19) -> 2 deep ones are too few: 4 of the 64-deep form
    _g(0, 512, 1024, 3072, "SPLITK_K128", 4, variant=S16), _g(0, 640, 832, 3072, "SPLITK_K128", 3, variant=S16),
    _g(0, 576, 1216, 3072, "SPLITK_K64", 4, variant=S16),
    # ... 2 t64 against 5 ncu.  At 256 units the 4 Mi-element scratch of mudpt_gemm refuses two slices of 640 tiles before the tile bound does
    # (t64 = 640 | 656: unsplit either way), so the bound itself is bracketed at 64 units: t64 = 160 | 161 (= 23 x 7)
    _g(0, 2560, 1024, 3072, "T64x64", variant=S16), _g(0, 2497, 976, 3072, "T64x64", variant=S16), _g(0, 2624, 1024, 3072, "T64x64", variant=S16),
    _g(0, 640, 1024, 3072, "SPLITK_K64", 2, variant=S16, ncu=64), _g(0, 1472, 448, 3072, "T64x64", variant=S16, ncu=64),
    # ... the shapes of test_gemm_split_k
    _g(5, 804, 768, 3072, "SPLITK_K128", 3, variant=S16), _g(5, 804, 768, 2304, "SPLITK_K128", 3, variant=S16),
    _g(5, 450, 512, 2048, "SPLITK_K128", 4, variant=S16), _g(5, 201, 768, 3072, "SPLITK_K128", 4, variant=S16),
    _g(5, 1000, 768, 1536, "SPLITK_K64", 3, variant=S16),
    # the knobs: 1 | 2 | 4 a simple tile instead of the persistent kernel (16141 x 1040: t256 = 320, M N above the large-problem size)
    _g(5, 16141, 1040, 192, "PP"), _g(5, 16141, 1040, 192, "T256x256", variant=1), _g(5, 16141, 1040, 192, "T128x256", variant=2),
    _g(5, 16141, 1040, 192, "T256x128", variant=4), _g(2, 16141, 1040, 192, "T256x256"), _g(4, 16170, 1040, 192, "T256x256"),
    # 5 | 6: 128 x 128 | the ring whatever the grid; 9 | 10: 64 x 64 (10: 128-deep where K allows); 12: the default without 128-deep tiles
    _g(5, 259, 144, 192, "T128x128", variant=5), _g(5, 259, 80, 192, "T128x64_RING4", variant=6), _g(5, 259, 80, 192, "T64x64"),
    _g(5, 131, 80, 192, "T64x64", variant=9), _g(5, 131, 80, 128, "T64x64", variant=9), _g(5, 131, 80, 128, "T64x64_K128", variant=10),
    _g(5, 131, 80, 192, "T64x64", variant=10), _g(5, 131, 80, 128, "T64x64", variant=12), _g(5, 131, 80, 128, "T64x64_K128"),
    # ... on a grid past small_tiles (4100 x 1296 x 3072: t64 = 1365, t128 = 363)
    _g(5, 4100, 1296, 3072, "T128x128"), _g(5, 4100, 1296, 3072, "T128x64_RING4", variant=6), _g(5, 4100, 1296, 3072, "T64x64", variant=9),
    _g(5, 4100, 1296, 3072, "T64x64", variant=10), _g(5, 4100, 1296, 3072, "T128x128", variant=12),
    # ... and at the persistent kernel's sizes: 5 | 6 | 12 leave it in place, 9 | 10 fall to the large simple tile
    _g(5, 33000, 768, 768, "PP", variant=5), _g(5, 33000, 768, 768, "PP", variant=6), _g(5, 33000, 768, 768, "PP", variant=12),
    _g(5, 33000, 768, 768, "T256x256", variant=9), _g(5, 33000, 768, 768, "T256x256", variant=10),
]
# arguments launch_gemm refuses: K % 64, N % 16, ldo0 < N, ldo0 % 4, ldo1 / ldaux where the epilogue reads them, epilogue, lo_mode, e4m3 pass at K % 128
GEMM_FORM_REFUSED = [_g(0, 64, 64, 96, None), _g(0, 64, 72, 64, None), _g(0, 64, 64, 64, None, ldo0=48), _g(0, 64, 64, 64, None, ldo0=66),
                     _g(1, 64, 64, 64, None, ldo1=48), _g(1, 64, 64, 64, None, ldo1=66), _g(2, 64, 64, 64, None, ldaux=48), _g(3, 64, 64, 64, None, ldaux=66),
                     _g(6, 64, 64, 64, None), _g(-1, 64, 64, 64, None), _g(0, 64, 64, 64, None, lo_mode=3), _g(0, 64, 64, 192, None, lo_mode=2),
                     _g(0, 0, 64, 64, None), _g(0, 64, 64, 64, None, ncu=0)]


def test_gemm_form_table(lib):
    """Which GEMM kernel a launch runs is host arithmetic (gemm_form, exported as mudpt_gemm_form): every form computes the same numbers bit for
    bit, so only this table notices a wrong edit to the dispatch before the benchmark does.  Every threshold is bracketed on both sides."""
    header = open(capi.HEADER_PATH).read()
    for code, name in enumerate(capi.GEMM_FORMS):
        assert f"#define MUDPT_GEMM_{name} {code} " in header, name
    for args, (want, slices) in GEMM_FORM_TABLE:
        got = lib.mudpt_gemm_form(*args)
        assert got == (capi.GEMM_FORMS.index(want) | slices << 8), (args, want, slices, (capi.GEMM_FORMS[got & 0xff], got >> 8) if got >= 0 else got)
    assert {want for _, (want, _) in GEMM_FORM_TABLE} == set(capi.GEMM_FORMS)
    # epilogue 0 does not read ldo1 / ldaux: strides that epilogues 1 / 3 refuse are accepted
    assert lib.mudpt_gemm_form(0, 64, 64, 64, 64, 0, 0, 0, 0, 256) == (capi.GEMM_FORMS.index("T64x64") | 1 << 8)
    for args, _ in GEMM_FORM_REFUSED:
        assert lib.mudpt_gemm_form(*args) == -1, args
    # a split operand never takes the 128-deep small tile or a split-K form: over the M, N, K of the table, with scratch, under the knobs that lead there
    never = {capi.GEMM_FORMS.index(f) for f in ("T64x64_K128", "SPLITK_K128", "SPLITK_K64")}
    shapes = sorted({args[1:4] for args, _ in GEMM_FORM_TABLE})
    plain = set()
    for M, N, K in shapes:
        for knob in (0, 10, 12):
            for epi in (0, 5):
                plain.add(lib.mudpt_gemm_form(epi, M, N, K, N, N, N, 0, S16 | knob, 256) & 0xff)
                for lo_mode in (1, 2):
                    if lo_mode == 2 and K % 128:
                        continue
                    got = lib.mudpt_gemm_form(epi, M, N, K, N, N, N, lo_mode, S16 | knob, 256)
                    assert got >= 0 and got & 0xff not in never and got >> 8 == 1, (epi, M, N, K, lo_mode, knob, got)
    assert never <= plain  # the sweep does reach all three without a split operand


def test_gemm_gpu_cases_reach_every_form(lib):
    """The cases tests/test_gemm_forms_gpu.py runs reach, at 256 compute units, all ten forms with the form each names, every grid regime of
    launch_pp and every tile-order regime of gemm_pp_kernel's tile_mn (a Python mirror of their formulas: GN lives in device code); and the
    mirrored tile order visits every tile of every persistent case exactly once."""
    from tests import helpers as H
    reached = set()
    for c in H.GEMM_FORM_CASES + H.GEMM_REFUSAL_CASES:
        for epi in c.epis:
            got = lib.mudpt_gemm_form(*H.gemm_form_args(c, epi, 256))
            assert got == (capi.GEMM_FORMS.index(c.form) | c.slices << 8), (c.name, epi, got)
            reached.add(got & 0xff)
    assert reached == set(range(len(capi.GEMM_FORMS))), sorted(capi.GEMM_FORMS[i] for i in set(range(10)) - reached)
    assert {c.name for c in H.GEMM_FORM_CASES} >= set(H.GEMM_GELU_CASES)
    assert {c.form for c in H.GEMM_FORM_CASES if c.name in H.GEMM_GELU_CASES} == set(capi.GEMM_FORMS) - {"SPLITK_K128", "SPLITK_K64"}
    pp = [c for c in H.GEMM_FORM_CASES if c.form == "PP"]
    for c in pp:
        assert (H.pp_grid_regime(c.M, c.N, 256), H.pp_order_regime(c.N)) == (c.grid, c.order), c.name
        ntm, ntn = -(-c.M // 256), -(-c.N // 256)
        assert sorted(H.pp_tile_mn(t, ntm, ntn) for t in range(ntm * ntn)) == [(m, n) for m in range(ntm) for n in range(ntn)], c.name
    assert {c.grid for c in pp} == {"all_split", "one_per_workgroup", "half_tile_tail", "whole_tile_tail"}
    assert {c.order for c in pp} == {"one_group", "full_groups", "leftover_group"}
    # K = 64 (one K-step per tile: the prefetch crosses a tile boundary every step) and 128 run on the persistent kernel too
    assert {64, 128} <= {c.K for c in pp}


def test_gemm_split_gpu_cases_reach_every_form(lib):
    """The split-operand cases tests/test_gemm_split_forms_gpu.py runs reach, at 256 compute units, exactly the seven forms a split operand can
    take, each case with the form it names, under both forms of the low half; the persistent cases reach every grid regime of launch_pp and
    every tile-order regime under each lo_mode, and the K-step counts per tile the second pass brings: lo_mode 1 doubles the count (always
    even; the first pass ends on either LDS stage), lo_mode 2 gives K / 64 + K / 128, odd and even."""
    from tests import helpers as H
    form = lambda c, epi: lib.mudpt_gemm_form(*H.gemm_form_args(c, epi, 256))  # noqa: E731
    reached = {1: set(), 2: set()}
    for c in H.GEMM_SPLIT_CASES + H.GEMM_SPLIT_PATCH_CASES:
        assert c.lo_mode in (1, 2) and (c.lo_mode == 1 or c.K % 128 == 0), c.name
        for epi in c.epis:
            got = form(c, epi)
            assert got == (capi.GEMM_FORMS.index(c.form) | 1 << 8), (c.name, epi, got)
            if c in H.GEMM_SPLIT_CASES:
                reached[c.lo_mode].add(c.form)
    assert reached[1] == reached[2] == set(H.GEMM_SPLIT_FORMS) == set(capi.GEMM_FORMS) - {"T64x64_K128", "SPLITK_K128", "SPLITK_K64"}
    names = {c.name for c in H.GEMM_SPLIT_CASES}
    assert len(names) == len(H.GEMM_SPLIT_CASES) and set(H.GEMM_SPLIT_SCALE_CASES) <= names
    assert {c.form == "PP" for c in H.GEMM_SPLIT_CASES if c.name in H.GEMM_SPLIT_SCALE_CASES} == {True, False}
    # the ring's K-tiles of both passes: below, at and above its prologue depth of 3
    ring = {lo: sorted(H.pp_ksteps(c) for c in H.GEMM_SPLIT_CASES if c.form == "T128x64_RING4" and c.lo_mode == lo) for lo in (1, 2)}
    assert ring == {1: [2, 4, 6, 8], 2: [3, 6, 9]}
    for lo in (1, 2):
        pp = [c for c in H.GEMM_SPLIT_CASES if c.form == "PP" and c.lo_mode == lo]
        for c in pp:
            assert (H.pp_grid_regime(c.M, c.N, 256), H.pp_order_regime(c.N)) == (c.grid, c.order), c.name
        assert {c.grid for c in pp} == {"all_split", "one_per_workgroup", "half_tile_tail", "whole_tile_tail"}
        assert {c.order for c in pp} == {"one_group", "full_groups", "leftover_group"}
        steps = {H.pp_ksteps(c) for c in pp}
        if lo == 1:
            assert steps == {2, 4, 6} and {c.K // 64 % 2 for c in pp} == {0, 1}
        else:
            assert steps == {3, 6, 15} and {n % 2 for n in steps} == {0, 1}
        # every regime sees both parities where the form has both
        for grid in ("all_split", "one_per_workgroup", "half_tile_tail", "whole_tile_tail"):
            assert {H.pp_ksteps(c) % 2 for c in pp if c.grid == grid} == ({0} if lo == 1 else {0, 1}), (lo, grid)
    # the QuickGELU cases: one per form, each form under every input form it runs with (epilogue 1 reads ldo1)
    assert [c.form for c in H.GEMM_SPLIT_GELU_CASES] == ["T64x64", "T128x64_RING4", "T128x128", "T256x256", "T128x256", "T256x128", "PP"]
    for c in H.GEMM_SPLIT_GELU_CASES:
        for lo in ((0, 1, 2) if c.name in H.GEMM_SPLIT_GELU_ALL_PAIRS else (1, 2)):
            k = H.gemm_split_gelu_case(c, lo)
            for windowed in (True, False):
                got = lib.mudpt_gemm_form(*H.gemm_form_args(k, 1, 256, windowed))
                assert got == (capi.GEMM_FORMS.index(c.form) | 1 << 8), (c.name, lo, windowed, got)
    # the patch cases: both tiles under both forms, whole images
    assert {(c.form, c.lo_mode) for c in H.GEMM_SPLIT_PATCH_CASES} == {(f, lo) for f in ("T256x256", "T64x64") for lo in (1, 2)}
    assert all(c.M % c.patch[0] == 0 for c in H.GEMM_SPLIT_PATCH_CASES)
