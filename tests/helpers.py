"""Shared test helpers: rebuild a golden case (weights from the seeded recipe) for the oracle."""
import ast
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch

from oracle import mudpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class FixtureCase:
    """One tests/golden/<name>.npz fixture of any variant, with everything the file holds as a recipe rebuilt: the frozen weights and the
    images from their seeds (the images held to the stored checksum), the tokenized class prompts with their EOT rows and token embeddings,
    labels, the reference's logits and loss, and the sampled block inputs ``taps`` = {"<vis|txt>.<i>": ([seq, rows, d], rows)}.  A variant's
    loader subclasses it and adds its own fields; ``keys`` (its trainables in order) lets :meth:`load_grads` read the gradients."""

    def __init__(self, name: str):
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        self.name, self.z = name, z
        self.cfg = O.Config(**ast.literal_eval(str(z["config"])))
        self.seeds = tuple(int(v) for v in z["seeds"])  # (frozen weights, trainables, images); the zero-shot fixtures have no trainables
        self.frozen = O.make_frozen_state(self.cfg, self.seeds[0])
        if "logit_scale" in z.files:  # the *_s100 fixtures: exp(logit_scale) = 100, what pretrained CLIP checkpoints hold (clip/model.py:919)
            self.frozen["logit_scale"] = torch.tensor(float(z["logit_scale"]))
        if "classnames" in z.files:
            self.classnames = [str(v) for v in z["classnames"]]
        if "tokenized_prompts" in z.files:
            self.tokens = torch.from_numpy(z["tokenized_prompts"]).long()
            self.eot = self.tokens.argmax(dim=-1)  # trainers/mudpt.py:154
            self.class_embedding = self.frozen["token_embedding.weight"][self.tokens]
        if "ctx_token_ids" in z.files:
            self.ctx_token_ids = [int(v) for v in z["ctx_token_ids"]]
        self.labels = torch.from_numpy(z["labels"])
        g = torch.Generator().manual_seed(self.seeds[-1])
        self.images = torch.randn(len(self.labels), 3, self.cfg.image_size, self.cfg.image_size, generator=g)
        if "images_checksum" in z.files:  # the seeded images are the ones the fixture was generated from
            img = self.images.double()
            np.testing.assert_allclose([img.sum().item(), img.abs().sum().item()], z["images_checksum"], rtol=1e-12)
        self.logits = torch.from_numpy(z["logits"])
        if "loss" in z.files:
            self.loss = float(z["loss"])
        self.taps = {k[4:]: (torch.from_numpy(z[k]), [int(r) for r in z[k + ".rows"]]) for k in z.files if k.startswith("tap.") and k + ".rows" in z.files}

    def load_grads(self):
        """grads: the full gradients; grad_samples: (rows, values [16, cols], rms of the whole tensor) of the ones stored as sampled rows."""
        z = self.z
        self.grads = {k: torch.from_numpy(z["grad." + k]) for k in self.keys if "grad." + k in z.files}
        self.grad_samples = {k: ([int(r) for r in z["grad_rows." + k + ".idx"]], torch.from_numpy(z["grad_rows." + k]), float(z["grad_rms." + k]))
                             for k in self.keys if "grad_rows." + k in z.files}


class GoldenCase(FixtureCase):
    """name "mudpt_*": trainers/mudpt.py fixtures; "cocoop_*": trainers/cocoop.py fixtures (5 trainables, cocoop_oracle)."""

    def __init__(self, name: str):
        super().__init__(name)
        self.cocoop = name.startswith("cocoop")
        if self.cocoop:
            from oracle import cocoop_oracle as variant
        else:
            variant = O
        self.params = variant.make_trainable_state(self.cfg, self.seeds[1], self.frozen, self.ctx_token_ids)

    def check_recipe(self):
        """The seeded recipe reproduced the tensors the fixture was generated from (the images: FixtureCase)."""
        assert "images_checksum" in self.z.files
        f = self.frozen
        if "frozen_checksum" not in self.z.files:
            return
        np.testing.assert_allclose(
            [f["visual.transformer.resblocks.0.attn.in_proj_weight"].double().sum().item(),
             f["token_embedding.weight"].double().abs().sum().item()], self.z["frozen_checksum"], rtol=1e-12)

    def grad(self, key):
        k = "grad." + key
        return torch.from_numpy(self.z[k]) if k in self.z.files else None

    def grad_sample(self, key):
        k = "grad_sample." + key
        return torch.from_numpy(self.z[k]) if k in self.z.files else None


# A TRAINING forward of a tiny batch (<= 8 ViT-B images: <= 320 tiles of 64 x 64) splits the contraction of the vision tower's out_proj /
# c_proj over K slices (a differently associated fp32 sum flips the T rounding of ~1 % of their outputs); an INFERENCE forward never does, so
# that the logits of an image do not depend on the size of the test batch it arrives in.  At such batches the two forwards
# agree to that rounding only (measured 2.8e-4 fp16 / 5e-3 bf16 at logit scale 14.29); above them, and in the parity mode, bit for bit.
FWD_SPLIT_TOL = {"fp16": 6e-4, "bf16": 1.2e-2, "fp32": 0.0}  # (CoCoOp, where the image features enter twice: 9.3e-3 bf16)


def assert_training_forward_is_the_inference_forward(train_logits, eval_logits, dtype):
    a, b = train_logits.detach().float().cpu(), eval_logits.detach().float().cpu()
    if torch.equal(a, b):
        return
    d = (a - b).abs().max().item()
    assert d <= FWD_SPLIT_TOL[dtype], f"training vs inference logits differ by {d:.3e} ({dtype})"


# ---- bounds of the whole-model parity tests (test_model_gpu.py, test_knobs_gpu.py and the variants' suites) ---------------------------
# Logit tolerance.  north_star: "logits matching the reference PyTorch CPU path within 1e-3 fp16".
# Measured on MI355X (tools/error_growth.py, ViT-B/16 B=4 golden case, 44 logits, logit scale 14.29):
#   fp16 operands: max 6.1e-4, rms 2.7e-4 (text features 3.1e-4 relative, image features 1.7e-4);  bf16: max 1.4e-2, rms 1.0e-2.
# fp16 mode runs the text tower with split [hi | lo] GEMM operands (Tower::split): with plain 11-bit operands the
# text features carried 6.5e-4 of relative error and single logits reached 1.5e-3.  The ViT-B/16 case is held to the north_star
# bound on the MAXIMUM over the logits; the 3-layer tiny shape (wider relative spread, 33 logits) gets 1.5x that.
# bf16 (8-bit significand) is 16x coarser and only sanity-bounded.
LOGIT_RMS = {"fp16": 5e-4, "bf16": 1.6e-2}
LOGIT_ATOL = {"fp16": 1e-3, "bf16": 3.2e-2}
TINY_SLACK = 1.5
GRAD_RTOL = {"fp16": 2e-2, "bf16": 1.5e-1}  # relative to each gradient tensor's RMS: single elements may be off by 4x this
# RMS of the error over a whole gradient tensor, relative to the tensor's RMS (the error model of tests/test_cocoop_gpu.py without the
# cancellation factor: MuDPT's gradients are sums of same-signed-on-average terms).  Measured on MI355X (round 3): fp16 <= 2.6e-3,
# bf16 <= 3.8e-2 over the four fixtures; the bounds leave a factor 2.3 / 1.6.
GRAD_RMS = {"fp16": 6e-3, "bf16": 6e-2}
GRAD_COS = {"fp16": 0.9995, "bf16": 0.99}  # direction: cosine similarity of a whole gradient tensor with the oracle's


# ---- the steps the variants' parity suites share ---------------------------------------------------------------------------------------------
def check_logits(logits, case, dtype, tag, slack=None, rms_bound=LOGIT_RMS, atol=LOGIT_ATOL):
    """A handle's logits against the fixture's: rms and maximum within slack x the mode's bounds; slack defaults to TINY_SLACK on the 3-layer
    shape.  Returns the slack (the suites hold the loss to slack * LOGIT_ATOL)."""
    d = logits.detach().cpu() - case.logits
    err, rms = d.abs().max().item(), d.pow(2).mean().sqrt().item()
    slack = (TINY_SLACK if case.cfg.v_layers < 12 else 1.0) if slack is None else slack
    print(f"{tag}: |logit - reference| max {err:.3e} rms {rms:.3e}")
    assert rms <= slack * rms_bound[dtype] and err <= slack * atol[dtype], (tag, err, rms)
    return slack


def check_sampled_taps(m, case, dtype):
    """The fixture's sampled block inputs (FixtureCase.taps: the rows a block splices, after its splice) against the handle's x_in buffers."""
    B = len(case.labels)
    for key, (ref, rows) in case.taps.items():
        tower, i = key.split(".")
        x = m.debug_read(f"{tower}.x_in.{i}", B)
        d = case.cfg.v_width if tower == "vis" else case.cfg.t_width
        x = x.view(-1, x.numel() // (d * (B if tower == "vis" else len(case.classnames))), d)[:, rows]
        tol = (2e-3 if dtype == "fp16" else 3e-2) * (1 + ref.abs().max().item())
        assert (x - ref).abs().max().item() <= tol, (key, (x - ref).abs().max().item())


def check_parity_mode_at_scale_100(m, case):
    """The body of the suites' test_parity_mode_at_logit_scale_100: a dtype "fp32" handle's eval logits within 1e-3 of the fixture's; closes m."""
    m.eval()
    logits = m(case.images).cpu()
    err, rms = (logits - case.logits).abs().max().item(), (logits - case.logits).pow(2).mean().sqrt().item()
    print(f"{case.name} parity mode: |logit - reference| max {err:.3e} rms {rms:.3e}")
    assert err <= 1e-3
    m.close()


def check_grad(g, r, dtype, tag, rms=None, rms_err=True, cos=False):
    """One gradient tensor against its reference: the largest error within 4 GRAD_RTOL x the reference's rms and (rms_err) the rms of the
    error within GRAD_RMS x it; cos: the cosine above GRAD_COS as well.  rms: of the whole tensor, where g and r are sampled rows of it."""
    g, r = g.detach().float().cpu(), r.float()
    rms = r.pow(2).mean().sqrt().item() if rms is None else rms
    err, rel_rms = (g - r).abs().max().item(), (g - r).pow(2).mean().sqrt().item() / max(rms, 1e-30)
    c = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item() if cos else None
    print(f"{tag}: rms {rms:.3e} max err / rms {err / max(rms, 1e-30):.3e} rms err {rel_rms:.3e}" + (f" cos {c:.6f}" if cos else ""))
    assert err <= GRAD_RTOL[dtype] * rms * 4 + 1e-9, (tag, err, rms)
    assert not rms_err or rel_rms <= GRAD_RMS[dtype], (tag, rel_rms)
    assert not cos or c > GRAD_COS[dtype], (tag, c)


def check_grads(got, ref, dtype, tag, **kw):
    """check_grad of every tensor of ref."""
    for k, r in ref.items():
        check_grad(got[k], r, dtype, f"{tag} {k}", **kw)


def check_fixture_grads(got, case, dtype, tag, factor=1.0):
    """Every trainable against factor x the fixture's stored gradient (the reference's own autograd): the full tensor, or its sampled rows
    with the stored rms of the whole; exactly zero where the reference's is."""
    for k in case.keys:
        if got[k].numel() == 0:
            continue
        if k in case.grads:
            if case.grads[k].abs().max().item() == 0:
                assert torch.count_nonzero(got[k]) == 0, k
            else:
                check_grad(got[k], case.grads[k] * factor, dtype, f"{tag} {k}")
        else:
            rows, vals, rms = case.grad_samples[k]
            if rms == 0:
                assert torch.count_nonzero(got[k]) == 0, k
            else:
                check_grad(got[k][rows], vals * factor, dtype, f"{tag} {k} [16 rows]", rms=rms * factor)


# ---- the parity mode's training step (dtype "fp32": an fp16-typed backward with lp_grad = 1) in the variants' suites ---------------------------
def grad_triple(g, r, rms=None):
    """(max error / rms, rms error / rms, cosine) of a gradient tensor against its reference; rms: of the whole tensor where r is a sample."""
    g, r = g.detach().double().cpu(), r.double()
    rms = max(r.pow(2).mean().sqrt().item() if rms is None else rms, 1e-30)
    cos = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
    return (g - r).abs().max().item() / rms, (g - r).pow(2).mean().sqrt().item() / rms, cos


def check_parity_step_grads(name, pairs, measured):
    """pairs: (key, the library's gradient, the restatement's) of every trainable of one parity-mode step.  The hard bound is the bf16 row
    (the mode runs lp_grad = 1, which test_knobs_gpu.py grades that way); inside it the worst tensor is held to TWICE what the variant
    measured on an MI355X: `measured` = (max error / rms, rms error / rms, cosine); for the cosine, twice its distance from 1.  Returns the
    worst triple."""
    worst = [0.0, 0.0, 1.0]
    for k, g, r in pairs:
        if g.numel() == 0 or r.abs().max().item() == 0:
            assert torch.count_nonzero(g) == 0, k
            continue
        t = grad_triple(g, r)
        print(f"{name} parity mode {k}: max err {t[0]:.3e} x rms, rms err {t[1]:.3e} x rms, cos {t[2]:.6f}")
        worst = [max(worst[0], t[0]), max(worst[1], t[1]), min(worst[2], t[2])]
    bmax, brms, bcos = 4 * GRAD_RTOL["bf16"], GRAD_RMS["bf16"], GRAD_COS["bf16"]
    bmax, brms, bcos = min(bmax, 2 * measured[0]), min(brms, 2 * measured[1]), max(bcos, 1 - 2 * (1 - measured[2]))
    print(f"{name} parity mode, worst tensor: max {worst[0]:.2e} (bound {bmax:.2e}) rms {worst[1]:.2e} (bound {brms:.2e}) cos {worst[2]:.6f} (floor {bcos:.6f})")
    assert worst[0] <= bmax and worst[1] <= brms and worst[2] > bcos, (name, worst)
    return tuple(worst)


# ---- the per-handle knobs of mudpt_model_set (include/mudpt.h): one row per name; test_capi_cpu.py holds the table to the names the library
# compares against and to the header's table, test_knobs_gpu.py runs the settings ----
class KnobSetting(namedtuple("KnobSetting", "dtype sets lowers construct", defaults=(False, False))):
    """One non-default setting of a knob on a handle of `dtype`: the (name, value) calls that apply it, in order; lowers = it lowers an fp16
    handle's arithmetic grade towards bf16's (test_knobs_gpu.py then bounds it by the bf16 constants); construct = it goes through ``knobs=``
    at construction, ahead of the weights."""
    __slots__ = ()

    @property
    def id(self):
        return "-".join(f"{k}{v}" for k, v in self.sets) + "-" + self.dtype


def _both(name, *values):
    return tuple(KnobSetting(dt, ((name, v),)) for v in values for dt in ("fp16", "bf16"))


def _parity(*sets):
    """A setting of the parity mode's own knobs on a dtype "fp32" handle."""
    return KnobSetting("fp32", tuple(sets))


# what test_knobs_gpu.py sets a handle back to after a case, in this order (lp_grad ahead of lp_upd, which it moves in bf16); the values are
# the header's table, the text tower's split operands exist in fp16 mode only.  "fp32" (the parity mode) is what mudpt_create starts such a
# handle with: an fp16-typed backward with the gradient stream in T (lp_grad 1), fp32 update stream, u in T; fp16 pairs and the fp32 attention
# forward in the text tower, e4m3 remainders at every site and fp16 attention in the vision tower
_COMMON = {"gemm_variant": 0, "split_k": 1, "attn_window": 1, "attn_two_kernels": 0, "attn_fused_w1": 0}
KNOB_DEFAULTS = {"fp16": dict(_COMMON, lp_grad=0, lp_upd=0, gelu_q8=0, txt_lo=1, txt_sites=31), "bf16": dict(_COMMON, lp_grad=1, lp_upd=1, gelu_q8=1),
                 "fp32": dict(_COMMON, lp_grad=1, lp_upd=0, gelu_q8=0, txt_lo=1, txt_sites=31, vis_lo=2, vis_sites=31, vis_exact_attn=0, txt_exact_attn=1)}
_ORACLE = "tests/test_knobs_gpu.py::test_setting_matches_the_oracle"
_ABLATION = "tests/test_exact_gpu.py::test_precision_ablation_on_the_gpu"
_BOTH_TESTS = _ORACLE + ", " + _ABLATION  # the ablation holds the logits of a handle built with the knob, the oracle test a whole step after a flip
# name -> (settings worth testing, the tests that hold the knob (", " between two), "" = none: say why in the third field)
MODEL_KNOBS = {
    "gemm_variant": (_both("gemm_variant", 12, 1, 10), _ORACLE, ""),
    "attn_window": (_both("attn_window", 0), _ORACLE, ""),
    "attn_two_kernels": (_both("attn_two_kernels", 1), _ORACLE, ""),
    "attn_fused_w1": (_both("attn_fused_w1", 1), _ORACLE, ""),
    # bf16: lp_grad moves lp_upd with it (mudpt_model_set), so lp_upd is set back behind it
    "lp_grad": ((KnobSetting("fp16", (("lp_grad", 1),), lowers=True), KnobSetting("bf16", (("lp_grad", 0), ("lp_upd", 1)))), _ORACLE, ""),
    "lp_upd": ((KnobSetting("fp16", (("lp_upd", 1),), lowers=True), KnobSetting("bf16", (("lp_upd", 0),))), _ORACLE, ""),
    "gelu_q8": ((KnobSetting("fp16", (("gelu_q8", 1),), lowers=True), KnobSetting("bf16", (("gelu_q8", 0),))), _ORACLE, ""),
    "txt_split": ((KnobSetting("fp16", (("txt_split", 0),), lowers=True, construct=True),), _ORACLE, ""),
    "txt_trim": ((), "tests/test_model_gpu.py::test_text_tower_trim_changes_nothing", ""),
    "txt_buckets": ((), "tests/test_manyclass_gpu.py::test_c208_length_buckets_change_nothing", ""),
    "txt_bucket_cost": ((), "tests/test_manyclass_gpu.py::test_c208_length_buckets_change_nothing", ""),
    "last_single": ((), "tests/test_model_gpu.py::test_last_block_single_query_path_equals_the_general_kernels", ""),
    "split_k": ((), "tests/test_model_gpu.py::test_split_k_agrees_with_the_sequential_contraction", ""),
    "fwd_split_k": ((), "tests/test_model_gpu.py::test_split_k_agrees_with_the_sequential_contraction", ""),
    "cocoop_chunk": ((), "tests/test_cocoop_gpu.py::test_larger_batch_against_oracle_and_sgd", ""),
    # the split-operand knobs: the parity mode's ablation holds the vision tower's and the text tower's attention; the fp16 mode's text-tower
    # ones run here between two steps (txt_lo 0 is txt_split 0 without a new handle; txt_sites 5: in_proj and c_fc only)
    # (the parity mode's own, on a dtype "fp32" handle at logit scale 100: logits, loss and gradients of the step under each)
    "vis_lo": ((_parity(("vis_lo", 1)),), _BOTH_TESTS, ""),
    "vis_sites": ((_parity(("vis_sites", 12)),), _BOTH_TESTS, ""),
    "vis_exact_attn": ((_parity(("vis_exact_attn", 1)), _parity(("vis_exact_attn", 1), ("vis_lo", 1))), _BOTH_TESTS, ""),
    "txt_exact_attn": ((_parity(("txt_exact_attn", 0)),), _BOTH_TESTS, ""),
    "txt_lo": ((KnobSetting("fp16", (("txt_lo", 0),), lowers=True),), _ORACLE, ""),
    "txt_sites": ((KnobSetting("fp16", (("txt_sites", 5),), lowers=True),), _ORACLE, ""),
    "prof_stride": ((), "", "measurement only: which persistent-GEMM launches the profiling mode brackets; no result depends on it"),
}
ATTN_FORM_KNOBS = ("attn_two_kernels", "attn_fused_w1")  # the ones that also run at L > 224 (staged / resident forms)


def knob_settings(names=None, dtype=None):
    """The settings of MODEL_KNOBS, of the knobs `names` (default: all) on handles of `dtype` (default: both)."""
    return [s for k, (settings, _, _) in MODEL_KNOBS.items() if names is None or k in names for s in settings if dtype is None or s.dtype == dtype]


# ---- single-kernel tests through the C ABI (test_kernels_gpu.py, test_movers_gpu.py) ------------------------------------------------
SENT = -1234.5  # destinations are pre-filled with it: exactly representable in fp32, bf16 and fp16


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ok(lib, rc):
    assert rc == 0, lib.mudpt_last_error().decode()
    torch.cuda.synchronize()


def refused(lib, rc, word):
    """MUDPT_ERR_ARG with a message that holds `word`; the caller then asserts that its sentinel-filled destinations are untouched."""
    torch.cuda.synchronize()
    msg = lib.mudpt_last_error().decode()
    assert rc == 1 and word in msg, (rc, msg)


def e4m3_spacing(s):
    """Distance between neighbouring OCP e4m3 values at magnitude |s|: 3 mantissa bits, minimum normal 2^-6, below it steps of 2^-9."""
    a = s.abs().double().clamp_min(2.0 ** -6)
    return torch.ldexp(torch.ones_like(a), torch.frexp(a).exponent - 1 - 3)


EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # half ulp relative


def check_split_pair(dtype, hi, lo16, lo8, ref):
    """hi [rows, Hd] in T, lo16 the remainder in T, lo8 its e4m3 codes (uint8), ref float64.  hi + lo against the definition; |lo| <= half an
    ulp of hi (hi is the T rounding of the kernel's fp32 value, as test_exact_attention_forward asserts); the e4m3 form decodes to the same
    remainder: e4m3(r 2^12) is within half an e4m3 step of r 2^12 and T(r) within EPS |r| of r, so the two forms differ by at most that sum.
    The bounds above hold for `hi` alone, so two more pin lo itself (both follow from lo = v - T(v) for the kernel's fp32 value v = ref + err,
    over N >= 768 elements of continuous data):
      * lo / ulp is uniform on [-1/2, 1/2]: its mean square is 1/12 (sampling noise ~1 / sqrt(N) of that); a lo that is zero, halved, doubled
        or saturated misses [1/16, 1/9];
      * ref - hi = lo + (ref - v), and the kernel's error ref - v does not depend on the rounding remainder, so <lo, ref - hi> / <lo, lo> is
        1 +- rms(err) / (rms(lo) sqrt(N)): with the error of the order of the remainder (the probabilities enter P.V rounded to T) that is a
        few per cent at the smallest N.  A sign-flipped lo gives -1, a lo unrelated to the value gives 0: [0.5, 1.5] is asserted."""
    mant, tiny = (7, 2.0 ** -126) if dtype == "bf16" else (10, 2.0 ** -14)
    torch.testing.assert_close(hi.double() + lo16.double(), ref, atol=6 * EPS[dtype], rtol=6 * EPS[dtype])
    ulp = torch.ldexp(torch.ones(()), torch.frexp(hi.float().abs().clamp_min(tiny)).exponent - 1 - mant)
    assert (lo16.float().abs() <= 0.5 * ulp * (1 + 1e-3)).all()
    msq = (lo16.double() / ulp.double()).pow(2).mean().item()
    proj = ((lo16.double() * (ref - hi.double())).sum() / lo16.double().pow(2).sum()).item()
    print(f"split pair {dtype}: N {hi.numel()}, mean (lo / ulp)^2 {msq:.4f} (1/12 = 0.0833), <lo, ref - hi> / <lo, lo> {proj:.3f}")
    assert 1 / 16 <= msq <= 1 / 9 and 0.5 <= proj <= 1.5
    r = lo16.double()
    assert (r.abs() * 4096 * (1 + 2 * EPS[dtype])).max().item() < 448  # no saturation on these inputs
    dec = lo8.contiguous().view(torch.float8_e4m3fn).double() / 4096.0
    bound = 0.5 * e4m3_spacing(r * 4096 * (1 + 2 * EPS[dtype])) / 4096.0 + 2 * EPS[dtype] * r.abs() + 2.0 ** -25  # (2^-25: half a subnormal fp16 step)
    assert ((dec - r).abs() <= bound).all()


PATCH_CASES = [(64, 224, 16, 768), (8, 224, 32, 3072), (16, 336, 14, 640), (5, 32, 8, 192), (3, 28, 14, 640)]  # (B, S, p, ldk) of test_patchify_plain
PATCH_SPLIT_CASES = [(128, 224, 16, 768), (3, 336, 14, 640), (5, 32, 8, 192), (3, 28, 14, 640), (2, 224, 32, 3072)]


def patchify_threads(form, B, S, p, ldk):
    """Threads the launcher's grid-stride loop has to cover and the most its capped grid holds (elementwise.hip launch_patchify*)."""
    if form == "vector":
        return B * 3 * S * (S // 8), 4096 * 256
    if form == "any":
        return B * (S // p) ** 2 * ldk, 16384 * 256
    return B * (S // p) ** 2 * (ldk // 4), 16384 * 256


# ---- attention cases of test_kernels_gpu.py, kept here so that test_capi_cpu.py can check, without a GPU, which kernel forms they reach ----
# (B, L, H, causal) of test_attention_fwd_bwd
ATTN_CASES = [(3, 201, 12, False), (11, 77, 8, True), (2, 7, 3, False), (2, 33, 2, True), (1, 224, 1, False), (2, 64, 2, True),
              # L > 224: the tiled (online-softmax) kernels; 581 = ViT-L/14@336's 577 tokens + 4 prompt rows (BASELINE configs[4])
              # (forward: K and V of a pair resident in LDS up to L = 640, one workgroup per pair; above that the staged 16-query-block form)
              (2, 300, 2, False), (1, 581, 3, False), (2, 260, 2, True), (1, 225, 1, False), (1, 640, 2, False), (1, 641, 1, False),
              (2, 513, 2, True), (70, 300, 4, False),
              # backward: Q | dO | lse | delta of a pair resident up to L = 608; 609 .. 640: resident forward, staged backward
              (1, 608, 1, False), (1, 609, 1, True),
              # more (sequence, head) pairs than resident workgroups: the persistent loops of the forward and the fused backward walk
              # several pairs per workgroup (images of the next pair stream in while the current one is computed)
              (150, 201, 2, False), (700, 20, 8, True),
              # a causal sequence of padded length >= 128: the default causal route at 97 .. 224 (pair forward, two-kernel backward, NC = 4)
              (2, 100, 2, True)]
ATTN_LONG_FWD_CASES = [(2, 581, 3, False, 1.0), (2, 581, 3, False, 3.0), (3, 400, 2, True, 2.5), (1, 640, 1, False, 0.05)]  # (B, L, H, causal, gain)
ATTN_WINDOW_CASES = [(3, 201, 12, False, 197, 4), (2, 77, 8, True, 1, 4), (3, 150, 2, False, 14, 4), (2, 581, 4, False, 577, 4),
                     (2, 581, 2, False, 62, 5), (4, 26, 8, True, 1, 16)]  # (B, L, H, causal, row0, n)
ATTN_SEL_CASES = [(26, 8, True), (77, 8, True), (201, 12, False), (581, 3, False)]  # (L, H, causal)


def attn64(qkv, H, causal):
    """softmax(q k^T / 8 [+ causal mask]) v per head in float64; qkv [B, L, 3 H 64] packed q | k | v, heads contiguous in each third."""
    B, L, _ = qkv.shape
    q, k, v = (t.reshape(B, L, H, 64).transpose(1, 2).double() for t in qkv.split(H * 64, dim=-1))
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, H * 64)


def attn64_fwd_bwd(qkv, dout, H, causal, round_to=None):
    """(out [B, L, H 64], lse [B, H, L], dqkv [B, L, 3 H 64]) of attn64 and its gradient under dout, in float64 without autograd (so that the
    4096-row case needs no graph).  round_to = a 16-bit torch dtype T: the same sums with the values rounded to T where the kernels round them
    (test_attention_forms_gpu.py lists the points); every product and sum stays float64."""
    rnd = (lambda x: x) if round_to is None else (lambda x: x.to(round_to).double())
    B, L, _ = qkv.shape
    q, k, v = (t.reshape(B, L, H, 64).transpose(1, 2).double() for t in qkv.split(H * 64, dim=-1))
    g = dout.reshape(B, L, H, 64).transpose(1, 2).double()
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    lse = m + torch.log(l)
    o = rnd((rnd(e) @ v) / l)  # forward: exp(s - max) to T before P.V, the row sum from the unrounded values, O to T
    p = torch.exp(s - lse)     # backward: the normalised probabilities again, from lse
    delta = (g * o).sum(dim=-1, keepdim=True)
    ds = rnd(p * (g @ v.transpose(-1, -2) - delta))
    dq, dk, dv = ds @ k / 8.0, ds.transpose(-1, -2) @ q / 8.0, rnd(p).transpose(-1, -2) @ g
    flat = lambda t: t.transpose(1, 2).reshape(B, L, H * 64)  # noqa: E731
    return flat(o), lse.squeeze(-1), rnd(torch.cat([flat(dq), flat(dk), flat(dv)], dim=-1))


def attn_bwd_form_flags(L, causal):
    """The kernel-choice bits test_attention_fwd_bwd adds to the backward after the default run; bit 4 (sweep) where a sweep kernel exists."""
    return (2, 4, 8) if causal or L > 224 else (2, 4, 8, 16)


ATTN_LONG_FWD_FLAGS = (0, 2)  # test_attention_long_forward_forms: the default form and the staged one (bit 1)
ATTN_WINDOW_FULL_FLAG = 2     # test_attention_backward_window_form: its reference run, the two-kernel form on all rows
ATTN_SEL_COMPARE = ((2, True), (0, False))  # test_attention_bwd_sel_rows: (flag of the general backward it compares with, equal bit for bit?)


def attn_window_flags(row0, n):
    """The window form of mudpt_attention_bwd: n rows per sequence from row0 on."""
    return (row0 << 8) | (n << 20)


def attention_test_launches():
    """(bwd, L, flags, sel) of every mudpt_attention_fwd / _bwd / _bwd_sel call that test_attention_fwd_bwd, test_attention_long_forward_forms,
    test_attention_backward_window_form and test_attention_bwd_sel_rows make: the arguments of mudpt_attention_form."""
    calls = []
    for _, L, _, causal in ATTN_CASES:
        c = int(causal)
        calls += [(0, L, c, 0), (1, L, c, 0)] + [(1, L, c | f, 0) for f in attn_bwd_form_flags(L, causal)]
    for _, L, _, causal, _ in ATTN_LONG_FWD_CASES:
        calls += [(0, L, int(causal) | f, 0) for f in ATTN_LONG_FWD_FLAGS]
    for _, L, _, causal, row0, n in ATTN_WINDOW_CASES:
        calls += [(0, L, int(causal), 0), (1, L, int(causal) | ATTN_WINDOW_FULL_FLAG, 0), (1, L, int(causal) | attn_window_flags(row0, n), 0)]
    for L, _, causal in ATTN_SEL_CASES:
        calls += [(0, L, int(causal), 0), (1, L, int(causal), 1)] + [(1, L, int(causal) | f, 0) for f, _ in ATTN_SEL_COMPARE]
    return calls


# ---- attention cases of test_attention_forms_gpu.py: every (form, NC = padded length / 32, mask) instantiation of the whole-pair kernels, the
# persistent loops over pairs, the single-query edges and the long forms; test_capi_cpu.py holds them to mudpt_attention_form without a GPU ----
ATTN_GUARD_ROWS = 64  # rows of NaN (operands) / sentinel (outputs) before and after every tensor
ATTN_NCS = range(1, 8)


def attn_instance_lengths(NC):
    """First length of the NC range, the two lengths around "the last 16-key tile is all padding", the full padded length; L = 1 is NC = 1's first."""
    return sorted({32 * (NC - 1) + 1, 32 * NC - 16, 32 * NC - 15, 32 * NC})


# (B, L, H, causal): three sequences (a middle one for the isolation test), two heads (a head offset)
ATTN_INSTANCE_CASES = [(3, L, 2, causal) for NC in ATTN_NCS for causal in (False, True) for L in attn_instance_lengths(NC)]
ATTN_PEAKED_CASES = [(3, 32 * NC - 15, 2, causal) for NC in ATTN_NCS for causal in (False, True)]  # one L per NC: padding inside the last real tile
ATTN_PEAKED_GAIN = 3.0  # on q and k, as test_attention_long_forward_forms; v and dout stay O(1)


def attn_instance_launches(L, causal):
    """(bwd, flags, form) of the forward and of every backward kernel-choice flag at L <= 224: default, 2 (two kernels), 4 (fused, two blocks
    per wave), 8 (fused), and 16 (sweep) where a sweep kernel exists (no mask).  flags carry the mask in bit 0, as mudpt_attention_form takes them."""
    assert L <= 224
    c, Lp = int(causal), -(-L // 32) * 32
    default = ("BWD_FUSED_W2" if Lp <= 96 else "BWD_TWO") if causal else ("BWD_SWEEP" if Lp >= 128 else "BWD_FUSED_W2")
    calls = [(0, c, "FWD_PAIR" if causal else "FWD_PERSISTENT"), (1, c, default), (1, c | 2, "BWD_TWO"), (1, c | 4, "BWD_FUSED_W1"), (1, c | 8, "BWD_FUSED_W2")]
    return calls if causal else calls + [(1, 16, "BWD_SWEEP")]


# Long sequences, (B, L, H, causal): the staged form at its largest L and above 1024 under the mask, then the edges of the resident forms
# (forward <= 640, backward <= 608) that ATTN_CASES holds, here between guards
ATTN_LONG_CASES = [(1, 4096, 1, False), (1, 1025, 2, True),
                   (1, 225, 1, False), (2, 260, 2, True), (2, 513, 2, True), (1, 581, 3, False), (1, 608, 1, False), (1, 609, 1, True), (1, 640, 2, False),
                   (1, 641, 1, False)]


def attn_long_launches(L, causal):
    """(bwd, flags, form) at L > 224: the default and the staged form by switch (bit 1), forward and backward."""
    assert L > 224
    c, Lp = int(causal), -(-L // 32) * 32
    fwd, bwd = ("FWD_RESIDENT" if Lp * 256 <= 160 * 1024 else "FWD_STAGED"), ("BWD_RESIDENT" if Lp * 264 <= 160 * 1024 else "BWD_STAGED")
    return [(0, c, fwd), (0, c | 2, "FWD_STAGED"), (1, c, bwd), (1, c | 2, "BWD_STAGED")]


# The persistent kernels walk pairs = B * H (sequence, head) pairs with at most `cap` resident workgroups: mirrors of fwd_cfg / bwd_fused_cfg (attention.hip)
def attn_fwd_cap(NC, ncu):
    lds = 4 * NC * 32 * 128 + NC * 32 * 4
    per_cu = max(163840 // lds, 1)
    return ncu * (per_cu if per_cu * 2 * NC <= 32 else 32 // (2 * NC))


def attn_fused_cap(NC, W2, ncu):
    lds = 4 * NC * 32 * 128 + 3 * NC * 32 * 4
    return ncu * min(max(min(163840 // lds, 32 // (NC * W2)), 1), 4)


class AttnMultiPairCase(namedtuple("AttnMultiPairCase", "kernel NC L H causal")):
    """More pairs than resident workgroups of one persistent kernel ("fwd": attn_fwd_kernel, "fused_w2" / "fused_w1": attn_bwd_fused_kernel)."""
    __slots__ = ()

    @property
    def flags(self):  # of mudpt_attention_bwd; the forward takes the mask alone
        return int(self.causal) | {"fwd": 0, "fused_w2": 8, "fused_w1": 4}[self.kernel]

    @property
    def form(self):
        return {"fwd": "FWD_PERSISTENT", "fused_w2": "BWD_FUSED_W2", "fused_w1": "BWD_FUSED_W1"}[self.kernel]

    def cap(self, ncu):
        return attn_fwd_cap(self.NC, ncu) if self.kernel == "fwd" else attn_fused_cap(self.NC, 2 if self.kernel == "fused_w2" else 1, ncu)

    def batch(self, ncu):
        """Sequences on a device of ncu compute units: the fewest that give about 1.3 caps of pairs and a ragged last round."""
        cap = self.cap(ncu)
        B = -(-13 * cap // (10 * self.H))
        while B * self.H % cap == 0:
            B += 1
        return B


_MULTI_LH = {1: (17, 8), 2: (54, 12), 3: (77, 8), 4: (100, 3), 5: (150, 3), 6: (180, 3), 7: (201, 3)}  # NC -> (L, H); 54 x 12: ViT-B/32 with 4 prompt rows
ATTN_MULTI_PAIR_CASES = ([AttnMultiPairCase("fwd", NC, *_MULTI_LH[NC], False) for NC in ATTN_NCS]
                         + [AttnMultiPairCase(k, NC, *_MULTI_LH[NC], causal) for k in ("fused_w2", "fused_w1") for NC in ATTN_NCS for causal in (False, True)])

# Single-query edges, (B, L, H, causal, positions | None): under the mask position 0 (one visible key) and L - 1 in every case, L = 1 under both masks
ATTN_SINGLE_EDGE_CASES = [(4, 26, 8, True, (0, 25, 0, 13)), (3, 77, 2, True, (76, 0, 1)), (2, 1, 3, True, (0, 0)), (2, 1, 3, False, None), (3, 201, 2, False, None),
                          (2, 581, 2, True, (0, 580))]


def attention_form_launches():
    """(bwd, L, flags, sel, form) of every launch of test_attention_forms_gpu.py whose form a table above names."""
    calls = []
    for _, L, _, causal in ATTN_INSTANCE_CASES + ATTN_PEAKED_CASES:
        calls += [(bwd, L, flags, 0, form) for bwd, flags, form in attn_instance_launches(L, causal)]
    for _, L, _, causal in ATTN_LONG_CASES:
        calls += [(bwd, L, flags, 0, form) for bwd, flags, form in attn_long_launches(L, causal)]
    for c in ATTN_MULTI_PAIR_CASES:
        calls += [(0, c.L, int(c.causal), 0, "FWD_PAIR" if c.causal else "FWD_PERSISTENT")] + ([] if c.kernel == "fwd" else [(1, c.L, c.flags, 0, c.form)])
    return calls


# ---- GEMM cases of test_gemm_forms_gpu.py, kept here so that test_capi_cpu.py can check, without a GPU, which kernel forms and which regimes of
# the persistent kernel they reach ----
class GemmCase(namedtuple("GemmCase", "name form variant M N K epis slices win patch grid order lo_mode", defaults=(1, None, None, None, None, 0))):
    """One launch shape of test_gemm_forms_gpu.py: the form (capi.GEMM_FORMS) and split-K slices it must take at 256 compute units under
    `variant` (mudpt_gemm's knob), the epilogues it runs, the (pad, off) of the operand windows it overrides (GEMM_WINDOWS), (P, L) of the
    patch epilogue, -- persistent cases -- the grid and tile-order regime it is there for, and the form of the split A operand (GEMM_SPLIT_CASES)."""
    __slots__ = ()


# (pad, off) in elements, multiples of 16: an operand is the window [rows, width] at column off of a buffer whose row stride is width + pad.
# Different for every operand, so that a stride or base taken from the wrong one shows.
GEMM_WINDOWS = {"A": (48, 16), "B": (32, 32), "out0": (48, 32), "out1": (32, 16), "aux": (64, 48),
                # the low buffers of a split launch keep the BYTE row stride of their counterpart (A, B, out1): the same pad, another offset
                "A_lo": (48, 32), "B8": (32, 16), "out1_lo": (32, 32)}
GEMM_GUARD_ROWS = 32  # rows of NaN (operands) / sentinel (outputs) before and after every window
_F32, _ST, _RES, _PATCH, _SPLIT = 5, 0, 2, 4, 0x10000  # epilogues (capi.EPI_*) and mudpt_gemm's "split K allowed" bit


def _cases(stem, form, variant, M, N, Ks, epis, **kw):
    return [GemmCase(f"{stem}_k{K}", form, variant, M, N, K, epis, **kw) for K in Ks]


# Every M is ragged against its tile and against 16; N is one 16-column group past a tile edge (80, 144, 1040, 1296, 3088) or one short (1008).
GEMM_FORM_CASES = (
    _cases("t64", "T64x64", 0, 131, 80, (64, 192), (_F32, _ST, _RES))
    + _cases("t64deep", "T64x64_K128", 0, 131, 80, (128, 384), (_F32, _ST, _RES))
    # the 4-deep ring: K below / at / above its prologue depth of three K-tiles
    + _cases("ring4_v6", "T128x64_RING4", 6, 259, 80, (64, 128, 192, 256), (_F32, _ST, _RES))
    + _cases("t128_v5", "T128x128", 5, 259, 144, (64, 192), (_F32, _ST, _RES))
    + _cases("t128", "T128x128", 0, 4100, 1296, (3072,), (_F32, _RES))
    + _cases("t64_v9", "T64x64", 9, 131, 80, (192,), (_F32, _ST)) + _cases("t64deep_v10", "T64x64_K128", 10, 131, 80, (128,), (_F32, _ST))
    + _cases("t64_v10", "T64x64", 10, 131, 80, (192,), (_F32, _ST)) + _cases("t64_v12", "T64x64", 12, 131, 80, (128,), (_F32, _ST))
    + _cases("t256_res", "T256x256", 0, 16141, 1040, (64, 192), (_RES,))
    + _cases("t256_patch", "T256x256", 0, 16170, 1040, (64, 192), (_PATCH,), patch=(98, 103))  # 165 images
    + _cases("t256_v1", "T256x256", 1, 16141, 1040, (64, 192), (_F32, _ST))
    + _cases("t128x256_v2", "T128x256", 2, 16141, 1040, (192,), (_F32, _ST, _RES))
    + _cases("t256x128_v4", "T256x128", 4, 16141, 1040, (192,), (_F32, _ST, _RES))
    + _cases("splitk_deep", "SPLITK_K128", _SPLIT, 804, 784, (3072,), (_F32, _ST), slices=3)
    + _cases("splitk", "SPLITK_K64", _SPLIT, 804, 784, (1728,), (_F32, _ST), slices=3)
    # the persistent kernel.  32 x 4 = 128 tiles: every tile split into halves
    + _cases("pp_all_split", "PP", 0, 8003, 1008, (64, 192), (_F32, _ST), grid="all_split", order="one_group")
    + _cases("pp_one_ntn5", "PP", 0, 8205, 1040, (128,), (_F32, _ST), grid="one_per_workgroup", order="one_group")  # 33 x 5 = 165 tiles
    + _cases("pp_half_tail", "PP", 0, 13069, 1296, (192,), (_F32, _ST), grid="half_tile_tail", order="full_groups")  # 52 x 6 = 312 = 256 + 56
    + _cases("pp_whole_tail", "PP", 0, 19469, 1040, (64,), (_F32, _ST), grid="whole_tile_tail", order="one_group")  # 77 x 5 = 385 = 256 + 129
    + _cases("pp_leftover_ntn16", "PP", 0, 2061, 4096, (64, 192), (_F32, _ST), grid="one_per_workgroup", order="leftover_group")  # ViT-L/14's fc
    + _cases("pp_leftover_ntn13", "PP", 0, 2600, 3088, (128,), (_F32, _ST), grid="one_per_workgroup", order="leftover_group")
    # as the model launches them (model.cpp): the kv GEMM writes 2 d columns at column d of the 3 d-wide qkv buffer; the last block's dX GEMM
    # reads A = dqkv + d and B = w_in_t + d, both 3 d wide
    + _cases("pp_kv", "PP", 0, 5640, 1536, (768,), (_ST,), win={"out0": (768, 768)}, grid="one_per_workgroup", order="full_groups")
    + _cases("pp_dx_last", "PP", 0, 10763, 768, (1536,), (_F32, _ST), win={"A": (768, 768), "B": (768, 768)}, grid="one_per_workgroup", order="one_group")
)
# one ragged, strided case per form that builds the QuickGELU epilogues (the split-K forms are store-only)
GEMM_GELU_CASES = ("t64_k64", "t64deep_k128", "ring4_v6_k64", "t128_v5_k64", "t256_v1_k64", "t128x256_v2_k192", "t256x128_v4_k192", "pp_all_split_k64")
# a persistent-kernel-sized launch whose ldo0 is no multiple of 8 elements falls to a simple tile (out0 pad 4)
GEMM_REFUSAL_CASES = _cases("pp_size_ldo0_mod8", "T64x64", 0, 8003, 1008, (64,), (_F32, _ST), win={"out0": (4, 0)})


# ---- split-operand cases of test_gemm_split_forms_gpu.py: the second pass (common.h LoMode 1: T remainders against the same B; 2: e4m3
# remainders against B8) in every form a split operand can take.  K per lo_mode: the e4m3 pass needs K % 128 == 0 ----
GEMM_SPLIT_FORMS = ("PP", "T256x256", "T128x256", "T256x128", "T64x64", "T128x64_RING4", "T128x128")  # never T64x64_K128 or split K
GEMM_SPLIT_B8_SCALE = 137     # E8M0 2^10 on the weights x the kernel's 2^-12 on the activations: the e4m3 pass adds (A_lo . B8^T) / 4, exactly
GEMM_SPLIT_B8_SCALE_ONE = 139  # net factor 1


def _split_cases(stem, form, variant, M, N, Ks16, Ks8, epis, **kw):
    return [GemmCase(f"{stem}_lo{lo}_k{K}", form, variant, M, N, K, epis, lo_mode=lo, **kw) for lo, Ks in ((1, Ks16), (2, Ks8)) for K in Ks]


GEMM_SPLIT_CASES = (
    _split_cases("t64", "T64x64", 0, 131, 80, (64, 192), (128, 384), (_F32, _ST, _RES))
    + _split_cases("t64_v10", "T64x64", 10, 131, 80, (128,), (128,), (_F32, _ST))  # K = 128 must not go 128-deep with a split operand
    # the ring: nt = K-tiles of both passes below / at / above its prologue depth of three (lo_mode 1: 2, 4, 6, 8; lo_mode 2: 3, 6, 9)
    + _split_cases("ring4_v6", "T128x64_RING4", 6, 259, 80, (64, 128, 192, 256), (128, 256, 384), (_F32, _ST, _RES))
    + _split_cases("t128_v5", "T128x128", 5, 259, 144, (64, 192), (128, 384), (_F32, _ST, _RES))
    + _split_cases("t128", "T128x128", 0, 4100, 1296, (640,), (640,), (_F32, _RES))  # K > 512, or small_tiles takes the shape
    + _split_cases("t256_res", "T256x256", 0, 16141, 1040, (64, 192), (128, 384), (_RES,))
    + _split_cases("t256_v1", "T256x256", 1, 16141, 1040, (64, 192), (128, 384), (_F32, _ST))
    + _split_cases("t128x256_v2", "T128x256", 2, 16141, 1040, (192,), (128,), (_F32, _ST, _RES))
    + _split_cases("t256x128_v4", "T256x128", 4, 16141, 1040, (192,), (128,), (_F32, _ST, _RES))
    # the persistent kernel, at the shapes and (grid, order) regimes of the pp_* cases above.  K-steps per tile: lo_mode 1 2 K / 64 (always
    # even; K = 128 on one shape so that the first pass ends on either LDS stage), lo_mode 2 K / 64 + K / 128 = 3, 6, 15
    + _split_cases("pp_all_split", "PP", 0, 8003, 1008, (64, 192), (128, 256, 640), (_F32, _ST), grid="all_split", order="one_group")
    + _split_cases("pp_one_ntn5", "PP", 0, 8205, 1040, (64, 128, 192), (128, 256, 640), (_F32, _ST), grid="one_per_workgroup", order="one_group")
    + _split_cases("pp_half_tail", "PP", 0, 13069, 1296, (64, 192), (128, 256, 640), (_F32, _ST), grid="half_tile_tail", order="full_groups")
    + _split_cases("pp_whole_tail", "PP", 0, 19469, 1040, (64, 192), (128, 256, 640), (_F32, _ST), grid="whole_tile_tail", order="one_group")
    + _split_cases("pp_leftover_ntn16", "PP", 0, 2061, 4096, (64, 192), (128, 256, 640), (_F32, _ST), grid="one_per_workgroup", order="leftover_group")
)
# one case per kernel family that runs again with GEMM_SPLIT_B8_SCALE_ONE
GEMM_SPLIT_SCALE_CASES = ("t64_lo2_k128", "pp_one_ntn5_lo2_k128")
# the patch-embed epilogue on a split operand (mudpt_gemm_split_patch): the 256 x 256 tile the benchmark batch runs, and the small tile
GEMM_SPLIT_PATCH_CASES = (
    _split_cases("t256_patch", "T256x256", 0, 16170, 1040, (64, 192), (128, 384), (_PATCH,), patch=(98, 103))
    + _split_cases("t64_patch", "T64x64", 0, 392, 80, (64,), (128,), (_PATCH,), patch=(98, 103))
)
# QuickGELU epilogue with a split input and a split output: (form, variant, M, N, K for lo_mode 0 | 1, K for lo_mode 2, all mode pairs?) --
# one ragged case per form; lo_mode 0 needs K % 128 != 0 on the small tile (or it goes 128-deep)
GEMM_SPLIT_GELU_CASES = (
    GemmCase("t64", "T64x64", 0, 131, 80, (64, 128), (1,)), GemmCase("ring4_v6", "T128x64_RING4", 6, 259, 80, (64, 128), (1,)),
    GemmCase("t128_v5", "T128x128", 5, 259, 144, (64, 128), (1,)), GemmCase("t256_v1", "T256x256", 1, 16141, 1040, (64, 128), (1,)),
    GemmCase("t128x256_v2", "T128x256", 2, 16141, 1040, (192, 128), (1,)), GemmCase("t256x128_v4", "T256x128", 4, 16141, 1040, (192, 128), (1,)),
    GemmCase("pp_all_split", "PP", 0, 8003, 1008, (64, 128), (1,), grid="all_split", order="one_group"),
)
GEMM_SPLIT_GELU_ALL_PAIRS = ("t64", "pp_all_split")  # (lo_mode, out1_lo_mode) in {0, 1, 2} x {1, 2} there; {1, 2} x {1, 2} on the rest


def gemm_split_gelu_case(case, lo_mode):
    """The launch shape of a GEMM_SPLIT_GELU_CASES entry under the input form lo_mode: its K is (K for lo_mode 0 | 1, K for lo_mode 2)."""
    return case._replace(K=case.K[1 if lo_mode == 2 else 0], lo_mode=lo_mode)


def pp_ksteps(case):
    """K-steps per tile of gemm_pp_kernel: K / 64 of the first pass, then K / 64 (lo_mode 1) or K / 128 (lo_mode 2) of the second."""
    return case.K // 64 + {0: 0, 1: case.K // 64, 2: case.K // 128}[case.lo_mode]


def gemm_windows(case, windowed=True):
    return dict(GEMM_WINDOWS, **(case.win or {})) if windowed else dict.fromkeys(GEMM_WINDOWS, (0, 0))


def gemm_form_args(case, epi, ncu, windowed=True):
    """mudpt_gemm_form's arguments for epilogue `epi` of a case, with the output strides of its windows."""
    w = gemm_windows(case, windowed)
    return (epi, case.M, case.N, case.K, case.N + w["out0"][0], case.N + w["out1"][0], case.N + w["aux"][0], case.lo_mode, case.variant, ncu)


# Mirrors of launch_pp's grid arithmetic and of gemm_pp_kernel's tile order (gemm_pp.hip); GN lives in device code.
def pp_grid(M, N, ncu):
    """(tiles, grid, rem_half) of launch_pp: rem_half > 0 = that many tiles of the last, partial wave run as two half tiles each."""
    nt = -(-M // 256) * -(-N // 256)
    grid = (2 * nt if 2 * nt <= ncu else nt) if nt < ncu else ncu
    rem = nt % grid
    return nt, grid, rem if rem > 0 and 2 * rem <= grid else 0


def pp_grid_regime(M, N, ncu):
    nt, grid, rem_half = pp_grid(M, N, ncu)
    if nt < ncu:
        return "all_split" if grid == 2 * nt else "one_per_workgroup"
    return "half_tile_tail" if rem_half else ("whole_tile_tail" if nt % grid else "whole_waves")


def pp_group_width(ntn):
    return 6 if ntn >= 12 else (3 if ntn >= 6 and ntn % 3 == 0 else ntn)


def pp_order_regime(N):
    ntn = -(-N // 256)
    gn = pp_group_width(ntn)
    return "one_group" if gn == ntn else ("full_groups" if ntn % gn == 0 else "leftover_group")


def pp_tile_mn(tile, ntm, ntn):
    """tile_mn: (row panel, column tile) of the tile-th tile in the kernel's order."""
    gn = pp_group_width(ntn)
    tpg, full = ntm * gn, ntn // gn
    ng = tile // tpg
    if ng < full:
        rem = tile - ng * tpg
        return rem // gn, ng * gn + rem % gn
    wl, rem = ntn - full * gn, tile - full * tpg
    return rem // wl, full * gn + rem % wl


def pp_case_for(case, ncu):
    """A persistent case on a device of ncu compute units: itself at 256; otherwise the smallest row count (same ragged edge) that reaches its
    grid regime there, or None where none does (the kernel takes 128 tiles or more: "all_split" needs at least 256 units)."""
    if case.grid is None or pp_grid_regime(case.M, case.N, ncu) == case.grid:
        return case
    ntn = -(-case.N // 256)
    for ntm in range(-(-128 // ntn), 4 * ncu):
        M = (ntm - 1) * 256 + (case.M - 1) % 256 + 1
        if pp_grid_regime(M, case.N, ncu) == case.grid:
            return case._replace(M=M)
    return None


# ---- LayerNorm: inputs, float64 reference and derived bounds of test_layernorm_cpu.py / test_layernorm_gpu.py -----------------------------
LN_EPS = 1e-5
LN_U = 2.0 ** -24  # unit roundoff of fp32
LN_REGIMES = ("plain", "offset", "eps_dominates", "var_near_eps", "constant", "outliers", "zero")
LN_ROWS_PER_REGIME = 5  # 35 rows: the last block of four waves is partial
# one lane, a few lanes, a partly filled last 64-lane slab at k = 1, 2, 3, the full register file
LN_WIDTHS = (4, 68, 260, 516, 772, 1020, 1024)
# pad (elements) of every row stride in the strided launches: all different, so that a stride taken from the wrong operand shows
LN_PADS = {"x": 4, "out": 8, "add": 12, "xout": 16, "dy": 20, "dres": 24, "dx": 28, "dx_lp": 32}
LN_NO_PADS = dict.fromkeys(LN_PADS, 0)


def ln_regimes(rows_per_regime, d, generator):
    """[7 rows_per_regime, d] fp32: the row groups of LN_REGIMES stacked, so that one launch covers them all.
      plain          randn * 2 + 0.5: the data of every older LayerNorm test (eps moves the result by 5e-6 here)
      offset         randn * 0.05 + 300: |mean| / std = 6000, a one-pass variance cancels to garbage
      eps_dominates  randn * 1e-3 + 0.25: variance 1e-6, a tenth of eps
      var_near_eps   randn * 3e-3 - 1: variance 9e-6
      constant       rows of 0.1 alternating with rows of -7.3: variance exactly 0, a mean that summing in fp32 does not reproduce exactly
      outliers       randn with column 3 = 2000 and column d - 1 = -900
      zero           all zeros: y = beta, rstd = 1 / sqrt(eps)"""
    n = rows_per_regime
    r = lambda: torch.randn(n, d, generator=generator)  # noqa: E731
    const = torch.empty(n, d)
    const[0::2], const[1::2] = 0.1, -7.3
    outl = r()
    outl[:, 3] = 2000.0
    outl[:, d - 1] = -900.0
    return torch.cat([r() * 2 + 0.5, r() * 0.05 + 300, r() * 1e-3 + 0.25, r() * 3e-3 - 1, const, outl, torch.zeros(n, d)])


def ln_groups(rows_per_regime=LN_ROWS_PER_REGIME):
    """Regime number (index into LN_REGIMES) of every row of ln_regimes."""
    return torch.arange(len(LN_REGIMES) * rows_per_regime) // rows_per_regime


def ln_operands(rows, d, generator):
    """gamma, beta, dy, dres as elsewhere in the suite."""
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=generator), 0.1 * torch.randn(d, generator=generator)
    return gamma, beta, torch.randn(rows, d, generator=generator), torch.randn(rows, d, generator=generator)


LnRef = namedtuple("LnRef", "x mean rstd xhat y amax")
LnBwdRef = namedtuple("LnBwdRef", "dx dgamma dbeta gmax")


def ln64(x, gamma, beta, eps=LN_EPS):
    """LayerNorm from the definition in float64 (biased variance) on the fp32 values given; mean / rstd / amax as [rows, 1]."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xhat = (x - mean) * rstd
    return LnRef(x, mean, rstd, xhat, xhat * gamma + beta, x.abs().amax(-1, keepdim=True))


def ln_bwd64(ref, gamma, dy, dres=None):
    """Gradients of ln64 in float64 from the definition: dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres, exactly), g = dy gamma;
    dgamma = sum_r dy xhat, dbeta = sum_r dy; gmax = max |g| of every row.  The kernels are GIVEN mean and rstd in fp32 (ln_stats32).  dx is
    held to the definition all the same: ln_bwd_bounds carries that rounding, 16 u amax rstd on xhat.  dgamma's bound has no such term --
    half an ulp of a mean of 300 moves xhat by 3e-4 in the offset regime, the same way in every column, 15 to 80 times the bound measured on
    a faithful fp32 restatement -- so dgamma is the same sum in float64 over the operands the kernel reads: xhat = (x - fp32(mean)) fp32(rstd)."""
    dy = dy.double()
    g = dy * gamma.double()
    dx = ref.rstd * (g - g.mean(-1, keepdim=True) - ref.xhat * (g * ref.xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.double()
    mean32, rstd32 = ln_stats32(ref)
    xhat_given = (ref.x - mean32.double().unsqueeze(-1)) * rstd32.double().unsqueeze(-1)
    return LnBwdRef(dx, (dy * xhat_given).sum(0), dy.sum(0), g.abs().amax(-1, keepdim=True))


def ln_stats32(ref):
    """mean, rstd [rows] of ln64 rounded to fp32: the backward's inputs, so that a backward test does not depend on the forward kernel."""
    return ref.mean.squeeze(-1).float(), ref.rstd.squeeze(-1).float()


def ln_bounds(ref, gamma, dtype=None, lo_mode=0, hi=None):
    """Bounds on |result - ln64| of a correct fp32 two-pass LayerNorm, derived (never fitted to a kernel).  u = 2^-24, amax = max |x| of the row:
      mean   16 u amax: d terms of at most amax summed in a tree of depth <= 10 + 6 (lane, then wave), each level rounding once
      rstd   relative 16 u + (16 u amax rstd)^2 / 2.  The first term covers the sum of squares, the division, the add of eps and the
             hardware rsqrt (1 ulp).  The second is what an error dm of the centre does to a small variance: sum (x - m - dm)^2 / d =
             var + dm^2, so rstd changes by dm^2 rstd^2 / 2 relative
      y      fp32: 2e-5 (1 + |y|) + 16 u amax rstd max |gamma|: the project's constant, and the error of the mean carried through
             (x - mean) rstd gamma
             T (dtype "bf16" | "fp16"): + EPS[dtype] |y|, half an ulp of T = correct rounding (the older tests allowed 4 EPS: truncation
             passed), + 2^-25 in fp16 (half a subnormal step)
             split pair hi + lo (lo_mode 1 | 2) instead: the fp32 bound + EPS^2 |y| (lo in T: half an ulp of T relative to a remainder of
             at most half an ulp of hi; 2^-22 in fp16) or + 2^-4 EPS |y| (e4m3: 3 mantissa bits; 2^-15 in fp16).  e4m3 saturates at
             448 / 4096: where half an ulp of `hi` exceeds that (bf16, |y| >= 32) the excess is added"""
    mean = 16 * LN_U * ref.amax
    e = mean * ref.rstd
    rstd = ref.rstd * (16 * LN_U + 0.5 * e * e)
    y = 2e-5 * (1 + ref.y.abs()) + e * gamma.double().abs().max()
    if dtype is not None and lo_mode == 0:
        y = y + EPS[dtype] * ref.y.abs() + (2.0 ** -25 if dtype == "fp16" else 0.0)
    elif lo_mode == 1:
        y = y + EPS[dtype] ** 2 * ref.y.abs()
    elif lo_mode == 2:
        mant, tiny = (7, 2.0 ** -126) if dtype == "bf16" else (10, 2.0 ** -14)
        half_ulp = torch.ldexp(torch.ones(()), torch.frexp(hi.float().abs().clamp_min(tiny)).exponent - 2 - mant).double()
        y = y + 2.0 ** -4 * EPS[dtype] * ref.y.abs() + (half_ulp - 448.0 / 4096.0).clamp_min(0)
    return {"mean": mean, "rstd": rstd, "y": y}


def ln_bwd_bounds(ref, bref, dy, dtype=None):
    """Bounds on |result - ln_bwd64| of a correct fp32 backward that is given mean / rstd rounded to fp32.  G = max |dy gamma| of the row,
    e = 16 u amax rstd (the error of xhat that the rounding of the centre leaves):
      dx      2e-5 (rstd G + |dx|) + rstd G e (1 + |xhat|): the project's constant on the size of the terms, and e through
              g - mean(g) - xhat mean(g xhat) (once in xhat itself, once in the mean that xhat enters)
      dx_lp   + EPS[dtype] |dx| (correct rounding to T)
      dgamma  4e-6 sqrt(rows) x the largest |dy xhat| term of the column (test_ln_bwd_affine's bound for unit-variance terms, scaled);
      dbeta   4e-6 sqrt(rows) x the largest |dy| of the column"""
    e = 16 * LN_U * ref.amax * ref.rstd
    dx = 2e-5 * (ref.rstd * bref.gmax + bref.dx.abs()) + ref.rstd * bref.gmax * e * (1 + ref.xhat.abs())
    if dtype is not None:
        dx = dx + EPS[dtype] * bref.dx.abs()
    s = 4e-6 * dy.shape[0] ** 0.5
    return {"dx": dx, "dgamma": s * (dy.double() * ref.xhat).abs().amax(0), "dbeta": s * dy.double().abs().amax(0)}


def ln_ratios(got, want, bound, groups=None):
    """Worst |got - want| / bound of every regime ([len(LN_REGIMES)], or one number without groups): 0 / 0 counts as 0, a NaN or an
    infinity in `got` as infinite."""
    got = got.detach().double().cpu()
    if got.dim() < want.dim():
        got = got.unsqueeze(-1)
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    if groups is None:
        return ratio.max()
    ratio = ratio.reshape(len(groups), -1).amax(-1)
    return torch.stack([ratio[groups == i].max() if (groups == i).any() else torch.zeros(()) for i in range(len(LN_REGIMES))])


def ln_check(tag, what, got, want, bound, groups=None, limit=1.0, record=None):
    """Assert ln_ratios <= limit; print the ratios first; record[(what, regime)] keeps the worst ratio seen."""
    r = ln_ratios(got, want, bound, groups)
    if groups is None:
        print(f"{tag} {what}: worst error / bound {r.item():.3f}")
        if record is not None:
            record[(what, "all")] = max(record.get((what, "all"), 0.0), r.item())
    else:
        print(f"{tag} {what}: worst error / bound " + " ".join(f"{n} {v:.3f}" for n, v in zip(LN_REGIMES, r.tolist())))
        if record is not None:
            for n, v in zip(LN_REGIMES, r.tolist()):
                record[(what, n)] = max(record.get((what, n), 0.0), v)
    assert (r <= limit).all(), (tag, what, r.tolist())
    return r
