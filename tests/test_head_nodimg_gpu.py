"""The training head without an image gradient (HeadArgs::dimg == nullptr: the head of a frozen, prompt-free image tower, as on a
mudpt_create_resnet handle), through mudpt_head_ex with dimg = NULL, against the float64 head_eval of tests/test_kernels_gpu.py and, bit for
bit, against the form with dimg.  Helpers and bounds are that file's."""
import ctypes as C

import pytest
import torch

from mudpt_amd import capi
from tests.helpers import SENT, P
from tests.test_kernels_gpu import FUSED_BOUND, head_errors, head_eval, head_fits, head_inputs, measured_bound, peaked_inputs, run_head, within

pytestmark = pytest.mark.gpu

SCALE, GSCALE = 14.2857, 0.5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return capi.load()


def nodimg_fits(C_, e):
    """head.hip's rule for a training call without dimg, recomputed from include/mudpt.h: the forward's LDS -- [16][e] normalised image rows
    and [16][Cpad] logits in fp32 plus 256 bytes, within 160 KB -- and e <= 1024, a multiple of 16 (the text-side kernel's tile)."""
    Cpad = (C_ + 15) // 16 * 16
    return e % 16 == 0 and e <= 1024 and (16 * e + 16 * Cpad) * 4 + 256 <= 163840


def run_nodimg(lib, img, txt, labels, scale, gscale, path):
    """mudpt_head_ex in training with dimg = NULL.  A sentinel-filled [B, e] buffer is allocated where run_head allocates dimg, between the
    row losses and dtxt, and must come back untouched."""
    B, e = img.shape
    Cn = txt.shape[0]
    ic, tc, lc = img.cuda(), txt.cuda(), labels.cuda()
    txt_n, txt_inv = torch.full((Cn, e), SENT, device="cuda"), torch.full((Cn,), SENT, device="cuda")
    logits = torch.full((B, Cn), SENT, device="cuda")
    loss, row_loss = torch.full((1,), SENT, device="cuda"), torch.full((B,), SENT, device="cuda")
    beside, dtxt = torch.full((B, e), SENT, device="cuda"), torch.full((Cn, e), SENT, device="cuda")
    taken = C.c_int32(-1)
    rc = lib.mudpt_head_ex(P(ic), P(tc), P(lc), scale, gscale, B, 0, Cn, e, P(txt_n), P(txt_inv), P(logits), P(loss), P(row_loss), None, P(dtxt), path,
                           C.byref(taken), None)
    assert rc == 0, lib.mudpt_last_error().decode()
    torch.cuda.synchronize()
    assert (beside == SENT).all(), "the buffer beside the outputs was written although dimg was NULL"
    return {"logits": logits.cpu(), "loss": loss.cpu()[0], "row_loss": row_loss.cpu(), "dimg": None, "dtxt": dtxt.cpu(), "txt_n": txt_n.cpu(),
            "txt_inv": txt_inv.cpu()}, taken.value


# (B, C, e, the path the dispatch must take: 0 fused, 1 unfused)
CASES = [(5, 11, 64, 0),           # one partial row group
         (17, 1000, 1024, 0),      # two groups, RN50 x ImageNet: the shape the form exists for
         (4, 1520, 1024, 0), (4, 1521, 1024, 1),   # both sides of the new LDS boundary at e = 1024
         (3, 9, 1040, 1),          # beyond the text-side kernel's 64 KB
         (16, 2032, 512, 0), (16, 2033, 512, 1)]   # both sides of the boundary at e = 512


@pytest.mark.parametrize("B,Cn,e,expect", CASES)
def test_head_without_dimg_against_float64(lib, B, Cn, e, expect):
    """Logits, loss, row losses and dtxt against float64 on the path the dispatch takes (asserted, and equal to the documented rule) and on
    the forced unfused path.  Fused: the suite's FUSED_BOUND; unfused: measured_bound("unfused")."""
    assert nodimg_fits(Cn, e) == (expect == 0)
    img, txt, labels = head_inputs(B, Cn, e)
    ref = head_eval(img, txt, labels, SCALE, GSCALE, torch.float64)
    for path in (0, 1):
        out, taken = run_nodimg(lib, img, txt, labels, SCALE, GSCALE, path)
        assert taken == (expect if path == 0 else 1), (path, taken)
        err = head_errors(out, ref)
        print(f"head without dimg B {B} C {Cn} e {e} path {path} -> {'fused' if taken == 0 else 'unfused'}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert set(err) == {"logits", "loss", "row_loss", "dtxt"}
        within(err, FUSED_BOUND if taken == 0 else measured_bound("unfused"), f"path {path}")


def test_the_rule_without_dimg_is_the_forward_rule_up_to_e_1024():
    assert nodimg_fits(1000, 1024) and not head_fits(1000, 1024, True)  # RN50 x ImageNet: fused only without the gradient tile
    assert nodimg_fits(1520, 1024) and not nodimg_fits(1521, 1024) and nodimg_fits(2032, 512) and not nodimg_fits(2033, 512)
    assert not nodimg_fits(9, 1040) and head_fits(9, 1040, False) and not nodimg_fits(5, 72)
    for Cn, e in [(1000, 1024), (1521, 1024), (2032, 512), (2033, 512), (11, 64), (7, 72)]:
        assert nodimg_fits(Cn, e) == head_fits(Cn, e, False)


@pytest.mark.parametrize("B,Cn,e,path", [(17, 1000, 512, 0), (5, 496, 1024, 0), (3, 9, 1040, 1)])
def test_head_without_dimg_is_bit_identical_to_the_head_with_it(lib, B, Cn, e, path):
    """Where both forms run on the same path -- fused at (17, 1000, 512) and (5, 496, 1024), the largest class count the form with dimg
    takes at e = 1024; unfused at (3, 9, 1040) -- everything but dimg is equal bit for bit."""
    img, txt, labels = head_inputs(B, Cn, e)
    assert path == 1 or (head_fits(Cn, e, True) and nodimg_fits(Cn, e))
    full, taken_full, state = run_head(lib, img, txt, labels, SCALE, GSCALE, 0)
    out, taken = run_nodimg(lib, img, txt, labels, SCALE, GSCALE, 0)
    assert taken_full == path and taken == path
    for k in ("logits", "row_loss", "dtxt"):
        assert torch.equal(out[k], full[k]), k
    assert out["loss"] == full["loss"]
    assert torch.equal(out["txt_n"], state[0].cpu()) and torch.equal(out["txt_inv"], state[1].cpu())
    assert (full["dimg"] != SENT).all()


@pytest.mark.parametrize("path", [0, 1])
def test_head_without_dimg_peaked_rows_at_logit_scale_100(lib, path):
    """tests/test_kernels_gpu.py's peaked rows (cosine ~0.9 with one class at exp(logit_scale) = 100) without dimg, on both paths, within
    measured_bound("peaked")."""
    img, txt, labels = peaked_inputs()
    ref = head_eval(img, txt, labels, 100.0, 1.0, torch.float64)
    out, taken = run_nodimg(lib, img, txt, labels, 100.0, 1.0, path)
    assert taken == path
    err = head_errors(out, ref)
    print(f"peaked head without dimg path {path}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    within(err, measured_bound("peaked"), f"path {path}")


def test_head_ex_still_refuses_labels_without_loss(lib):
    B, Cn, e = 4, 5, 64
    f = lambda *shape: torch.full(shape, SENT, device="cuda")  # noqa: E731
    img, txt, lab = torch.randn(B, e, device="cuda"), torch.randn(Cn, e, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    tn, ti, lg = f(Cn, e), f(Cn), f(B, Cn)
    rc = lib.mudpt_head_ex(P(img), P(txt), P(lab), 1.0, 1.0, B, 0, Cn, e, P(tn), P(ti), P(lg), None, None, None, None, 0, None, None)
    assert rc == 1 and b"training needs" in lib.mudpt_last_error()
    assert (lg == SENT).all() and (tn == SENT).all()
