"""No-GPU checks of the fused convolution's entry points (``mudpt_conv2d``, ``mudpt_conv2d_form``, ``mudpt_resnet_conv_path``): declared, exported,
every refusal of the launcher answered on the host with MUDPT_ERR_ARG and a word that names the argument, and the tile rule held to a table."""
import os

import pytest
import torch

from mudpt_amd import build, capi


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        build.build_library()
    return capi.load()


def refused(lib, rc, word):
    msg = lib.mudpt_last_error().decode()
    assert rc == 1 and word in msg, (rc, word, msg)


def test_declared_exported_and_built(lib):
    for name in ("mudpt_conv2d", "mudpt_conv2d_form", "mudpt_resnet_conv_path"):
        assert name in capi.DECLARATIONS and hasattr(lib, name), name
    assert [n for n, _ in capi.DECLARATIONS["mudpt_conv2d"][1]] == ["dtype", "src", "B", "H", "W", "C", "lds", "k", "stride", "w", "ldk", "bias", "residual", "ldres",
                                                                   "out", "ldo", "N", "relu", "stream"]
    assert [n for n, _ in capi.DECLARATIONS["mudpt_resnet_conv_path"][1]] == ["m", "path"]
    assert "conv.hip" in build.SOURCES


def test_conv2d_refusals(lib):
    """Host memory stands in for the operands: every case is refused before anything could read it."""
    x = torch.zeros(2 * 4 * 4 * 16, dtype=torch.float16)
    w = torch.zeros(32 * 160, dtype=torch.float16)
    bias = torch.zeros(32)
    res = torch.zeros(32 * 40, dtype=torch.float16)
    out = torch.full((32 * 40,), -1234.5, dtype=torch.float16)
    assert all(t.data_ptr() % 16 == 0 for t in (x, w, bias, res, out))
    args = dict(dtype=capi.F16, src=x, B=2, H=4, W=4, C=16, lds=16, k=3, stride=1, w=w, ldk=160, bias=bias, residual=res, ldres=40, out=out, ldo=40, N=32, relu=1)
    cases = [({"dtype": 2}, "dtype"), ({"src": None}, "null"), ({"w": None}, "null"), ({"out": None}, "null"),
             ({"B": 0}, "B=0"), ({"H": 0}, "H=0"), ({"W": -1}, "W=-1"), ({"C": 0}, "C=0"), ({"N": 0}, "N=0"),
             ({"k": 2}, "k 2"), ({"k": 5}, "k 5"), ({"stride": 0}, "stride 0"), ({"stride": 3}, "stride 3"), ({"k": 1, "stride": 2}, "stride 2"),
             ({"C": 12}, "C 12"), ({"lds": 8}, "lds 8"), ({"lds": 20}, "lds 20"), ({"ldk": 136}, "ldk 136"), ({"ldk": 148}, "ldk 148"),
             ({"N": 24}, "N 24"), ({"ldo": 24}, "ldo 24"), ({"ldo": 42}, "ldo 42"), ({"ldres": 24}, "ldres 24"), ({"ldres": 42}, "ldres 42"),
             ({"src": x[4:]}, "aligned"), ({"w": w[4:]}, "aligned"), ({"out": out[4:]}, "aligned"), ({"residual": res[4:]}, "aligned"), ({"bias": bias[1:]}, "aligned"),
             ({"B": 1 << 20, "H": 1 << 10, "W": 1 << 10}, "31 bits")]
    for change, word in cases:
        refused(lib, capi.call("mudpt_conv2d", **dict(args, **change)), word)
    assert (out == -1234.5).all()


def test_resnet_conv_path_refusals(lib):
    refused(lib, lib.mudpt_resnet_conv_path(None, 1), "null")
    refused(lib, lib.mudpt_resnet_conv_path(None, 2), "null")


def test_conv2d_form_table(lib):
    """The first rule that matches, in tiles against 256 compute units: N > 64 and >= 256 tiles of 128 x 128; >= 256 tiles of 128 x 64; 64 x 64.
    The brackets of each threshold, and the tower's own shapes (RN50 at B 100: stage 1 and the stem on 128-pixel tiles, stage 4 on 64 x 64)."""
    T128x128, T128x64, T64x64 = (capi._DEFINES["CONV_" + n] for n in ("T128x128", "T128x64", "T64x64"))
    assert (T128x128, T128x64, T64x64) == (0, 1, 2)
    table = [((128 * 255 + 1, 128), T128x128), ((128 * 255, 128), T128x64), ((128 * 127 + 1, 144), T128x128), ((128 * 127, 144), T128x64),
             ((128 * 127, 128), T64x64), ((128 * 127 + 1, 128), T128x64), ((128 * 255 + 1, 64), T128x64), ((128 * 255, 64), T64x64), ((1 << 24, 64), T128x64),
             ((1 << 24, 16), T128x64), ((70, 16), T64x64), ((1200, 192), T64x64),
             ((100 * 56 * 56, 64), T128x64), ((100 * 56 * 56, 256), T128x128), ((100 * 28 * 28, 512), T128x128), ((100 * 14 * 14, 256), T128x128),
             ((100 * 7 * 7, 512), T128x64), ((100 * 7 * 7, 2048), T128x128), ((32 * 7 * 7, 512), T64x64)]
    for (M, N), want in table:
        assert lib.mudpt_conv2d_form(M, N) == want, (M, N)
    assert lib.mudpt_conv2d_form(0, 64) == -1 and lib.mudpt_conv2d_form(64, 0) == -1
