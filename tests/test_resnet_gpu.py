"""GPU tests of CLIP's ResNet image tower on the frozen handle (``mudpt_create_frozen_resnet``): the memory movers of resnet.hip one by one
against torch -- bit for bit, since each is a copy, a single rounding or a fixed sequence of fp32 operations -- and the whole tower against the
fixtures of the reference's own ``ModifiedResNet`` inside its ``ZeroshotCLIP`` / ``ZeroshotCLIP2`` (tests/golden/gen_golden_resnet.py).

The feature bound is 3 x ``emulated_rel``: the float64 restatement with rounding to T at the library's five sites (tests/resnet_reference.py)
against the reference's features, computed by the generator on the CPU; the factor covers fp32 accumulation in another order, another sample
of the same rounding noise and toolchain changes.  The logits are held to helpers.check_logits, the project's bounds at logit scale 14.29."""
import pytest
import torch

from mudpt_amd import capi
from tests import resnet_reference as R
from tests.helpers import SENT, check_logits, ok, refused

pytestmark = pytest.mark.gpu
DTYPES = {"fp16": (capi.F16, torch.float16), "bf16": (capi.BF16, torch.bfloat16)}
GUARD = 3  # rows of SENT before and after every destination


def build(case, dtype, max_batch=None, state=None, tokens=None):
    from mudpt_amd.zsclip import FrozenCLIP
    return FrozenCLIP(case.shape(), case.state if state is None else state, case.tokens if tokens is None else tokens, max_batch=max_batch or len(case.labels), dtype=dtype)


def guarded(rows, ld, T):
    """(buffer [GUARD + rows + GUARD, ld] of SENT, its rows GUARD .. GUARD + rows: the destination)."""
    buf = torch.full((rows + 2 * GUARD, ld), SENT, dtype=T, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def untouched(buf, rows, cols=None):
    """The guard rows, and the columns from `cols` on, still hold SENT."""
    assert (buf[:GUARD] == SENT).all() and (buf[GUARD + rows:] == SENT).all()
    assert cols is None or (buf[GUARD:GUARD + rows, cols:] == SENT).all()


def bits(t):
    return t.contiguous().view(torch.int16)


def patch_rows(x, stride, ldk):
    """x [B, H, W, C] -> [B Ho Wo, ldk]: column (ky * 3 + kx) * C + c of a 3 x 3, pad 1 window, zeros outside the image and from 9 C on."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=x.dtype, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    taps = [xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] for ky in range(3) for kx in range(3)]
    out = torch.zeros(B * Ho * Wo, ldk, dtype=x.dtype, device=x.device)
    out[:, :9 * C] = torch.stack(taps, dim=3).reshape(B * Ho * Wo, 9 * C)
    return out


def nhwc(B, H, W, C, lds, T, seed):
    """(storage [B H W, lds], the [B, H, W, C] view of its first C channels); the channels behind C are NaN: nothing may read them."""
    g = torch.Generator().manual_seed(seed)
    store = torch.full((B * H * W, lds), float("nan"), dtype=T, device="cuda")
    store[:, :C] = torch.randn(B * H * W, C, generator=g).to(T).cuda()
    return store, store[:, :C].reshape(B, H, W, C)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,H,W,C,lds,stride,ldk", [(2, 5, 7, 8, 8, 1, 128), (2, 6, 6, 32, 48, 1, 320), (2, 7, 6, 16, 16, 2, 192), (3, 64, 64, 8, 8, 1, 72)])
def test_im2col_nhwc(dtype, B, H, W, C, lds, stride, ldk):
    """Odd extents, a channel stride above C, both strides, a ldk tail (and none), more than one block (the last case: 12 288 rows of 9 chunks);
    then a second, smaller call into the same buffer, whose border taps and tail must be written as zeros over the first call's values."""
    code, T = DTYPES[dtype]
    lib = capi.load()
    store, x = nhwc(B, H, W, C, lds, T, 1)
    want = patch_rows(x, stride, ldk)
    buf, dst = guarded(want.shape[0], ldk, T)
    ok(lib, capi.call("mudpt_im2col", dtype=code, src=store, src_planar=0, B=B, H=H, W=W, C=C, lds=lds, stride=stride, dst=dst, ldk=ldk))
    assert torch.equal(bits(dst), bits(want))
    untouched(buf, want.shape[0])
    store2, x2 = nhwc(1, 3, 3, C, lds, T, 2)
    want2 = patch_rows(x2, stride, ldk)
    ok(lib, capi.call("mudpt_im2col", dtype=code, src=store2, src_planar=0, B=1, H=3, W=3, C=C, lds=lds, stride=stride, dst=dst, ldk=ldk))
    n2 = want2.shape[0]
    assert torch.equal(bits(dst[:n2]), bits(want2)) and torch.equal(bits(dst[n2:]), bits(want[n2:]))
    untouched(buf, want.shape[0])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,S,stride,ldk", [(2, 10, 2, 64), (2, 9, 2, 32), (1, 5, 1, 64)])
def test_im2col_planar_pixels(dtype, B, S, stride, ldk):
    """The stem's first convolution: fp32 planar pixels, rounded to T once, channel fastest inside a tap."""
    code, T = DTYPES[dtype]
    lib = capi.load()
    img = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(3)).cuda()
    want = patch_rows(img.permute(0, 2, 3, 1).to(T), stride, ldk)
    buf, dst = guarded(want.shape[0], ldk, T)
    ok(lib, capi.call("mudpt_im2col", dtype=code, src=img, src_planar=1, B=B, H=S, W=S, C=3, lds=0, stride=stride, dst=dst, ldk=ldk))
    assert torch.equal(bits(dst), bits(want))
    untouched(buf, want.shape[0])


def test_im2col_refusals():
    lib = capi.load()
    store, _ = nhwc(1, 4, 4, 8, 8, torch.float16, 1)
    buf, dst = guarded(16, 128, torch.float16)
    args = dict(dtype=capi.F16, src=store, src_planar=0, B=1, H=4, W=4, C=8, lds=8, stride=1, dst=dst, ldk=128)
    for change, word in (({"ldk": 64}, "ldk"), ({"ldk": 100}, "ldk"), ({"stride": 3}, "stride"), ({"C": 12, "ldk": 128}, "C % 8"), ({"lds": 4}, "channel stride"),
                         ({"src_planar": 1}, "3 channels"), ({"src": None}, "null"), ({"B": 0}, "empty"), ({"dtype": 2}, "dtype")):
        refused(lib, capi.call("mudpt_im2col", **dict(args, **change)), word)
    assert (buf == SENT).all()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
def test_bias_act(dtype, residual, relu):
    """M 37, N 48, every row stride above N: out = T(act((acc + bias) + residual)) with both adds in fp32 -- the same IEEE operations in torch."""
    code, T = DTYPES[dtype]
    lib = capi.load()
    M, N, ldacc, ldres, ldo = 37, 48, 52, 64, 56
    g = torch.Generator().manual_seed(5)
    acc = torch.full((M, ldacc), float("nan"), device="cuda")
    acc[:, :N] = torch.randn(M, N, generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda()
    res = torch.full((M, ldres), float("nan"), dtype=T, device="cuda")
    res[:, :N] = torch.randn(M, N, generator=g).to(T).cuda()
    v = acc[:, :N] + bias
    if residual:
        v = v + res[:, :N].float()
    want = (torch.where(v < 0, torch.zeros_like(v), v) if relu else v).to(T)
    buf, dst = guarded(M, ldo, T)
    ok(lib, capi.call("mudpt_bias_act", dtype=code, acc=acc, ldacc=ldacc, bias=bias, residual=res if residual else None, ldres=ldres, out=dst, ldo=ldo, M=M, N=N, relu=relu))
    assert torch.equal(bits(dst[:, :N]), bits(want))
    untouched(buf, M, N)
    if relu:
        assert (dst[:, :N] >= 0).all() and (dst[:, :N] == 0).any()
    ok(lib, capi.call("mudpt_bias_act", dtype=code, acc=acc, ldacc=ldacc, residual=res if residual else None, ldres=ldres, out=dst, ldo=ldo, M=M, N=N, relu=relu))  # no bias
    v = acc[:, :N] + res[:, :N].float() if residual else acc[:, :N]
    assert torch.equal(bits(dst[:, :N]), bits((torch.where(v < 0, torch.zeros_like(v), v) if relu else v).to(T)))
    for change, word in (({"N": 44}, "N % 8"), ({"ldo": 40}, "ldo"), ({"ldacc": 50}, "ldacc"), ({"acc": None}, "null")):
        before = buf.clone()
        refused(lib, capi.call("mudpt_bias_act", **dict(dict(dtype=code, acc=acc, ldacc=ldacc, bias=bias, out=dst, ldo=ldo, M=M, N=N, relu=relu), **change)), word)
        assert torch.equal(bits(buf), bits(before))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,H,W,C,lds,ldo,k", [(2, 6, 4, 16, 24, 32, 2), (1, 5, 7, 8, 8, 8, 2), (2, 6, 6, 8, 16, 8, 3)])
def test_avgpool2d(dtype, B, H, W, C, lds, ldo, k):
    """The fp32 sum in window order times 1 / k^2, one rounding: bit for bit the same operations in torch; within one rounding of the float64
    mean.  Odd extents drop the last row / column as AvgPool2d does."""
    code, T = DTYPES[dtype]
    lib = capi.load()
    store, x = nhwc(B, H, W, C, lds, T, 7)
    Ho, Wo = H // k, W // k
    s = torch.zeros(B, Ho, Wo, C, device="cuda")
    for dy in range(k):
        for dx in range(k):
            s = s + x[:, dy:dy + k * Ho:k, dx:dx + k * Wo:k].float()
    want = (s * torch.tensor(1.0 / (k * k), dtype=torch.float32)).to(T).reshape(B * Ho * Wo, C)
    buf, dst = guarded(B * Ho * Wo, ldo, T)
    ok(lib, capi.call("mudpt_avgpool2d", dtype=code, src=store, lds=lds, dst=dst, ldo=ldo, B=B, H=H, W=W, C=C, k=k))
    assert torch.equal(bits(dst[:, :C]), bits(want))
    untouched(buf, B * Ho * Wo, C)
    mean64 = x[:, :k * Ho, :k * Wo].double().reshape(B, Ho, k, Wo, k, C).mean(dim=(2, 4)).reshape(-1, C)
    assert ((dst[:, :C].double() - mean64).abs() <= 2 * (2.0 ** -8 if dtype == "bf16" else 2.0 ** -11) * mean64.abs() + 1e-7).all()
    refused(lib, capi.call("mudpt_avgpool2d", dtype=code, src=store, lds=lds, dst=dst, ldo=ldo, B=B, H=H, W=W, C=C + 4, k=k), "C % 8")
    refused(lib, capi.call("mudpt_avgpool2d", dtype=code, src=store, lds=lds, dst=dst, ldo=ldo, B=B, H=H, W=W, C=C, k=H + 1), "k=")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,HW,C,lds,ldo", [(3, 4, 64, 64, 64), (2, 49, 128, 136, 144)])
def test_attnpool_tokens(dtype, B, HW, C, lds, ldo):
    """Row 0 = (the fp32 sum over the pixels in order) x fp32(1 / HW) + pos[0]; row 1 + l = pixel l + pos[1 + l]; every element rounded once."""
    code, T = DTYPES[dtype]
    lib = capi.load()
    g = torch.Generator().manual_seed(11)
    store = torch.full((B * HW, lds), float("nan"), dtype=T, device="cuda")
    store[:, :C] = torch.randn(B * HW, C, generator=g).to(T).cuda()
    x = store[:, :C].reshape(B, HW, C).float()
    pos = (torch.randn(HW + 1, C, generator=g) * 0.3).cuda()
    s = torch.zeros(B, C, device="cuda")
    for l in range(HW):
        s = s + x[:, l]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(HW), dtype=torch.float32)
    want = torch.cat([(s * inv.cuda() + pos[0])[:, None], x + pos[1:]], dim=1).to(T).reshape(B * (HW + 1), C)
    buf, dst = guarded(B * (HW + 1), ldo, T)
    ok(lib, capi.call("mudpt_attnpool_tokens", dtype=code, src=store, lds=lds, pos=pos, dst=dst, ldo=ldo, B=B, HW=HW, C=C))
    assert torch.equal(bits(dst[:, :C]), bits(want))
    untouched(buf, B * (HW + 1), C)
    refused(lib, capi.call("mudpt_attnpool_tokens", dtype=code, src=store, lds=lds, dst=dst, ldo=ldo, B=B, HW=HW, C=C), "null")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,L,H", [(3, 5, 8), (2, 50, 32), (5, 10, 3)])
def test_attnpool_attend(dtype, B, L, H):
    """softmax(q k^T / 8) v per (image, head) in fp32 against float64: within one rounding to T plus the fp32 sums; k and v interleaved in one
    buffer as the tower's k_proj | v_proj GEMM leaves them.  (5, 10, 3): 15 pairs, the last block of four waves is partial."""
    code, T = DTYPES[dtype]
    lib = capi.load()
    g = torch.Generator().manual_seed(13)
    C = H * 64
    q = (torch.randn(B, C, generator=g) * 2).cuda()
    kv = torch.randn(B * L, 2 * C, generator=g).cuda()
    qh = (q.double() * 0.125).reshape(B, H, 1, 64)
    kh, vh = (kv[:, i * C:(i + 1) * C].double().reshape(B, L, H, 64).transpose(1, 2) for i in (0, 1))
    want = (torch.softmax(qh @ kh.transpose(-1, -2), dim=-1) @ vh).reshape(B, C)
    buf, dst = guarded(B, C + 8, T)
    ok(lib, capi.call("mudpt_attnpool_attend", dtype=code, q=q, ldq=C, k=kv, v=kv[:, C:], ldkv=2 * C, out=dst, ldo=C + 8, B=B, L=L, H=H))
    eps = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    assert ((dst[:, :C].double() - want).abs() <= eps * want.abs() + 1e-5).all()
    untouched(buf, B, C)
    refused(lib, capi.call("mudpt_attnpool_attend", dtype=code, q=q, ldq=C - 1, k=kv, v=kv[:, C:], ldkv=2 * C, out=dst, ldo=C + 8, B=B, L=L, H=H), "strides")


# ---- the tower --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_features_and_logits_match_the_reference(name, dtype):
    """Measured on an MI355X, |F - reference| / |reference| (emulated_rel in brackets): DESIGN.md 4.9 holds the table."""
    case = R.case(name)
    B = len(case.labels)
    m = build(case, dtype)
    raw = m.encode_image(case.images)
    assert torch.equal(m.debug_read("image_features", B).view(B, -1), raw.cpu())
    logits = m(case.images)
    assert torch.equal(m.image_features(), raw)
    txt = m.text_features().cpu()
    m.close()
    rel, bound = R.feature_error(raw, case.image_features), 3 * case.emulated_rel[dtype]
    print(f"{name} {dtype}: raw image features, relative: {rel:.3e} (emulated {case.emulated_rel[dtype]:.3e}, bound {bound:.3e}); "
          f"text features max {(txt - case.text_features).abs().max().item():.3e}")
    assert rel <= bound, (rel, bound)
    check_logits(logits, case, dtype, f"{name} {dtype}")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["rn_tiny", "rn_tiny2"])
def test_features_of_an_image_do_not_depend_on_its_batch(name, dtype):
    """No GEMM of the tower splits its contraction, so an image's features are the same bits alone and in a batch."""
    case = R.case(name)
    m = build(case, dtype)
    whole = m.encode_image(case.images)
    for i in range(len(case.labels)):
        assert torch.equal(m.encode_image(case.images[i:i + 1])[0], whole[i]), i
    m.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_the_flow_behind_the_tower(dtype):
    """forward_features(encode_image(x)) is forward(x) bit for bit, and the linear-probe extractor returns those features."""
    from mudpt_amd import lpclip
    case = R.case("rn_tiny2")
    m = build(case, dtype)
    logits = m(case.images)
    feat = m.encode_image(case.images)
    assert torch.equal(m.forward_features(feat), logits)
    got, labels = lpclip.extract_features(m, [{"img": case.images[:1], "label": case.labels[:1]}, {"img": case.images[1:], "label": case.labels[1:]}])
    assert torch.equal(got, feat.cpu()) and torch.equal(labels, case.labels)
    m.close()


def test_missing_weights_and_refolding():
    """Until the last visual.* tensor is there the tower's entry points answer MUDPT_ERR_STATE with a missing key while the text side already
    works; a BatchNorm tensor uploaded again is folded again at the next forward; integer tensors of a state dict are skipped."""
    case = R.case("rn_tiny")
    key = "visual.layer2.0.downsample.1.running_var"
    state = {k: v for k, v in case.state.items() if k != key}
    state["visual.bn1.num_batches_tracked"] = torch.tensor(7)
    m = build(case, "fp16", state=state)
    txt = m.text_features()
    for call in (lambda: m(case.images), lambda: m.encode_image(case.images)):
        with pytest.raises(capi.MudptError, match="bad state.*" + key.replace(".", "\\.")):
            call()
    feat = torch.zeros(len(case.labels), case.cfg.embed_dim) + case.image_features
    cached = m.forward_features(feat)  # needs no visual.* weight
    m.set_weight(key, case.state[key])
    ok(m.lib, m.lib.mudpt_set_weight(m._h, b"visual.layer1.0.bn3.num_batches_tracked", capi.ptr(torch.ones(1)), 1))
    ref = build(case, "fp16")
    want, want_logits = ref.encode_image(case.images), ref(case.images)
    assert torch.equal(m.encode_image(case.images), want) and torch.equal(m(case.images), want_logits) and torch.equal(m.text_features(), txt)
    assert torch.equal(ref.forward_features(feat), cached)
    m.set_weight("visual.bn1.weight", 2 * case.state["visual.bn1.weight"])
    changed = m.encode_image(case.images)
    assert R.feature_error(changed, want) > 1e-2
    m.set_weight("visual.bn1.weight", case.state["visual.bn1.weight"])
    assert torch.equal(m.encode_image(case.images), want)
    with pytest.raises(AssertionError, match="visual.conv1.weight expects 432 elements"):
        m.set_weight("visual.conv1.weight", torch.zeros(16, 3, 16, 16))
    with pytest.raises(AssertionError, match="unknown key 'visual.proj'"):
        m.set_weight("visual.proj", torch.zeros(4))
    m.close()
    ref.close()


def test_refusals_of_the_python_layer():
    from mudpt_amd.model import CustomCLIP
    case = R.case("rn_tiny")
    with pytest.raises(AssertionError, match="ResNet towers run in bf16 / fp16; the parity mode is not built for them"):
        build(case, "fp32")
    with pytest.raises(AssertionError, match="ResNet backbones run on the frozen handle only \\(ZeroshotCLIP, ZeroshotCLIP2, feature extraction\\)"):
        CustomCLIP(case.shape(), case.state, case.tokens[0])
