"""Timing of CLIP's ResNet image tower on the frozen handle (mudpt_create_frozen_resnet) on one MI355X: random-init RN50 / RN101, synthetic
images.  A measurement, not a test: nothing here is a bound.

    python tools/resnet_bench.py [--models RN50,RN101] [--batches 100,256] [--dtypes fp16,bf16] [--iters 5] [--rounds 5] [--no-split] [--ours-only]

Per (model, batch, dtype), in ONE process and in alternating rounds (ours, fused, yardstick, ViT, ours, ...): median and min-max of `rounds`
rounds of `iters` encode_image calls, device-synchronised, for
  ours       FrozenCLIP.encode_image on the ResNet handle (im2col + MFMA GEMM per convolution, mudpt_amd/csrc/resnet.hip);
  fused      the same on a second handle with rn_fused_conv=True (one mudpt_conv2d launch per convolution, mudpt_amd/csrc/conv.hip);
  yardstick  the same tower written below as plain torch.nn modules (eval-mode BatchNorm, AvgPool2d, F.scaled_dot_product_attention for the
             pool) in T and channels_last on torch-ROCm: what a user gets without this library;
  vit        the ViT-B/16 frozen handle's encode_image of the same process, batch and dtype (the project's flagship tower, as a scale).
Then the time split of ours by kernel class -- patch rows / GEMM / epilogue / pool -- from HIP events around every launch of a replay of the
tower's launch list through the single-kernel exports (mudpt_im2col, mudpt_gemm epilogue 5, mudpt_bias_act, mudpt_avgpool2d; the attention
pool's four small launches are not replayed).  An event pair adds queue time per launch, so the split's sum is above the forward's time: read
the shares, not the sum.  The same replay for the fused path: the stem's patch rows, one mudpt_conv2d per convolution ("conv"), the pools.
--ours-only leaves the yardstick and the ViT out (the two paths against each other, in less time)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch import nn

from mudpt_amd import capi, synth
from mudpt_amd.model import ModelShape
from mudpt_amd.zsclip import FrozenCLIP

TORCH_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}


def up64(v):
    return (v + 63) // 64 * 64


class TorchTower(nn.Module):
    """The yardstick: ModifiedResNet's arithmetic as a flat list of torch modules, built from a state dict's shapes."""

    def __init__(self, shape, sd):
        super().__init__()
        self.stages, self.heads = shape.v_stages, shape.v_heads
        self.p = nn.ParameterDict({k.replace(".", "_"): nn.Parameter(v.clone(), requires_grad=False) for k, v in sd.items() if k.startswith("visual.")})

    def cb(self, x, conv, bn, stride=1):
        g = lambda n: self.p[(n).replace(".", "_")]  # noqa: E731
        w = g(conv + ".weight")
        x = F.conv2d(x, w, None, stride, w.shape[-1] // 2)
        return F.batch_norm(x, g(bn + ".running_mean"), g(bn + ".running_var"), g(bn + ".weight"), g(bn + ".bias"), False, 0.0, 1e-5)

    def forward(self, x):
        x = x.to(self.p["visual_conv1_weight"].dtype).contiguous(memory_format=torch.channels_last)
        x = F.relu(self.cb(x, "visual.conv1", "visual.bn1", 2))
        x = F.relu(self.cb(x, "visual.conv2", "visual.bn2"))
        x = F.avg_pool2d(F.relu(self.cb(x, "visual.conv3", "visual.bn3")), 2)
        for s, blocks in enumerate(self.stages):
            for i in range(blocks):
                p, stride = f"visual.layer{s + 1}.{i}.", 2 if (s > 0 and i == 0) else 1
                y = F.relu(self.cb(x, p + "conv1", p + "bn1"))
                y = F.relu(self.cb(y, p + "conv2", p + "bn2"))
                y = F.avg_pool2d(y, stride) if stride > 1 else y
                if i == 0:
                    x = self.cb(F.avg_pool2d(x, stride) if stride > 1 else x, p + "downsample.0", p + "downsample.1")
                x = F.relu(self.cb(y, p + "conv3", p + "bn3") + x)
        B, C, H, W = x.shape
        t = x.flatten(2).transpose(1, 2)
        t = torch.cat([t.mean(dim=1, keepdim=True), t], dim=1) + self.p["visual_attnpool_positional_embedding"]
        lin = lambda v, n: F.linear(v, self.p[f"visual_attnpool_{n}_weight"], self.p[f"visual_attnpool_{n}_bias"])  # noqa: E731
        q = lin(t[:, :1], "q_proj").reshape(B, 1, self.heads, 64).transpose(1, 2)
        k, v = (lin(t, n).reshape(B, H * W + 1, self.heads, 64).transpose(1, 2) for n in ("k_proj", "v_proj"))
        return lin(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, C), "c_proj")


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def launch_list(shape):
    """(kind, arguments) of the tower's convolution and pooling launches in order, as mudpt_amd/csrc/model.cpp resnet_forward sequences them:
    ("conv", cin, cout, k, H, stride, ld_in, np) and ("pool", H, C, k)."""
    w, S = shape.v_width, shape.image_size
    out = [("conv", 3, w // 2, 3, S, 2, 0, w // 2), ("conv", w // 2, w // 2, 3, S // 2, 1, w // 2, w // 2), ("conv", w // 2, w, 3, S // 2, 1, w // 2, up64(w)),
           ("pool", S // 2, up64(w), 2)]
    H, inplanes, ldx = S // 4, w, up64(w)
    for s, blocks in enumerate(shape.v_stages):
        planes = w << s
        for i in range(blocks):
            stride = 2 if (s > 0 and i == 0) else 1
            out += [("conv", inplanes, planes, 1, H, 1, ldx, planes), ("conv", planes, planes, 3, H, 1, planes, up64(planes))]
            if stride > 1:
                out += [("pool", H, up64(planes), stride), ("pool", H, ldx, stride)]
            Ho = H // stride
            if i == 0:
                out.append(("conv", inplanes, 4 * planes, 1, Ho, 1, ldx, 4 * planes))
            out.append(("conv", planes, 4 * planes, 1, Ho, 1, up64(planes), 4 * planes))
            inplanes, ldx, H = 4 * planes, 4 * planes, Ho
    return out


def class_split(shape, B, dtype, passes=3, fused=False):
    """ms per kernel class of one forward's convolution / pooling launches, the median over `passes` replays; fused: of the mudpt_conv2d path."""
    code, T = {"fp16": capi.F16, "bf16": capi.BF16}[dtype], TORCH_DTYPE[dtype]
    launches = launch_list(shape)
    px = lambda H, stride=1: ((H - 1) // stride + 1) ** 2  # noqa: E731
    act = max(px(a[4], a[5]) * max(a[7], a[6]) if a[0] == "conv" else a[1] ** 2 * a[2] for a in launches)
    rows = max(px(a[4], a[5]) * up64(9 * a[1]) for a in launches if a[0] == "conv" and a[3] == 3)
    src, dst = (torch.randn(B * max(act, 3 * shape.image_size ** 2), device="cuda").to(T) for _ in range(2))
    pixels = torch.randn(B, 3, shape.image_size, shape.image_size, device="cuda")
    patch = torch.zeros(B * rows, dtype=T, device="cuda")
    acc = torch.zeros(B * act, device="cuda")
    wmax = max(a[7] * up64(a[3] * a[3] * a[1]) for a in launches if a[0] == "conv")
    weight, bias = torch.randn(wmax, device="cuda").to(T) * 0.01, torch.zeros(8192, device="cuda")
    out = []
    for _ in range(passes):
        evs = []

        def run(cls, name, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.check(capi.call(name, stream=torch.cuda.current_stream().cuda_stream, **kw), name)
            e1.record()
            evs.append((cls, e0, e1))
        for a in launches:
            if a[0] == "pool":
                run("pool", "mudpt_avgpool2d", dtype=code, src=src, lds=a[2], dst=dst, ldo=a[2], B=B, H=a[1], W=a[1], C=a[2], k=a[3])
                continue
            _, cin, cout, k, H, stride, ld_in, np_ = a
            ldk, M = up64(k * k * cin), B * px(H, stride)
            if fused:
                if cin == 3:  # the planar pixels keep their patch rows; the kernel runs over them as a 1 x 1
                    run("patch rows", "mudpt_im2col", dtype=code, src=pixels, src_planar=1, B=B, H=H, W=H, C=3, lds=0, stride=stride, dst=patch, ldk=ldk)
                    run("conv", "mudpt_conv2d", dtype=code, src=patch, B=B, H=(H - 1) // stride + 1, W=(H - 1) // stride + 1, C=ldk, lds=ldk, k=1, stride=1, w=weight, ldk=ldk,
                        bias=bias, out=dst, ldo=np_, N=np_, relu=1)
                else:
                    run("conv", "mudpt_conv2d", dtype=code, src=src, B=B, H=H, W=H, C=cin, lds=ld_in, k=k, stride=stride, w=weight, ldk=ldk, bias=bias, residual=src, ldres=np_,
                        out=dst, ldo=np_, N=np_, relu=1)
                continue
            if k == 3:
                run("patch rows", "mudpt_im2col", dtype=code, src=pixels if cin == 3 else src, src_planar=int(cin == 3), B=B, H=H, W=H, C=cin, lds=ld_in, stride=stride,
                    dst=patch, ldk=ldk)
            run("gemm", "mudpt_gemm", dtype=code, epilogue=capi.EPI_STORE_F32, M=M, N=np_, K=ldk, A=patch if k == 3 else src, lda=ldk if k == 3 else ld_in, B=weight, ldb=ldk,
                out0=acc, ldo0=np_)
            run("epilogue", "mudpt_bias_act", dtype=code, acc=acc, ldacc=np_, bias=bias, residual=src, ldres=np_, out=dst, ldo=np_, M=M, N=np_, relu=1)
        torch.cuda.synchronize()
        ms = {}
        for cls, e0, e1 in evs:
            ms[cls] = ms.get(cls, 0.0) + e0.elapsed_time(e1)
        out.append(ms)
    flop = sum(2.0 * B * px(a[4], a[5]) * a[7] * up64(a[3] * a[3] * a[1]) for a in launches if a[0] == "conv")
    return {c: statistics.median(o[c] for o in out) for c in out[0]}, flop, sum(1 for a in launches if a[0] == "conv")


def print_split(tag, split, flop, convs, gemm_class):
    total = sum(split.values())
    print(f"{tag} split over {convs} convolutions: " + ", ".join(f"{c} {v:6.2f} ms ({v / total * 100:2.0f} %)" for c, v in split.items())
          + f"; sum {total:.2f} ms; GEMM {flop / 1e12:.2f} TFLOP -> {flop / split[gemm_class] / 1e9:.0f} TFLOP/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="RN50,RN101")
    ap.add_argument("--batches", default="100,256")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--ours-only", action="store_true")
    a = ap.parse_args()
    tok = synth.bench_tokenized_prompts()
    vit_shape = ModelShape(n_ctx=0, depth=1)
    vit_state = synth.random_clip_state(vit_shape, 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    for name in a.models.split(","):
        shape = ModelShape(**synth.RESNET_SHAPES[name], n_ctx=0, depth=1)
        state = synth.random_clip_state(shape, 0)
        for B in (int(v) for v in a.batches.split(",")):
            images = torch.randn(B, 3, shape.image_size, shape.image_size, generator=torch.Generator().manual_seed(0)).cuda()
            vit_images = images if shape.image_size == 224 else torch.randn(B, 3, 224, 224, device="cuda")
            for dtype in a.dtypes.split(","):
                ours = FrozenCLIP(shape, state, tok, max_batch=B, dtype=dtype, rn_fused_conv=False)
                fused = FrozenCLIP(shape, state, tok, max_batch=B, dtype=dtype, rn_fused_conv=True)
                fns = {"ours": lambda: ours.encode_image(images), "fused": lambda: fused.encode_image(images)}
                vit = yard = None
                if not a.ours_only:
                    vit = FrozenCLIP(vit_shape, vit_state, tok, max_batch=B, dtype=dtype)
                    yard = TorchTower(shape, state).cuda().to(TORCH_DTYPE[dtype]).eval()
                    fns.update({"yardstick": lambda: yard(images), "vit_b16": lambda: vit.encode_image(vit_images)})
                with torch.no_grad():
                    got, got1 = ours.encode_image(images).double(), fused.encode_image(images).double()
                    want = yard(images).double() if yard is not None else got
                    rel = ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()
                    rel1 = ((got1 - got).norm(dim=1) / got.norm(dim=1)).max().item()
                    for fn in fns.values():  # warm up (the yardstick's convolution algorithm search included)
                        fn(); fn()
                    ms = {k: [] for k in fns}
                    for _ in range(a.rounds):
                        for k, fn in fns.items():
                            ms[k].append(timed(fn, a.iters))
                line = "; ".join(f"{k} {statistics.median(v):7.2f} ms ({min(v):.2f}-{max(v):.2f})" for k, v in ms.items())
                med = {k: statistics.median(v) for k, v in ms.items()}
                print(f"{name} B={B:3d} {dtype}: {line}; fused / ours {med['fused'] / med['ours']:.3f}; "
                      + (f"ours / yardstick {med['ours'] / med['yardstick']:.2f}; ours vs yardstick features {rel:.1e}; " if yard is not None else "")
                      + f"{B / med['ours'] * 1e3:6.0f} images/s, fused {B / med['fused'] * 1e3:6.0f}; fused vs ours features {rel1:.1e}", flush=True)
                ours.close(); fused.close()
                if vit is not None:
                    vit.close()
                del ours, fused, vit, yard
                torch.cuda.empty_cache()
                if not a.no_split:
                    print_split(f"{name} B={B:3d} {dtype}", *class_split(shape, B, dtype), "gemm")
                    print_split(f"{name} B={B:3d} {dtype} fused", *class_split(shape, B, dtype, fused=True), "conv")


if __name__ == "__main__":
    main()
