"""The device-side input pipeline (mudpt_augment, mudpt_amd/csrc/augment.hip) against what bounds it and what it replaces, in ONE process:

  kernel      one launch for B random-resized crops of seeded uint8 sources of 256 - 500 pixels a side -> [B, 3, 224, 224] fp32 (device events
              around the launch, rows already on the device; median)
  d2d copy    a device-to-device copy of the same output bytes: the ceiling of a kernel that has to write them
  h2d copy    the pageable host -> device copy of the same fp32 batch: what parse_batch_train pays per step without the store
  loader      DeviceImageStore.augment as the loader calls it: rows checked on the host, uploaded, launched (host clock to a synchronise)

at B 256 and B 4.  One JSON line per batch size; exit status 1 if the kernel is not faster than the host copy it replaces.

    python tools/augment_bench.py [--images 512] [--reps 50]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudpt_amd import augment, capi, synth


def events_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def host_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench needs the GPU: a timing taken anywhere else says nothing"
    S = a.size
    store = augment.DeviceImageStore.from_arrays(*synth.synthetic_uint8_images(a.images, 11, seed=0, lo=256, hi=500), device="cuda:0")
    mean_std = (C.c_float * 6)(*augment.CLIP_MEAN, *augment.CLIP_STD)
    stream = torch.cuda.current_stream().cuda_stream
    ok = True
    for B in (256, 4):
        g = torch.Generator().manual_seed(1)
        rows = [augment.rrc_params(store, torch.randint(0, len(store), (B,), generator=g), S, generator=g) for _ in range(4)]  # four batches of crops, rotated
        for p in rows:
            augment.check_params(store.table, p, S)
        forms = {}
        for r in torch.cat(rows).tolist():
            f = augment.augment_form(r[3], r[4], r[7], r[8], S)
            forms[f"{f[0]}/{f[1]}"] = forms.get(f"{f[0]}/{f[1]}", 0) + 1
        rows_dev = [p.cuda() for p in rows]
        outs = [torch.empty(B, 3, S, S, device="cuda:0") for _ in range(3)]  # rotated: 3 x 154 MB at B 256 do not stay in the 256 MB cache
        k = [0]

        def kernel():
            k[0] += 1
            capi.check(capi.call("mudpt_augment", pixels_dev=store.pixels, images_dev=store.table_dev, n_images=len(store), params_dev=rows_dev[k[0] % 4], batch=B,
                                 size=S, mean_std_host=C.addressof(mean_std), out_dev=outs[k[0] % 3], stream=stream), "augment")

        def d2d():
            k[0] += 1
            outs[k[0] % 3].copy_(outs[(k[0] + 1) % 3])

        host = torch.randn(B, 3, S, S)  # pageable, as a DataLoader's collated batch

        def h2d():
            k[0] += 1
            outs[k[0] % 3].copy_(host)

        def loader():
            k[0] += 1
            store.augment(rows[k[0] % 4], S, out=outs[k[0] % 3])

        kern, kern_min = events_ms(kernel, a.reps)
        copy, _ = events_ms(d2d, a.reps)
        h2d_ms, _ = host_ms(h2d, max(a.reps // 5, 5))
        load, _ = host_ms(loader, a.reps)
        nbytes = B * 3 * S * S * 4
        ok = ok and kern < h2d_ms
        print(json.dumps({"batch": B, "size": S, "sources": f"{a.images} images of 256-500 px, {store.nbytes / 2 ** 20:.0f} MiB", "forms": forms,
                          "kernel_ms_median": round(kern, 4), "kernel_ms_min": round(kern_min, 4), "output_MB": round(nbytes / 1e6, 1),
                          "kernel_write_TBps": round(nbytes / kern / 1e9, 3), "d2d_copy_ms": round(copy, 4), "fraction_of_copy_ceiling": round(copy / kern, 3),
                          "pageable_h2d_copy_ms": round(h2d_ms, 3), "kernel_faster_than_h2d_copy": kern < h2d_ms, "loader_call_ms": round(load, 4)}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
