// Device-side input pipeline (INPUT.TRANSFORMS random_resized_crop / random_flip / normalize with INTERPOLATION "bicubic", and the
// evaluation transform Resize + CenterCrop): one launch turns B crop boxes over uint8 HWC images resident in HBM into the [B, 3, S, S] fp32
// batch the model takes.  The resample is Pillow's 8-bit bicubic (ImagingResample: ImagingResampleHorizontal_8bpc then _Vertical_8bpc), restated
// rule by rule in include/mudpt.h at mudpt_augment: weights in fp64 -> 22-bit fixed point, int32 accumulators, a rounding to bytes between
// the two passes.  So the output bytes are Pillow's bytes, and the fp32 values are ToTensor + Normalize's, bit for bit.
//
// This file is compiled with -ffp-contract=off (build.EXTRA_FLAGS): a fused multiply-add in the weight arithmetic would move a weight by
// an ulp, and one time in ~10^4 that moves a fixed-point weight by one and an output byte by one level.
//
// Two forms, the same bytes (augment_plan decides per sample; mudpt_augment_form exports the decision):
//   TABLE   a workgroup owns kBand output rows of one sample.  It builds the x weights of all S columns and the y weights of its rows in
//           LDS once, then takes its rows R at a time (R = 16, 8, 4, 2 or 1, the most whose source rows fit): the horizontal pass of the
//           source rows those R output rows read lands in LDS as bytes (planar per channel), the vertical pass reads them back a dword
//           (four columns) at a time and ends in one 16-byte store per thread.  Sources sit at any byte offset with any width: the
//           horizontal pass reads four taps (twelve bytes) in one unaligned 12-byte load, and byte by byte only where that load would run
//           past the end of the store.
//   DIRECT  for samples whose tables do not fit (tap counts grow with in_len / out_len without bound): a thread per output pixel
//           recomputes every weight where it needs it.  No LDS but the normalisation table, ky * kx weight evaluations per pixel: slow,
//           and only there so that no crop is refused.
// (b / 255 - mean) / std has 3 x 256 possible values: each workgroup computes them once into LDS with IEEE subtract and divide.
#include <algorithm>
#include <climits>
#include <cmath>

#include "kernels.h"

namespace mudpt {

namespace {

constexpr int kBand = 16;          // output rows per workgroup
constexpr int kThreads = 256;
constexpr int kLdsBudget = 40000;  // dynamic LDS per workgroup: four workgroups per CU (160 KiB)
constexpr int kLutBytes = 3 * 256 * 4;
constexpr int kPrecisionBits = 22;

struct Axis {
    double scale, fs, support;
    int in_len, out_off;
};

__host__ __device__ inline Axis make_axis(int in_len, int out_len, int out_off) {
    Axis a;
    a.scale = (double)in_len / (double)out_len;
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * a.fs;
    a.in_len = in_len;
    a.out_off = out_off;
    return a;
}

// Pillow's bicubic_filter (a = -0.5), in its order of operations
__host__ __device__ inline double cubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct Taps {
    double center;
    int lo, n;  // taps [lo, lo + n)
};

__host__ __device__ inline Taps taps_of(const Axis& a, int o) {
    Taps t;
    t.center = ((double)(o + a.out_off) + 0.5) * a.scale;
    int lo = (int)(t.center - a.support + 0.5), hi = (int)(t.center + a.support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > a.in_len) hi = a.in_len;
    t.lo = lo;
    t.n = hi - lo;
    return t;
}

__host__ __device__ inline double raw_weight(const Axis& a, const Taps& t, int i) {  // tap lo + i
    return cubic(((double)(t.lo + i) - t.center + 0.5) / a.fs);
}

__host__ __device__ inline double weight_sum(const Axis& a, const Taps& t) {  // ascending taps
    double s = 0.0;
    for (int i = 0; i < t.n; ++i) s += raw_weight(a, t, i);
    return s;
}

__host__ __device__ inline int fixed_weight(double w) {
    return (int)(w * (double)(1 << kPrecisionBits) + (w < 0.0 ? -0.5 : 0.5));
}

__host__ __device__ inline int clip8(int acc) {
    const int v = acc >> kPrecisionBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct Plan {
    int form, R, kx, ky;  // kx / ky: the table's row length (Pillow's ksize = 2 ceil(support) + 1 >= every tap count)
};

// Which form a sample takes and, for TABLE, how many output rows share one pass over the source rows.  Host and device run this same
// arithmetic (IEEE fp64, no contraction), so the launcher's LDS size and the kernel's carving agree.
__host__ __device__ inline Plan augment_plan(int x_len, int x_out, int y_len, int y_out, int S) {
    Plan p = {MUDPT_AUGMENT_DIRECT, 0, 0, 0};
    const Axis ax = make_axis(x_len, x_out, 0), ay = make_axis(y_len, y_out, 0);
    const double kxd = ceil(ax.support) * 2 + 1, kyd = ceil(ay.support) * 2 + 1;
    if (kxd > 1e6 || kyd > 1e6) return p;
    p.kx = (int)kxd;
    p.ky = (int)kyd;
    const long long Sp = (S + 3) & ~3;
    const long long fixed = kLutBytes + 8LL * S + 4LL * S * p.kx + 8LL * kBand + 4LL * kBand * p.ky;
    for (int R = kBand; R >= 1; R >>= 1) {
        // R consecutive outputs read source rows from the first one's lower bound to the last one's upper bound: their centres lie
        // (R - 1) scale apart and each bound is within support + 0.5 of its centre after truncation
        const long long rows = (long long)((R - 1) * ay.scale + 2.0 * ay.support + 1.0) + 2;
        if (fixed + rows * 3 * Sp <= kLdsBudget) {
            p.form = MUDPT_AUGMENT_TABLE;
            p.R = R;
            return p;
        }
    }
    return p;
}

struct Norm {
    float mean[3], std[3];
};

__device__ inline void build_taps(const Axis& a, int o, int2* meta, int* k) {
    const Taps t = taps_of(a, o);
    const double sum = weight_sum(a, t);
    for (int i = 0; i < t.n; ++i) k[i] = fixed_weight(raw_weight(a, t, i) / sum);
    *meta = make_int2(t.lo, t.n);
}

__global__ __launch_bounds__(kThreads) void augment_kernel(const uint8_t* __restrict__ pixels, const int64_t* __restrict__ images,
                                                           const int32_t* __restrict__ params, int n_images, int S, int bands, Norm nm,
                                                           float* __restrict__ out, int vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / bands, r0 = (blockIdx.x - n * bands) * kBand, nr = min(kBand, S - r0);
    const int32_t* p = params + (size_t)n * 10;
    const int flip = p[1], x_lo = p[2], x_len = p[3], x_out = p[4], x_off = p[5], y_lo = p[6], y_len = p[7], y_out = p[8], y_off = p[9];
    const int64_t* im = images + (size_t)p[0] * 3;
    const int64_t W = im[2];
    const int64_t src_off = im[0] + ((int64_t)y_lo * W + x_lo) * 3;
    const uint8_t* src = pixels + src_off;  // tap (ty, tx), channel c: src[(ty * W + tx) * 3 + c]
    const int64_t* last = images + (size_t)(n_images - 1) * 3;
    const int64_t store_end = last[0] + 3 * last[1] * last[2];  // offsets ascend (mudpt_augment_check): one past the store's last byte
    float* lut = (float*)lds;
    for (int i = tid; i < 768; i += kThreads) {
        const int c = i >> 8;
        const float m = c == 0 ? nm.mean[0] : (c == 1 ? nm.mean[1] : nm.mean[2]), s = c == 0 ? nm.std[0] : (c == 1 ? nm.std[1] : nm.std[2]);
        lut[i] = ((float)(i & 255) / 255.0f - m) / s;
    }
    const Axis ax = make_axis(x_len, x_out, x_off), ay = make_axis(y_len, y_out, y_off);
    const Plan plan = augment_plan(x_len, x_out, y_len, y_out, S);
    float* const out_n = out + (size_t)n * 3 * S * S;

    if (plan.form == MUDPT_AUGMENT_DIRECT) {
        __syncthreads();
        for (int i = tid; i < nr * S; i += kThreads) {
            const int r = i / S, o = i - r * S, oy = r0 + r;
            const Taps tx = taps_of(ax, o), ty = taps_of(ay, oy);
            const double sx = weight_sum(ax, tx), sy = weight_sum(ay, ty);
            int v0 = 1 << (kPrecisionBits - 1), v1 = v0, v2 = v0;
            for (int j = 0; j < ty.n; ++j) {
                const int kyj = fixed_weight(raw_weight(ay, ty, j) / sy);
                const uint8_t* q = src + ((int64_t)(ty.lo + j) * W + tx.lo) * 3;
                int h0 = 1 << (kPrecisionBits - 1), h1 = h0, h2 = h0;
                for (int t = 0; t < tx.n; ++t) {
                    const int k = fixed_weight(raw_weight(ax, tx, t) / sx);
                    h0 += k * q[3 * t];
                    h1 += k * q[3 * t + 1];
                    h2 += k * q[3 * t + 2];
                }
                v0 += kyj * clip8(h0);
                v1 += kyj * clip8(h1);
                v2 += kyj * clip8(h2);
            }
            float* dst = out_n + (size_t)oy * S + (flip ? S - 1 - o : o);
            dst[0] = lut[clip8(v0)];
            dst[(size_t)S * S] = lut[256 + clip8(v1)];
            dst[(size_t)2 * S * S] = lut[512 + clip8(v2)];
        }
        return;
    }

    const int Sp = (S + 3) & ~3, row_bytes = 3 * Sp;
    int2* xmeta = (int2*)(lds + kLutBytes);
    int2* ymeta = xmeta + S;
    int* xk = (int*)(ymeta + kBand);
    int* yk = xk + (size_t)S * plan.kx;
    unsigned char* hbuf = (unsigned char*)(yk + kBand * plan.ky);
    for (int o = tid; o < S; o += kThreads) build_taps(ax, o, xmeta + o, xk + (size_t)o * plan.kx);
    for (int r = tid; r < nr; r += kThreads) build_taps(ay, r0 + r, ymeta + r, yk + r * plan.ky);
    __syncthreads();

    const int G = Sp >> 2;
    for (int rb = 0; rb < nr; rb += plan.R) {
        const int re = min(rb + plan.R, nr);
        const int ya = ymeta[rb].x, rows = ymeta[re - 1].x + ymeta[re - 1].y - ya;  // lower and upper tap bounds both rise with the row
        // horizontal pass of source rows [ya, ya + rows) -> bytes, planar per channel
        for (int i = tid; i < rows * S; i += kThreads) {
            const int row = i / S, o = i - row * S;
            const int2 m = xmeta[o];
            const int* k = xk + (size_t)o * plan.kx;
            const int64_t qoff = src_off + ((int64_t)(ya + row) * W + m.x) * 3;
            const uint8_t* q = pixels + qoff;
            int h0 = 1 << (kPrecisionBits - 1), h1 = h0, h2 = h0;
            const int groups = (m.y + 3) >> 2;
            if (qoff + 12LL * groups <= store_end) {
                // four taps = twelve bytes = three dwords at any alignment (one load each); taps past the last get weight 0, and the bytes
                // read for them lie inside the store (the branch's condition)
                for (int g = 0; g < groups; ++g) {
                    uint32_t w0, w1, w2;
                    __builtin_memcpy(&w0, q + 12 * g, 4);
                    __builtin_memcpy(&w1, q + 12 * g + 4, 4);
                    __builtin_memcpy(&w2, q + 12 * g + 8, 4);
                    const int t = 4 * g;
                    const int k0 = k[t], k1 = t + 1 < m.y ? k[t + 1] : 0, k2 = t + 2 < m.y ? k[t + 2] : 0, k3 = t + 3 < m.y ? k[t + 3] : 0;
                    h0 += k0 * (int)(w0 & 255u) + k1 * (int)(w0 >> 24) + k2 * (int)((w1 >> 16) & 255u) + k3 * (int)((w2 >> 8) & 255u);
                    h1 += k0 * (int)((w0 >> 8) & 255u) + k1 * (int)(w1 & 255u) + k2 * (int)(w1 >> 24) + k3 * (int)((w2 >> 16) & 255u);
                    h2 += k0 * (int)((w0 >> 16) & 255u) + k1 * (int)((w1 >> 8) & 255u) + k2 * (int)(w2 & 255u) + k3 * (int)(w2 >> 24);
                }
            } else {  // the last pixels of the store's last image: byte by byte
                for (int t = 0; t < m.y; ++t) {
                    const int kt = k[t];
                    h0 += kt * q[3 * t];
                    h1 += kt * q[3 * t + 1];
                    h2 += kt * q[3 * t + 2];
                }
            }
            unsigned char* h = hbuf + row * row_bytes + o;
            h[0] = (unsigned char)clip8(h0);
            h[Sp] = (unsigned char)clip8(h1);
            h[2 * Sp] = (unsigned char)clip8(h2);
        }
        __syncthreads();
        // vertical pass: a thread per (row, channel, four columns)
        for (int i = tid; i < (re - rb) * 3 * G; i += kThreads) {
            const int g = i % G, rc = i / G, c = rc % 3, r = rb + rc / 3;
            const int2 m = ymeta[r];
            const int* k = yk + r * plan.ky;
            const unsigned char* h = hbuf + (m.x - ya) * row_bytes + c * Sp + 4 * g;
            int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int t = 0; t < m.y; ++t) {
                const uint32_t w = *(const uint32_t*)(h + t * row_bytes);
                const int kt = k[t];
                a0 += kt * (int)(w & 255u);
                a1 += kt * (int)((w >> 8) & 255u);
                a2 += kt * (int)((w >> 16) & 255u);
                a3 += kt * (int)(w >> 24);
            }
            const float* l = lut + c * 256;
            const float v0 = l[clip8(a0)], v1 = l[clip8(a1)], v2 = l[clip8(a2)], v3 = l[clip8(a3)];
            float* dst = out_n + ((size_t)c * S + (r0 + r)) * S;
            if (vec) {  // S % 4 == 0 and a 16-byte aligned batch: the mirrored group is aligned too
                if (flip) *(f32x4*)(dst + (S - 4 - 4 * g)) = f32x4{v3, v2, v1, v0};
                else *(f32x4*)(dst + 4 * g) = f32x4{v0, v1, v2, v3};
            } else {
                const float v[4] = {v0, v1, v2, v3};
                for (int j = 0; j < 4; ++j) {
                    const int o = 4 * g + j;
                    if (o < S) dst[flip ? S - 1 - o : o] = v[j];
                }
            }
        }
        __syncthreads();  // the next rows' horizontal pass overwrites hbuf
    }
}

}  // namespace

int augment_form(int x_len, int x_out, int y_len, int y_out, int size) {
    if (x_len < 1 || x_out < 1 || y_len < 1 || y_out < 1 || size < 1) return -1;
    const Plan p = augment_plan(x_len, x_out, y_len, y_out, size);
    return p.form | p.R << 8;
}

int launch_augment(const uint8_t* pixels, const int64_t* images, int n_images, const int32_t* params, int batch, int size, const float* mean_std_host,
                   float* out, hipStream_t s) {
    ARG_CHECK(pixels && images && params && mean_std_host && out, "augment: null argument");
    ARG_CHECK(batch >= 0 && size >= 1 && n_images >= 0, "augment: batch %d, size %d, n_images %d: batch and n_images must be >= 0 and size >= 1", batch, size, n_images);
    if (batch == 0) return MUDPT_OK;
    ARG_CHECK(n_images >= 1, "augment: %d rows over a store of %d images", batch, n_images);
    const int bands = (size + kBand - 1) / kBand;
    ARG_CHECK((long long)batch * bands <= INT_MAX, "augment: batch %d x %d row bands exceed the grid", batch, bands);
    ARG_CHECK((long long)batch * 3 * size * size <= (1LL << 40), "augment: batch %d at size %d is too large", batch, size);
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean_std_host[c];
        nm.std[c] = mean_std_host[3 + c];
    }
    const int vec = size % 4 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(augment_kernel, dim3(batch * bands), dim3(kThreads), kLdsBudget, s, pixels, images, params, n_images, size, bands, nm, out, vec);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
