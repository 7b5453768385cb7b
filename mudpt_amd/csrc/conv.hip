// Implicit-GEMM convolution for gfx950: the ResNet tower's 3 x 3 (pad 1, stride 1 | 2) and 1 x 1 convolutions as ONE kernel,
//
//   out[b, oy, ox, n] = T(act(sum_{ky, kx, c} x[b, oy s + ky - p, ox s + kx - p, c] w[n, (ky k + kx) C + c]  + bias[n] + residual[b, oy, ox, n]))
//
// instead of launch_im2col -> launch_gemm(EPI_STORE_F32) -> launch_bias_act (resnet.hip): no patch rows and no fp32 accumulator go through
// memory.  The operands are the ones that path uses: x NHWC in T, w as mudpt_conv_pack writes it, bias fp32.  The rounding sites are the
// ones resnet.hip's header lists: T operands, an fp32 accumulator on the 16-bit MFMA, acc + bias, + residual and ReLU in fp32, one rounding.
//
// Structure: a GEMM  out[M = B Ho Wo, N] = P[M, K = k k C] . w[N, K]^T  whose A operand P (the patch rows) is never written: K is walked in
// steps of 64 columns = 8 chunks of 8 channels; C % 8 == 0, so a chunk lies inside one tap (as in im2col_nhwc_kernel) and is 16 contiguous
// bytes of one source pixel, or zeros when the tap falls outside the image.  A workgroup of 4 waves (2 x 2) owns BM pixels x BN channels.
// Per K-step a thread gathers its chunks (BM / 32 of the pixels, BN / 32 of the weights; its chunk column is fixed, so tap and channel are
// worked out once per step, and the division of a row into (b, oy, ox) once per tile) into registers while the MFMAs of the step before
// run from LDS, then writes them into the other of two LDS buffers: one barrier per K-step.  The LDS image is gemm.hip's: rows of 64 T
// (128 bytes), 16-byte chunk c of row r in slot c ^ (r & 7), so the ds_read_b128 of a fragment (16 rows x 4 chunks) is conflict free.
// The weights are the MFMA's A operand and the pixels its B operand: a lane then holds 4 consecutive channels of one pixel and the epilogue
// loads bias (16 bytes) and residual (8 bytes) and stores 8 bytes along the channels.
//
// What is read: a source chunk only where row < M, the tap lies inside the image and its column is < k k C (so never a channel >= C); a weight
// chunk only where n < N and its column is < k k C.  What is written: out[m, n .. n + 3] for m < M, n < N.  Every index is formed in 64 bits.
// No split of K, no atomics, no workspace; every tile form walks K in the same order with the same instruction, so the bits of a pixel do not
// depend on the form, the batch size or its position in the batch.
#include "kernels.h"

namespace mudpt {

namespace {

template <typename T, int BM, int BN>
__global__ __launch_bounds__(256) void conv2d_kernel(const typename T::elem* __restrict__ x, const typename T::elem* __restrict__ w, const float* __restrict__ bias,
                                                     const typename T::elem* __restrict__ res, typename T::elem* __restrict__ out, int H, int W, int C, int lds, int taps,
                                                     int stride, int Ho, int Wo, int ldk, int ldres, int ldo, int M, int N, int relu) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    using vec4 = typename T::vec4;
    constexpr int ROWB = 128;          // bytes of an LDS row: 64 T
    constexpr int RA = BM / 32;        // pixel rows a thread gathers per K-step
    constexpr int RB = BN / 32;        // weight rows
    constexpr int TM = BM / 2 / 16;    // 16-pixel sub-tiles per wave
    constexpr int TN = BN / 2 / 16;    // 16-channel sub-tiles per wave
    constexpr int STAGE = (BM + BN) * ROWB;
    static_assert(BM % 32 == 0 && BN % 32 == 0, "tile rows split over 32 thread rows");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = (N + BN - 1) / BN;
    const int m0 = (int)(blockIdx.x / ntn) * BM, n0 = (int)(blockIdx.x % ntn) * BN;
    const int K = taps * C, ksize = taps == 9 ? 3 : 1, pad = taps == 9 ? 1 : 0;

    // ---- this thread's gather: chunk column cc of every K-step, rows trow + 32 i of both tiles ----
    const int cc = tid & 7, trow = tid >> 3;
    int iy0[RA], ix0[RA];
    ptrdiff_t pix[RA];  // index of the pixel under tap (0, 0); may lie outside the image, it is only ever used behind the bounds check
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + trow + 32 * i;
        if (m < M) {
            const int ox = m % Wo, t = m / Wo, oy = t % Ho, b = t / Ho;
            iy0[i] = oy * stride - pad;
            ix0[i] = ox * stride - pad;
            pix[i] = ((ptrdiff_t)b * H + iy0[i]) * W + ix0[i];
        } else {
            iy0[i] = -4; ix0[i] = -4; pix[i] = 0;  // no tap of a row past M is inside the image
        }
    }
    ptrdiff_t wrow[RB];
    bool wok[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int n = n0 + trow + 32 * j;
        wok[j] = n < N;
        wrow[j] = (ptrdiff_t)n * ldk;
    }
    // LDS write offsets of those rows (the swizzle is on the slot of the chunk)
    int awr[RA], bwr[RB];
#pragma unroll
    for (int i = 0; i < RA; ++i) { const int r = trow + 32 * i; awr[i] = r * ROWB + ((cc ^ (r & 7)) << 4); }
#pragma unroll
    for (int j = 0; j < RB; ++j) { const int r = trow + 32 * j; bwr[j] = BM * ROWB + r * ROWB + ((cc ^ (r & 7)) << 4); }

    vec8 ga[RA], gb[RB];
    auto gather = [&](int step) {
        const int k0 = step * 64 + cc * 8;
        const bool kin = k0 < K;
        const int tap = k0 / C, c = k0 - tap * C;
        const int ky = tap / ksize, kx = tap - ky * ksize;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int iy = iy0[i] + ky, ix = ix0[i] + kx;
            vec8 v = {};
            if (kin && iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const vec8*)(x + (pix[i] + (ptrdiff_t)ky * W + kx) * lds + c);
            ga[i] = v;
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            vec8 v = {};
            if (kin && wok[j]) v = *(const vec8*)(w + wrow[j] + k0);
            gb[j] = v;
        }
    };
    auto put = [&](int buf) {
        char* base = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < RA; ++i) *(vec8*)(base + awr[i]) = ga[i];
#pragma unroll
        for (int j = 0; j < RB; ++j) *(vec8*)(base + bwr[j]) = gb[j];
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment reads: row = sub-tile base + (lane & 15), chunk = 4 ks + (lane >> 4); sub-tile bases are multiples of 16, so row & 7 = frow & 7
    const int frow = lane & 15, fq = lane >> 4, sw = frow & 7;
    int aoff[TM], boff[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aoff[i] = (wm * (BM / 2) + i * 16 + frow) * ROWB;
#pragma unroll
    for (int j = 0; j < TN; ++j) boff[j] = BM * ROWB + (wn * (BN / 2) + j * 16 + frow) * ROWB;

    const int nsteps = (K + 63) / 64;
    gather(0);
    put(0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) gather(step + 1);  // in flight under the MFMAs below
        const char* base = smem + (step & 1) * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int c = ((ks * 4 + fq) ^ sw) << 4;
            vec8 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *(const vec8*)(base + aoff[i] + c);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *(const vec8*)(base + boff[j] + c);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = T::mfma16(bf[j], af[i], acc[i][j]);
        }
        // the other buffer was last read in step - 1, which every wave left before the barrier that ended it
        if (more) put((step + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: lane holds out[m][n .. n + 3], m = sub-tile pixel (lane & 15), n = 4 (lane >> 4) ----
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm * (BM / 2) + i * 16 + frow;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * (BN / 2) + j * 16 + fq * 4;
            if (n >= N) continue;  // N % 16 == 0: a sub-tile is all in or all out
            f32x4 v = acc[i][j];
            if (bias) {
                const f32x4 b4 = *(const f32x4*)(bias + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], b4[e]);
            }
            if (res) {
                const vec4 r4 = *(const vec4*)(res + (size_t)m * ldres + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], (float)r4[e]);
            }
            vec4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = round_to<elem>(relu && v[e] < 0.f ? 0.f : v[e]);
            *(vec4*)(out + (size_t)m * ldo + n) = o;
        }
    }
}

template <typename T, int BM, int BN>
static int launch_tile(const void* x, const void* w, const float* bias, const void* res, void* out, int H, int W, int C, int lds, int taps, int stride, int Ho, int Wo,
                       int ldk, int ldres, int ldo, int M, int N, int relu, hipStream_t s) {
    using E = typename T::elem;
    constexpr int bytes = 2 * (BM + BN) * 128;
    constexpr auto kern = conv2d_kernel<T, BM, BN>;
    if (int e = lds_limit_once<kern>(current_device(), bytes)) return e;
    const size_t tiles = (size_t)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    ARG_CHECK(tiles <= (size_t)0x7fffffff, "conv2d: %zu tiles do not fit one grid", tiles);
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), bytes, s, (const E*)x, (const E*)w, bias, (const E*)res, (E*)out, H, W, C, lds, taps, stride, Ho, Wo, ldk, ldres,
                       ldo, M, N, relu);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

template <typename T>
static int launch_form(int form, const void* x, const void* w, const float* bias, const void* res, void* out, int H, int W, int C, int lds, int taps, int stride, int Ho,
                       int Wo, int ldk, int ldres, int ldo, int M, int N, int relu, hipStream_t s) {
    switch (form) {
        case MUDPT_CONV_T128x128: return launch_tile<T, 128, 128>(x, w, bias, res, out, H, W, C, lds, taps, stride, Ho, Wo, ldk, ldres, ldo, M, N, relu, s);
        case MUDPT_CONV_T128x64: return launch_tile<T, 128, 64>(x, w, bias, res, out, H, W, C, lds, taps, stride, Ho, Wo, ldk, ldres, ldo, M, N, relu, s);
        case MUDPT_CONV_T64x64: return launch_tile<T, 64, 64>(x, w, bias, res, out, H, W, C, lds, taps, stride, Ho, Wo, ldk, ldres, ldo, M, N, relu, s);
    }
    set_error("conv2d: unknown tile form %d", form);
    return MUDPT_ERR_ARG;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// Which tile runs M pixels x N channels (host arithmetic; exported as mudpt_conv2d_form).  The widest tile whose grid still gives each of
// the MI355X's 256 compute units a workgroup: 128 x 128 halves the operand traffic per output of 128 x 64, which halves that of 64 x 64, but
// a grid smaller than the chip is a set of latency chains over K, and more, smaller tiles shorten the wall time then.  N <= 64 (the stem and
// stage 1 of the tower) never takes the 128-wide tile: half of it would be empty.  The constant is the chip's, not the device's, so that a
// shape's form is the same everywhere; the bits do not depend on the form either way.
int conv2d_form(int M, int N) {
    if (M < 1 || N < 1) return -1;
    constexpr size_t kCus = 256;
    const size_t r128 = ((size_t)M + 127) / 128;
    if (N > 64 && r128 * (((size_t)N + 127) / 128) >= kCus) return MUDPT_CONV_T128x128;
    if (r128 * (((size_t)N + 63) / 64) >= kCus) return MUDPT_CONV_T128x64;
    return MUDPT_CONV_T64x64;
}

int launch_conv2d(int dtype, const void* src, int B, int H, int W, int C, int lds, int k, int stride, const void* w, int ldk, const float* bias, const void* residual,
                  int ldres, void* out, int ldo, int N, bool relu, hipStream_t s) {
    ARG_CHECK(dtype == DT_BF16 || dtype == DT_F16, "conv2d: unknown dtype %d", dtype);
    ARG_CHECK(src && w && out, "conv2d: null src, w or out");
    ARG_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1 && N >= 1, "conv2d: empty shape B=%d H=%d W=%d C=%d N=%d", B, H, W, C, N);
    ARG_CHECK(k == 1 || k == 3, "conv2d: k %d (1 or 3)", k);
    ARG_CHECK(stride == 1 || (k == 3 && stride == 2), "conv2d: stride %d (1, or 2 with k = 3)", stride);
    ARG_CHECK(C % 8 == 0, "conv2d: C %d must be a multiple of 8", C);
    ARG_CHECK(lds >= C && lds % 8 == 0, "conv2d: lds %d must be a multiple of 8 and >= C = %d", lds, C);
    ARG_CHECK((int64_t)k * k * C <= 0x7fffffff && ldk >= k * k * C && ldk % 8 == 0, "conv2d: ldk %d must be a multiple of 8 and >= k k C = %lld", ldk, (long long)k * k * C);
    ARG_CHECK(N % 16 == 0, "conv2d: N %d must be a multiple of 16", N);
    ARG_CHECK(ldo >= N && ldo % 4 == 0, "conv2d: ldo %d must be a multiple of 4 and >= N = %d", ldo, N);
    ARG_CHECK(!residual || (ldres >= N && ldres % 4 == 0), "conv2d: ldres %d must be a multiple of 4 and >= N = %d", ldres, N);
    ARG_CHECK(aligned16(src) && aligned16(w) && aligned16(out) && (!bias || aligned16(bias)) && (!residual || aligned16(residual)),
              "conv2d: src, w, bias, residual and out must be 16-byte aligned");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int64_t M = (int64_t)B * Ho * Wo;
    ARG_CHECK(M <= 0x7fffffff - 128 && (int64_t)B * H * W <= 0x7fffffff, "conv2d: B H W = %d x %d x %d pixels do not fit 31 bits", B, H, W);
    const int form = conv2d_form((int)M, N);
    if (dtype == DT_BF16) return launch_form<BF16>(form, src, w, bias, residual, out, H, W, C, lds, k * k, stride, Ho, Wo, ldk, ldres, ldo, (int)M, N, relu ? 1 : 0, s);
    return launch_form<F16>(form, src, w, bias, residual, out, H, W, C, lds, k * k, stride, Ho, Wo, ldk, ldres, ldo, (int)M, N, relu ? 1 : 0, s);
}

}  // namespace mudpt
