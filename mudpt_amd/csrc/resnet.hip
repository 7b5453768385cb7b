// Data movement of CLIP's ModifiedResNet image tower (clip/model.py:17-161) around the MFMA GEMMs: every convolution and every Linear of the
// attention pool is a launch_gemm; what is here are the memory movers between them.  Activations are NHWC in T (bf16 / fp16), one pixel =
// one row of C channels at a row stride >= C, so a 1 x 1 convolution reads them as its A operand as they lie and a 3 x 3 convolution reads
// the patch rows launch_im2col writes.  Every kernel below moves 16 bytes of T per thread and access (8 channels), stores with plain vector
// stores, uses no atomics and no LDS; a thread's index is checked against the launch's element count, nothing else bounds an access, so the
// launchers refuse every shape whose strides could not hold its rows.
//
// Rounding sites of the tower (tests/resnet_reference.py emulates exactly these; model.cpp resnet_forward sequences them):
//   1. the folded conv + BatchNorm weights are rounded to T once, from fp64 (mudpt_conv_pack); the folded bias stays fp32;
//   2. every GEMM operand activation is T: the pixels (launch_im2col rounds them), every post-ReLU tensor, the pooled tensors
//      (launch_avgpool2d: fp32 sum in window order, one rounding) and the pooled tokens (launch_attnpool_tokens: fp32 mean + fp32
//      positional embedding, one rounding);
//   3. the residual is read in T; acc + bias, + residual and ReLU are fp32, then one rounding (launch_bias_act);
//   4. q / k / v (fp32 GEMM outputs) and the attention are fp32 (launch_attnpool_attend); its output is rounded to T for c_proj;
//   5. the features c_proj writes are fp32.
// The fused convolution (conv.hip, mudpt_resnet_conv_path 1) rounds at these five sites and nowhere else: it reads the same T operands (1, 2),
// accumulates in fp32 on the same matrix instruction, adds bias and residual and applies the ReLU in fp32 in the order of launch_bias_act and
// rounds once (3).  The emulation and every emulated_rel of the fixtures therefore hold for it as they stand.
// Sums are written with __fadd_rn / __fmul_rn: hipcc contracts a * b + c into one fma by default, and the tests hold these kernels to the
// bits of the same fp32 operations done one after the other.
#include "kernels.h"

namespace mudpt {

namespace {

constexpr int kThreads = 256;

// one thread per 16-byte chunk: `chunks` of them, refused beyond what a 1-D grid holds
static int chunk_grid(const char* what, size_t chunks, unsigned* grid) {
    const size_t blocks = (chunks + kThreads - 1) / kThreads;
    ARG_CHECK(blocks >= 1 && blocks <= (size_t)0x7fffffff, "%s: %zu chunks of 16 bytes do not fit one grid", what, chunks);
    *grid = (unsigned)blocks;
    return MUDPT_OK;
}

// patch rows of a 3 x 3, pad 1 convolution from NHWC T: dst[row, (ky * 3 + kx) * C + c] = src[b, oy * stride + ky - 1, ox * stride + kx - 1, c],
// zero outside the image and from column 9 C on.  C % 8 == 0: a chunk of 8 columns lies inside one tap
template <typename T>
__global__ __launch_bounds__(kThreads) void im2col_nhwc_kernel(const typename T::elem* __restrict__ src, typename T::elem* __restrict__ dst, int H, int W, int C,
                                                               int lds, int Ho, int Wo, int stride, int ldk, size_t chunks) {
    using vec8 = typename T::vec8;
    const size_t idx = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (idx >= chunks) return;
    const int cpr = ldk / 8;
    const int k0 = (int)(idx % cpr) * 8;
    const size_t row = idx / cpr;
    const int tap = k0 / C, c = k0 - tap * C;
    vec8 v = {};
    if (tap < 9) {
        const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
        const size_t b = row / ((size_t)Wo * Ho);
        const int iy = oy * stride + tap / 3 - 1, ix = ox * stride + tap % 3 - 1;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const vec8*)(src + ((b * H + iy) * W + ix) * (size_t)lds + c);
    }
    *(vec8*)(dst + row * ldk + k0) = v;
}

// the same from fp32 planar pixels [B, 3, H, W] (the stem's first convolution): column (ky * 3 + kx) * 3 + c, rounded to T
template <typename T>
__global__ __launch_bounds__(kThreads) void im2col_planar_kernel(const float* __restrict__ img, typename T::elem* __restrict__ dst, int H, int W, int Ho, int Wo,
                                                                 int stride, int ldk, size_t chunks) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    const size_t idx = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (idx >= chunks) return;
    const int cpr = ldk / 8;
    const int k0 = (int)(idx % cpr) * 8;
    const size_t row = idx / cpr;
    const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
    const size_t b = row / ((size_t)Wo * Ho);
    vec8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e, tap = k / 3, c = k - tap * 3;
        float f = 0.f;
        if (tap < 9) {
            const int iy = oy * stride + tap / 3 - 1, ix = ox * stride + tap % 3 - 1;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) f = img[((b * 3 + c) * H + iy) * (size_t)W + ix];
        }
        v[e] = (elem)f;
    }
    *(vec8*)(dst + row * ldk + k0) = v;
}

// out = T(act(acc + bias + residual)), the two adds and the ReLU in fp32
template <typename T>
__global__ __launch_bounds__(kThreads) void bias_act_kernel(const float* __restrict__ acc, int ldacc, const float* __restrict__ bias,
                                                            const typename T::elem* __restrict__ res, int ldres, typename T::elem* __restrict__ out, int ldo, int N,
                                                            int relu, size_t chunks) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    const size_t idx = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (idx >= chunks) return;
    const int cpr = N / 8;
    const int n0 = (int)(idx % cpr) * 8;
    const size_t row = idx / cpr;
    const f32x4 a0 = *(const f32x4*)(acc + row * ldacc + n0), a1 = *(const f32x4*)(acc + row * ldacc + n0 + 4);
    float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    if (bias) {
        const f32x4 b0 = *(const f32x4*)(bias + n0), b1 = *(const f32x4*)(bias + n0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = __fadd_rn(v[e], b0[e]); v[4 + e] = __fadd_rn(v[4 + e], b1[e]); }
    }
    if (res) {
        const vec8 r = *(const vec8*)(res + row * ldres + n0);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __fadd_rn(v[e], (float)r[e]);
    }
    vec8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = round_to<elem>(relu && v[e] < 0.f ? 0.f : v[e]);
    *(vec8*)(out + row * ldo + n0) = o;
}

// k x k window, stride k: the fp32 sum in window order (rows, then columns) times 1 / k^2, one rounding
template <typename T>
__global__ __launch_bounds__(kThreads) void avgpool_kernel(const typename T::elem* __restrict__ src, int lds, typename T::elem* __restrict__ dst, int ldo, int H, int W,
                                                           int C, int k, float inv, size_t chunks) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    const size_t idx = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (idx >= chunks) return;
    const int cpr = C / 8, Ho = H / k, Wo = W / k;
    const int c0 = (int)(idx % cpr) * 8;
    const size_t pix = idx / cpr;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const size_t b = pix / ((size_t)Wo * Ho);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const vec8 x = *(const vec8*)(src + ((b * H + oy * k + dy) * W + ox * k + dx) * (size_t)lds + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] = __fadd_rn(s[e], (float)x[e]);
        }
    vec8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = round_to<elem>(__fmul_rn(s[e], inv));
    *(vec8*)(dst + pix * ldo + c0) = o;
}

// AttentionPool2d's token rows (clip/model.py:76-78): row 0 = mean over the HW pixels (fp32 sum in pixel order, times 1 / HW) + pos[0],
// row 1 + l = pixel l + pos[1 + l]; one thread walks the HW pixels of 8 channels of one image
template <typename T>
__global__ __launch_bounds__(kThreads) void attnpool_tokens_kernel(const typename T::elem* __restrict__ src, int lds, const float* __restrict__ pos,
                                                                   typename T::elem* __restrict__ dst, int ldo, int HW, int C, float inv, size_t chunks) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    const size_t idx = blockIdx.x * (size_t)kThreads + threadIdx.x;
    if (idx >= chunks) return;
    const int cpr = C / 8;
    const int c0 = (int)(idx % cpr) * 8;
    const size_t b = idx / cpr;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < HW; ++l) {
        const vec8 x = *(const vec8*)(src + (b * HW + l) * (size_t)lds + c0);
        const float* p = pos + (size_t)(l + 1) * C + c0;
        const f32x4 p0 = *(const f32x4*)p, p1 = *(const f32x4*)(p + 4);
        vec8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xf = (float)x[e];
            s[e] = __fadd_rn(s[e], xf);
            o[e] = round_to<elem>(__fadd_rn(xf, e < 4 ? p0[e] : p1[e - 4]));
        }
        *(vec8*)(dst + (b * (HW + 1) + l + 1) * (size_t)ldo + c0) = o;
    }
    const f32x4 p0 = *(const f32x4*)(pos + c0), p1 = *(const f32x4*)(pos + c0 + 4);
    vec8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = round_to<elem>(__fadd_rn(__fmul_rn(s[e], inv), e < 4 ? p0[e] : p1[e - 4]));
    *(vec8*)(dst + b * (HW + 1) * (size_t)ldo + c0) = o;
}

// The pooled query against its image's L keys (clip/model.py:79-97 with query = x[:1]): one wave per (image, head), lane = one of the 64
// head dimensions, fp32 throughout; q arrives unscaled and is multiplied by 64^-0.5 = 1/8 here, as multi_head_attention_forward does after
// the projection.  The softmax runs online over the keys in order
template <typename T>
__global__ __launch_bounds__(kThreads) void attnpool_attend_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, const float* __restrict__ v, int ldkv,
                                                                   typename T::elem* __restrict__ out, int ldo, int L, int H, int pairs) {
    using elem = typename T::elem;
    const int pair = blockIdx.x * (kThreads / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (pair >= pairs) return;  // a whole wave leaves: the reductions below run with all 64 lanes
    const int b = pair / H, h = pair % H;
    const float qv = q[(size_t)b * ldq + h * 64 + lane] * 0.125f;
    float m = -INFINITY, den = 0.f, acc = 0.f;
    for (int l = 0; l < L; ++l) {
        const size_t at = ((size_t)b * L + l) * ldkv + h * 64 + lane;
        const float s = wave_sum(qv * k[at]);
        const float mn = fmaxf(m, s), scale = expf(m - mn), p = expf(s - mn);
        den = den * scale + p;
        acc = acc * scale + p * v[at];
        m = mn;
    }
    out[(size_t)b * ldo + h * 64 + lane] = round_to<elem>(acc / den);
}

}  // namespace


// kern<BF16> or kern<F16> on `grid` blocks; E names the element type for the casts of the argument list
#define RN_LAUNCH(kern, ...)                                                                                   \
    do {                                                                                                       \
        if (dtype == DT_BF16) { using E = __bf16; hipLaunchKernelGGL(kern<BF16>, dim3(grid), dim3(kThreads), 0, s, __VA_ARGS__); } \
        else { using E = _Float16; hipLaunchKernelGGL(kern<F16>, dim3(grid), dim3(kThreads), 0, s, __VA_ARGS__); }               \
        HIP_TRY(hipGetLastError());                                                                            \
    } while (0)

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool known_dtype(int dtype) { return dtype == DT_BF16 || dtype == DT_F16; }

int launch_im2col(int dtype, const void* src, bool planar, int B, int H, int W, int C, int lds, int stride, void* dst, int ldk, hipStream_t s) {
    ARG_CHECK(known_dtype(dtype), "im2col: unknown dtype %d", dtype);
    ARG_CHECK(src && dst && B > 0 && H > 0 && W > 0 && C > 0, "im2col: null operand or empty shape B=%d H=%d W=%d C=%d", B, H, W, C);
    ARG_CHECK(stride == 1 || stride == 2, "im2col: stride %d (1 or 2)", stride);
    ARG_CHECK(ldk >= 9 * C && ldk % 8 == 0 && aligned16(dst), "im2col: ldk %d must be a multiple of 8 and >= 9 C = %d, dst 16-byte aligned", ldk, 9 * C);
    if (planar) ARG_CHECK(C == 3, "im2col: planar fp32 pixels have 3 channels, not %d", C);
    else ARG_CHECK(C % 8 == 0 && lds >= C && lds % 8 == 0 && aligned16(src), "im2col: an NHWC source needs C %% 8 == 0 (C = %d), a channel stride (%d) >= C that is a multiple of 8, 16-byte alignment", C, lds);
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const size_t chunks = (size_t)B * Ho * Wo * (ldk / 8);
    unsigned grid = 0;
    if (int rc = chunk_grid("im2col", chunks, &grid)) return rc;
    if (planar) RN_LAUNCH(im2col_planar_kernel, (const float*)src, (E*)dst, H, W, Ho, Wo, stride, ldk, chunks);
    else RN_LAUNCH(im2col_nhwc_kernel, (const E*)src, (E*)dst, H, W, C, lds, Ho, Wo, stride, ldk, chunks);
    return MUDPT_OK;
}

int launch_bias_act(int dtype, const float* acc, int ldacc, const float* bias, const void* residual, int ldres, void* out, int ldo, int M, int N, bool relu, hipStream_t s) {
    ARG_CHECK(known_dtype(dtype), "bias_act: unknown dtype %d", dtype);
    ARG_CHECK(acc && out && M > 0 && N > 0 && N % 8 == 0, "bias_act: null operand or bad shape M=%d N=%d (N %% 8 == 0)", M, N);
    ARG_CHECK(ldacc >= N && ldacc % 4 == 0 && ldo >= N && ldo % 8 == 0 && aligned16(acc) && aligned16(out), "bias_act: bad ldacc / ldo %d / %d or alignment", ldacc, ldo);
    ARG_CHECK(!bias || aligned16(bias), "bias_act: bias must be 16-byte aligned");
    ARG_CHECK(!residual || (ldres >= N && ldres % 8 == 0 && aligned16(residual)), "bias_act: bad ldres %d or alignment", ldres);
    const size_t chunks = (size_t)M * (N / 8);
    unsigned grid = 0;
    if (int rc = chunk_grid("bias_act", chunks, &grid)) return rc;
    RN_LAUNCH(bias_act_kernel, acc, ldacc, bias, (const E*)residual, ldres, (E*)out, ldo, N, relu ? 1 : 0, chunks);
    return MUDPT_OK;
}

int launch_avgpool2d(int dtype, const void* src, int lds, void* dst, int ldo, int B, int H, int W, int C, int k, hipStream_t s) {
    ARG_CHECK(known_dtype(dtype), "avgpool2d: unknown dtype %d", dtype);
    ARG_CHECK(src && dst && B > 0 && C > 0 && C % 8 == 0 && k >= 1 && H >= k && W >= k, "avgpool2d: null operand or bad shape B=%d H=%d W=%d C=%d k=%d (C %% 8 == 0)", B, H, W, C, k);
    ARG_CHECK(lds >= C && lds % 8 == 0 && ldo >= C && ldo % 8 == 0 && aligned16(src) && aligned16(dst), "avgpool2d: bad strides %d / %d or alignment", lds, ldo);
    const size_t chunks = (size_t)B * (H / k) * (W / k) * (C / 8);
    unsigned grid = 0;
    if (int rc = chunk_grid("avgpool2d", chunks, &grid)) return rc;
    RN_LAUNCH(avgpool_kernel, (const E*)src, lds, (E*)dst, ldo, H, W, C, k, 1.0f / (float)(k * k), chunks);
    return MUDPT_OK;
}

int launch_attnpool_tokens(int dtype, const void* src, int lds, const float* pos, void* dst, int ldo, int B, int HW, int C, hipStream_t s) {
    ARG_CHECK(known_dtype(dtype), "attnpool_tokens: unknown dtype %d", dtype);
    ARG_CHECK(src && pos && dst && B > 0 && HW > 0 && C > 0 && C % 8 == 0, "attnpool_tokens: null operand or bad shape B=%d HW=%d C=%d (C %% 8 == 0)", B, HW, C);
    ARG_CHECK(lds >= C && lds % 8 == 0 && ldo >= C && ldo % 8 == 0 && aligned16(src) && aligned16(dst) && aligned16(pos), "attnpool_tokens: bad strides %d / %d or alignment", lds, ldo);
    const size_t chunks = (size_t)B * (C / 8);
    unsigned grid = 0;
    if (int rc = chunk_grid("attnpool_tokens", chunks, &grid)) return rc;
    RN_LAUNCH(attnpool_tokens_kernel, (const E*)src, lds, pos, (E*)dst, ldo, HW, C, 1.0f / (float)HW, chunks);
    return MUDPT_OK;
}

int launch_attnpool_attend(int dtype, const float* q, int ldq, const float* k, const float* v, int ldkv, void* out, int ldo, int B, int L, int H, hipStream_t s) {
    ARG_CHECK(known_dtype(dtype), "attnpool_attend: unknown dtype %d", dtype);
    ARG_CHECK(q && k && v && out && B > 0 && L > 0 && H > 0 && (size_t)B * H <= (size_t)0x7fffffff, "attnpool_attend: null operand or bad shape B=%d L=%d H=%d", B, L, H);
    ARG_CHECK(ldq >= H * 64 && ldkv >= H * 64 && ldo >= H * 64, "attnpool_attend: strides %d / %d / %d below H * 64 = %d", ldq, ldkv, ldo, H * 64);
    const int pairs = B * H;
    const unsigned grid = (unsigned)((pairs + kThreads / 64 - 1) / (kThreads / 64));
    RN_LAUNCH(attnpool_attend_kernel, q, ldq, k, v, ldkv, (E*)out, ldo, L, H, pairs);
    return MUDPT_OK;
}

}  // namespace mudpt
