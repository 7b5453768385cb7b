// Fused cosine-logit / cross-entropy head for gfx950 (trainers/mudpt.py:178-182 and F.cross_entropy at :250).
//
//   logits[B, C] = exp(logit_scale) * normalise(img)[B, e] . normalise(txt)[C, e]^T,  loss = mean_b CE(logits[b], label[b])
//
// The contraction runs on the matrix cores in EXACT fp32 (v_mfma_f32_16x16x4_f32: a k-ordered fp32 fma chain, bit for bit; the
// logits feed a 1e-3 parity bound at logit scale 14-100, so bf16 / fp16 operands are not an option here), and the row softmax /
// cross-entropy / dlogits never leave the workgroup that made the logit rows:
//   head_rows_kernel  (one workgroup per 16 images): normalise the 16 image rows -> LDS; logit tile [16, C] by MFMA -> LDS + HBM;
//       [training] per-row log-sum-exp, loss row, dlogits = (softmax - onehot) * gscale in place; d(normalised image features) =
//       scale * dlogits . txt_n by MFMA; backward of the normalisation -> dimg.  [training, HeadArgs::dimg null: a frozen image tower
//       with nothing trainable in front of it] the kernel ends behind dlogits: no gradient tile in LDS, no second contraction.
//   head_dtxt_kernel  (one workgroup per 16 classes, training): d(normalised text features) = scale * dlogits^T . img_n by MFMA
//       (images in ascending order: a fixed summation order), backward of the normalisation -> dtxt.
// plus the existing row-normalisation of the C text features and the fixed-order mean of the loss rows: 4 launches instead of 9.
// MFMA operand maps (16x16x4 f32): lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; D: column l & 15, rows 4 (l >> 4) + r.
// Four consecutive k are fetched as one float4 per operand and fed to four MFMAs; any partition of k works as long as A and B agree.
#include "kernels.h"

namespace mudpt {

constexpr int HEAD_MAX_E_TRAIN = 65536 / (16 * 4);  // head_dtxt_kernel: [16][e] fp32 within the 64 KB it asks for
constexpr int HEAD_ROWS = 16, HEAD_WAVES = 8, HEAD_RPW = HEAD_ROWS / HEAD_WAVES;  // 16 rows per workgroup, 8 waves, 2 rows per wave in the row-wise phases

// acc[t] += A[16, K] . B[K, 16 tile t]: A from `a_row` (this lane's row, k contiguous: LDS or global), B rows from `b_base + k * ldb`
// (k-major operand: element (k, col) at b[k * ldb + col]); K a multiple of 16; rows of B beyond k_valid read as zero.
// GUARD_A (A straight from memory, not from a padded LDS tile): A is read only where a_ok and k < k_valid, zero elsewhere.
template <int NT, bool GUARD_A = false>
__device__ inline void mfma_kmajor(f32x4 (&acc)[NT], const float* a_row, int a_stride_k, const float* b_base, size_t ldb, const int (&col)[NT],
                                   const bool (&col_ok)[NT], int K, int k_valid, int g, bool a_ok = true) {
    // 4 steps' operands are requested before the first MFMA (the loop is otherwise one dependent memory round trip per step); K % 16 == 0
    for (int k0 = 0; k0 < K; k0 += 16) {
        float av[4], bv[4][NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + g;
            if constexpr (GUARD_A) av[u] = (a_ok && k < k_valid) ? a_row[(size_t)k * a_stride_k] : 0.f;
            else av[u] = a_row[(size_t)k * a_stride_k];
#pragma unroll
            for (int t = 0; t < NT; ++t) bv[u][t] = (col_ok[t] && k < k_valid) ? b_base[(size_t)k * ldb + col[t]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][t], acc[t], 0, 0, 0);
    }
}

// y = inv * (d - n * <d, n>) for 4 rows per wave: backward of n = x / ||x||; d and n are LDS / global rows of length e
__device__ inline void l2norm_bwd_row(const float* d, const float* n, float inv, float* out, int e, int lane) {
    float s = 0.f;
    for (int k = lane; k < e; k += 64) s += d[k] * n[k];
    s = wave_sum(s);
    for (int k = lane; k < e; k += 64) out[k] = inv * (d[k] - n[k] * s);
}
// l2norm_bwd_row + gmul * extra in the one store; extra null: l2norm_bwd_row itself.  out may be d (every lane reads its d[k] before it writes out[k],
// and the sum is complete before the first store)
__device__ inline void l2norm_bwd_row_add(const float* d, const float* n, float inv, float* out, const float* extra, float gmul, int e, int lane) {
    if (!extra) { l2norm_bwd_row(d, n, inv, out, e, lane); return; }
    float s = 0.f;
    for (int k = lane; k < e; k += 64) s += d[k] * n[k];
    s = wave_sum(s);
    for (int k = lane; k < e; k += 64) out[k] = inv * (d[k] - n[k] * s) + gmul * extra[k];
}

// DIMG = false (training only): the image features need no gradient -- steps 4 and 5 and their [16][e] tile are left out, steps 1 to 3 are
// the same instructions in the same order, so everything they write is bit-identical to the form with dimg
template <bool TRAIN, bool DIMG = TRAIN>
__global__ __launch_bounds__(HEAD_WAVES * 64) void head_rows_kernel(HeadArgs p, int Cpad) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    float* In = hsm;                          // [16][e] normalised image rows
    float* Zt = In + HEAD_ROWS * p.e;         // [16][Cpad] logits, then dlogits
    float* Dn = Zt + HEAD_ROWS * Cpad;        // [16][e] d(normalised image features)   (DIMG only)
    __shared__ float inv_s[HEAD_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * HEAD_ROWS, e = p.e, C = p.C, B = p.B;

    // ---- 1. normalise the image rows (HEAD_RPW per wave) ----------------------------------------------------------------------------
    for (int i = 0; i < HEAD_RPW; ++i) {
        const int rl = wave * HEAD_RPW + i, r = r0 + rl;
        float s = 0.f;
        if (r < B)
            for (int k = lane; k < e; k += 64) { const float v = p.img[(size_t)r * e + k]; s += v * v; }
        const float iv = r < B ? 1.0f / sqrtf(wave_sum(s)) : 0.f;
        for (int k = lane; k < e; k += 64) {
            const float v = r < B ? p.img[(size_t)r * e + k] * iv : 0.f;
            In[rl * e + k] = v;
            if (r < B && p.img_n) p.img_n[(size_t)r * e + k] = v;
        }
        if (lane == 0) {
            inv_s[rl] = iv;
            if (r < B && p.img_inv) p.img_inv[r] = iv;
        }
    }
    __syncthreads();

    // ---- 2. logits: class tiles of 16 over the waves; k = e in float4 pieces (four MFMAs each) ----------------------------------
    for (int ct = wave; ct < Cpad / 16; ct += HEAD_WAVES) {
        const int cls = ct * 16 + c;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* ar = In + c * e + 4 * g;
        const float* br = p.txt_n + (size_t)(cls < C ? cls : 0) * e + 4 * g;
        for (int j0 = 0; j0 < e; j0 += 128) {  // 8 float4 pairs requested before the first MFMA: the loads overlap instead of chaining
            f32x4 a4[8], b4[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + 16 * u;
                const bool in = j < e;
                a4[u] = in ? *(const f32x4*)(ar + j) : f32x4{0.f, 0.f, 0.f, 0.f};
                b4[u] = (in && cls < C) ? *(const f32x4*)(br + j) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u][t], b4[u][t], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = 4 * g + r;
            const float z = p.scale * acc[r];
            Zt[rl * Cpad + cls] = z;
            if (r0 + rl < B && cls < C) p.logits[(size_t)(r0 + rl) * C + cls] = z;
        }
    }
    if constexpr (!TRAIN) return;
    __syncthreads();

    // ---- 3. cross-entropy rows; dlogits = (softmax - onehot) * gscale, in place ---------------------------------------------------
    const float gscale = p.grad_scale / (p.B_total > 0 ? p.B_total : B);
    for (int i = 0; i < HEAD_RPW; ++i) {
        const int rl = wave * HEAD_RPW + i, r = r0 + rl;
        float* z = Zt + rl * Cpad;
        if (r >= B) {  // padding rows contribute nothing to the gradients
            for (int k = lane; k < Cpad; k += 64) z[k] = 0.f;
            continue;
        }
        float m = -INFINITY;
        for (int k = lane; k < C; k += 64) m = fmaxf(m, z[k]);
        m = wave_max(m);
        float s = 0.f;
        for (int k = lane; k < C; k += 64) s += __expf(z[k] - m);
        s = wave_sum(s);
        // a label outside [0, C) (torch's F.cross_entropy asserts on it): NaN loss row, no one-hot, never an out-of-bounds access
        const int64_t y64 = p.labels[r];
        const bool y_ok = y64 >= 0 && y64 < (int64_t)C;
        const int y = y_ok ? (int)y64 : -1;
        if (lane == 0) p.row_loss[r] = y_ok ? (m + __logf(s)) - z[y] : __builtin_nanf("");
        const float is = 1.f / s;
        for (int k = lane; k < Cpad; k += 64) {
            const float d = k < C ? (__expf(z[k] - m) * is - (k == y ? 1.f : 0.f)) * gscale : 0.f;
            z[k] = d;
            if (k < C && p.dlogits) p.dlogits[(size_t)r * C + k] = d;
        }
    }
    if constexpr (!DIMG) return;
    __syncthreads();

    // ---- 4. d(normalised image features)[16, e] = scale * dlogits[16, C] . txt_n[C, e]: e tiles over the waves, 4 at a time -------
    {
        const int ne = e / 16;
        for (int et0 = wave * 4; et0 < ne; et0 += 4 * HEAD_WAVES) {
            f32x4 acc[4];
            int col[4];
            bool ok[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; col[t] = (et0 + t) * 16 + c; ok[t] = et0 + t < ne; }
            mfma_kmajor<4>(acc, Zt + c * Cpad, 1, p.txt_n, (size_t)e, col, ok, Cpad, C, g);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (ok[t])
#pragma unroll
                    for (int r = 0; r < 4; ++r) Dn[(4 * g + r) * e + col[t]] = p.scale * acc[t][r];
        }
    }
    __syncthreads();
    // ---- 5. backward of the normalisation -> gradient of the raw image features ------------------------------------------------
    for (int i = 0; i < HEAD_RPW; ++i) {
        const int rl = wave * HEAD_RPW + i, r = r0 + rl;
        if (r < B) l2norm_bwd_row(Dn + rl * e, In + rl * e, inv_s[rl], p.dimg + (size_t)r * e, e, lane);
    }
}

// d(raw text features) of 16 classes: scale * G^T[16, B] . img_n[B, e], then the backward of the normalisation, + gmul * Etxt.
// p.scale is the product the launcher folded (head scale * gmul).  The training head passes G = dlogits, ldg = C, gmul = 1, Etxt = null.
__global__ __launch_bounds__(HEAD_WAVES * 64) void head_dtxt_kernel(HeadGradArgs p) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    float* Dn = hsm;  // [16][e]
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = blockIdx.x * HEAD_ROWS, e = p.e, C = p.C, B = p.B;
    const int Bpad = (B + 3) & ~3, ne = e / 16;
    const int cls = c0 + c;
    const size_t ldg = (size_t)p.ldg;
    // A[class c][k = image] = G[image][class]: this lane's "row" is a column of G, stride ldg between consecutive k
    const float* a_row = p.G + (cls < C ? cls : 0);
    for (int et0 = wave * 4; et0 < ne; et0 += 4 * HEAD_WAVES) {
        f32x4 acc[4];
        int col[4];
        bool ok[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; col[t] = (et0 + t) * 16 + c; ok[t] = et0 + t < ne; }
        // the sum over the images is a latency chain (one dependent global round trip per step of 4 images): 8 steps' operands are
        // requested before the first MFMA so the loads overlap; the MFMA order (images ascending) is unchanged
        for (int k0 = 0; k0 < Bpad; k0 += 32) {
            float av[8], bv[8][4];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + 4 * u + g;
                av[u] = (k < B && cls < C) ? a_row[(size_t)k * ldg] : 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) bv[u][t] = (ok[t] && k < B) ? p.img_n[(size_t)k * e + col[t]] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][t], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (ok[t])
#pragma unroll
                for (int r = 0; r < 4; ++r) Dn[(4 * g + r) * e + col[t]] = p.scale * acc[t][r];
    }
    __syncthreads();
    for (int i = 0; i < HEAD_RPW; ++i) {
        const int rl = wave * HEAD_RPW + i, r = c0 + rl;
        if (r >= C) continue;
        l2norm_bwd_row_add(Dn + rl * e, p.txt_n + (size_t)r * e, p.txt_inv[r], p.dtxt + (size_t)r * e, p.Etxt ? p.Etxt + (size_t)r * e : nullptr, p.gmul, e, lane);
    }
}

// d(raw image features) of 16 images: scale * G[16, C] . txt_n[C, e] (G's rows are the A operand straight from memory, classes ascending: a
// fixed summation order, and a row's result does not depend on the rows beside it), then steps 5 of head_rows_kernel<true> on img_n / img_inv
// from memory, + gmul * Eimg.  A row >= B or a class >= C is never read (the padding columns of ldg > C may hold anything).
__global__ __launch_bounds__(HEAD_WAVES * 64) void head_dimg_kernel(HeadGradArgs p) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    float* Dn = hsm;  // [16][e]
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * HEAD_ROWS, e = p.e, C = p.C, B = p.B;
    const int Cpad = (C + 15) / 16 * 16, ne = e / 16;
    const bool row_ok = r0 + c < B;
    const float* a_row = p.G + (size_t)(row_ok ? r0 + c : 0) * (size_t)p.ldg;
    for (int et0 = wave * 4; et0 < ne; et0 += 4 * HEAD_WAVES) {
        f32x4 acc[4];
        int col[4];
        bool ok[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; col[t] = (et0 + t) * 16 + c; ok[t] = et0 + t < ne; }
        mfma_kmajor<4, true>(acc, a_row, 1, p.txt_n, (size_t)e, col, ok, Cpad, C, g, row_ok);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (ok[t])
#pragma unroll
                for (int r = 0; r < 4; ++r) Dn[(4 * g + r) * e + col[t]] = p.scale * acc[t][r];
    }
    __syncthreads();
    for (int i = 0; i < HEAD_RPW; ++i) {
        const int rl = wave * HEAD_RPW + i, r = r0 + rl;
        if (r >= B) continue;
        l2norm_bwd_row_add(Dn + rl * e, p.img_n + (size_t)r * e, p.img_inv[r], p.dimg + (size_t)r * e, p.Eimg ? p.Eimg + (size_t)r * e : nullptr, p.gmul, e, lane);
    }
}

// unfused form, behind launch_sgemm: the same row step in place on d, one wave per row
__global__ __launch_bounds__(256) void head_grad_rows_kernel(float* d, const float* n, const float* inv, const float* extra, float gmul, int rows, int e) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (size_t)rows) return;
    float* dr = d + r * e;
    l2norm_bwd_row_add(dr, n + r * e, inv[r], dr, extra ? extra + r * e : nullptr, gmul, e, lane);
}
// y = gmul * x: the gradient of a loss that reads the features only (no logit gradient, no contraction)
__global__ __launch_bounds__(256) void head_grad_scale_kernel(const float* x, float gmul, float* y, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = gmul * x[i];
}

static int head_lds_bytes(const HeadArgs& a, bool train) {
    const int Cpad = (a.C + 15) / 16 * 16;
    return (HEAD_ROWS * a.e * (train && a.dimg ? 2 : 1) + HEAD_ROWS * Cpad) * 4;  // the gradient tile: only where dimg is asked for
}
// true if the fused kernels can hold a 16-row problem in LDS (otherwise the caller keeps the unfused fp32 path of elementwise.hip)
// Training: head_dtxt_kernel keeps a [16][e] fp32 tile in its 64 KB LDS allowance, so e <= 1024 there (launch_head_fused_train refuses more).
// Training without dimg needs the forward's LDS: e = 1024 fits up to Cpad 1520 (with dimg: 496), e = 512 up to 2032 (1520).
bool head_fused_fits(const HeadArgs& a, bool train) {
    return a.e > 0 && a.e % 16 == 0 && (!train || a.e <= HEAD_MAX_E_TRAIN) && head_lds_bytes(a, train) + 256 <= 163840;
}

// logits (and the normalised features the backward needs).  txt_n / txt_inv are (re)computed unless a.txt is null (cached text features).
int launch_head_fused_fwd(const HeadArgs& a, hipStream_t s) {
    ARG_CHECK(a.img && a.logits && a.txt_n && a.txt_inv && a.B > 0 && a.C > 0 && a.e > 0, "head: bad arguments");
    ARG_CHECK(head_fused_fits(a, false), "head: the fused forward does not take B=%d C=%d e=%d (e %% 16, LDS)", a.B, a.C, a.e);
    if (a.txt)
        if (int rc = launch_l2norm(a.txt, a.txt_n, a.txt_inv, a.C, a.e, s)) return rc;
    const int Cpad = (a.C + 15) / 16 * 16, lds = head_lds_bytes(a, false);
    if (int e = lds_limit_once<head_rows_kernel<false>>(current_device(), 163840 - 256)) return e;
    hipLaunchKernelGGL(head_rows_kernel<false>, dim3((a.B + HEAD_ROWS - 1) / HEAD_ROWS), dim3(HEAD_WAVES * 64), lds, s, a, Cpad);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

// forward + mean cross-entropy + backward to the RAW features in one pass over the logit rows (logits are written too)
int launch_head_fused_train(const HeadArgs& a, hipStream_t s) {
    ARG_CHECK(a.img && a.logits && a.txt_n && a.txt_inv && a.img_n && a.img_inv && a.labels && a.loss && a.dlogits && a.row_loss,
              "head: null operand");  // dimg may be null: no image gradient
    ARG_CHECK(a.B > 0 && a.C > 0 && a.e > 0 && a.e <= HEAD_MAX_E_TRAIN, "head: bad shape B=%d C=%d e=%d", a.B, a.C, a.e);
    ARG_CHECK(a.B_total <= 0 || a.B_total >= a.B, "head: B_total=%d is smaller than its chunk of B=%d rows", a.B_total, a.B);
    ARG_CHECK(head_fused_fits(a, true), "head: the fused training head does not take B=%d C=%d e=%d (e %% 16, LDS)", a.B, a.C, a.e);
    if (a.txt)
        if (int rc = launch_l2norm(a.txt, a.txt_n, a.txt_inv, a.C, a.e, s)) return rc;
    const int Cpad = (a.C + 15) / 16 * 16, lds = head_lds_bytes(a, true);
    const int dev = current_device();
    if (int e = a.dimg ? lds_limit_once<head_rows_kernel<true>>(dev, 163840 - 256) : lds_limit_once<head_rows_kernel<true, false>>(dev, 163840 - 256)) return e;
    if (int e = lds_limit_once<head_dtxt_kernel>(dev, 65536)) return e;
    const dim3 grid((a.B + HEAD_ROWS - 1) / HEAD_ROWS), block(HEAD_WAVES * 64);
    if (a.dimg) hipLaunchKernelGGL(head_rows_kernel<true>, grid, block, lds, s, a, Cpad);
    else hipLaunchKernelGGL((head_rows_kernel<true, false>), grid, block, lds, s, a, Cpad);
    HIP_TRY(hipGetLastError());
    if (a.B_total <= 0)
        if (int rc = launch_mean(a.row_loss, a.B, a.loss, s)) return rc;
    if (!a.dtxt) return MUDPT_OK;  // the text features have nothing to learn (VPT): no text half
    HeadGradArgs t; t.img_n = a.img_n; t.txt_n = a.txt_n; t.txt_inv = a.txt_inv; t.G = a.dlogits; t.ldg = a.C; t.dtxt = a.dtxt; t.scale = a.scale;
    t.B = a.B; t.C = a.C; t.e = a.e;
    hipLaunchKernelGGL(head_dtxt_kernel, dim3((a.C + HEAD_ROWS - 1) / HEAD_ROWS), dim3(HEAD_WAVES * 64), HEAD_ROWS * a.e * 4, s, t);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

bool head_grad_fused_fits(const HeadGradArgs& a) { return a.e > 0 && a.e % 16 == 0 && a.e <= HEAD_MAX_E_TRAIN; }
// head_dimg_kernel has one workgroup per 16 images and each walks ALL classes, 16 per step of a dependent load chain (head_dtxt_kernel: the
// same over the images); the unfused form spreads each contraction over an sgemm grid.  Measured (tools/custom_loss_bench.py):
// the fused pair is the faster one only while each kernel is ONE workgroup (13.7 against 16.6 us at B 4, 11 classes); from 50 classes or 32
// images on it loses, 2.3 x at 256 x 1000, e 512 and 4.4 x at 32 x 1000, e 1024.  The dispatch follows that
constexpr int HEAD_GRAD_FUSED_MAX_ROWS = HEAD_ROWS;
bool head_grad_fused(const HeadGradArgs& a) { return head_grad_fused_fits(a) && a.B <= HEAD_GRAD_FUSED_MAX_ROWS && a.C <= HEAD_GRAD_FUSED_MAX_ROWS; }

// one output of a feature-only loss: gmul * E, or zeros where that output has no gradient input at all
static int head_grad_scaled(const float* E, float gmul, float* out, size_t n, hipStream_t s) {
    if (!E) { HIP_TRY(hipMemsetAsync(out, 0, n * 4, s)); return MUDPT_OK; }
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(head_grad_scale_kernel, dim3(grid), dim3(256), 0, s, E, gmul, out, n);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

int launch_head_grad(const HeadGradArgs& a, hipStream_t s, int form) {
    ARG_CHECK(form >= 0 && form <= 2, "head_grad: form %d is none of 0 (dispatch), 1 (unfused), 2 (fused)", form);
    ARG_CHECK(form != 2 || head_grad_fused_fits(a), "head_grad: the fused form does not take e=%d (e %% 16 == 0, e <= %d)", a.e, HEAD_MAX_E_TRAIN);
    ARG_CHECK(a.img_n, "head_grad: img_n is null");
    ARG_CHECK(a.img_inv, "head_grad: img_inv is null");
    ARG_CHECK(a.txt_n, "head_grad: txt_n is null");
    ARG_CHECK(a.txt_inv, "head_grad: txt_inv is null");
    ARG_CHECK(a.B >= 1, "head_grad: B=%d must be at least 1", a.B);
    ARG_CHECK(a.C >= 1, "head_grad: C=%d must be at least 1", a.C);
    ARG_CHECK(a.e >= 1, "head_grad: e=%d must be at least 1", a.e);
    ARG_CHECK(!a.G || a.ldg >= a.C, "head_grad: ldg=%lld is smaller than C=%d", (long long)a.ldg, a.C);
    ARG_CHECK(a.dimg || a.dtxt, "head_grad: dimg and dtxt are both null: nothing to compute");
    ARG_CHECK(a.G || a.Eimg || a.Etxt, "head_grad: G, Eimg and Etxt are all null: no gradient to start from");
    const size_t ne_img = (size_t)a.B * a.e, ne_txt = (size_t)a.C * a.e;
    if (!a.G) {
        if (a.dimg) if (int rc = head_grad_scaled(a.Eimg, a.gmul, a.dimg, ne_img, s)) return rc;
        if (a.dtxt) if (int rc = head_grad_scaled(a.Etxt, a.gmul, a.dtxt, ne_txt, s)) return rc;
        return MUDPT_OK;
    }
    HeadGradArgs p = a;
    p.scale = a.scale * a.gmul;  // l2norm_bwd is linear: gmul goes through the contraction's scale
    if (form == 2 || (form == 0 && head_grad_fused(a))) {
        const int dev = current_device(), lds = HEAD_ROWS * a.e * 4;
        if (a.dimg) {
            if (int e = lds_limit_once<head_dimg_kernel>(dev, 65536)) return e;
            hipLaunchKernelGGL(head_dimg_kernel, dim3((a.B + HEAD_ROWS - 1) / HEAD_ROWS), dim3(HEAD_WAVES * 64), lds, s, p);
        }
        if (a.dtxt) {
            if (int e = lds_limit_once<head_dtxt_kernel>(dev, 65536)) return e;
            hipLaunchKernelGGL(head_dtxt_kernel, dim3((a.C + HEAD_ROWS - 1) / HEAD_ROWS), dim3(HEAD_WAVES * 64), lds, s, p);
        }
        HIP_TRY(hipGetLastError());
        return MUDPT_OK;
    }
    ARG_CHECK(a.ldg <= 0x7fffffff, "head_grad: ldg=%lld is beyond the unfused form's 32-bit stride", (long long)a.ldg);
    if (a.dimg) {
        if (int rc = launch_sgemm(false, false, a.B, a.e, a.C, p.scale, a.G, (int)a.ldg, a.txt_n, a.e, 0.f, a.dimg, a.e, nullptr, s)) return rc;
        hipLaunchKernelGGL(head_grad_rows_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a.dimg, a.img_n, a.img_inv, a.Eimg, a.gmul, a.B, a.e);
    }
    if (a.dtxt) {
        if (int rc = launch_sgemm(true, false, a.C, a.e, a.B, p.scale, a.G, (int)a.ldg, a.img_n, a.e, 0.f, a.dtxt, a.e, nullptr, s)) return rc;
        hipLaunchKernelGGL(head_grad_rows_kernel, dim3((a.C + 3) / 4), dim3(256), 0, s, a.dtxt, a.txt_n, a.txt_inv, a.Etxt, a.gmul, a.C, a.e);
    }
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
