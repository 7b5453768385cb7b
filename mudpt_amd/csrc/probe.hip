// The linear probe (lpclip/linear_probe.py: multinomial logistic regression on frozen CLIP features), one objective evaluation in HIP:
//   probe_gemm_kernel<false>   Z [M, N] = A [M, K] . B [N, K]^T + bias[N]                      (logits: A = features, B = W)
//   probe_gemm_kernel<true>    partial_z [M, N] = A[k in slice z, M]^T . B[k in slice z, N]    (A = P [samples, classes], B = features)
//   probe_tn_reduce_kernel     C = sum_z partial_z (z ascending) + beta W;  db[m] = sum_z (column sums of A over slice z)
//   probe_rows_kernel          per row of Z, in place: max, logsumexp, row loss, P = (softmax - onehot) / rows
//   probe_loss_sum_kernel      the row losses summed in double, in a fixed tree
//   probe_argmax_kernel        lowest index of the row maximum (numpy.argmax), optionally counted against labels
// The two GEMMs run on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 (one f32 per lane and operand, bit for bit a k-ordered fmaf
// chain): a workgroup of 4 waves owns a 128 x 128 tile, a wave 2 x 2 tiles of 32 x 32, and both operands of a 32-deep K-step pass through LDS
// once per workgroup -- each element loaded from memory feeds 128 products.  No atomics on floats anywhere: two runs give the same bits.
#include <algorithm>
#include <climits>

#include "kernels.h"

namespace mudpt {

constexpr int PB_T = 128, PB_S = 32;  // block edge, K-step
// LDS images of one operand's K-step.  k-contiguous operands (the logit GEMM): [128 rows][36]; a lane reads its row's k = 16 h .. 16 h + 15
// (h = lane >> 5) as four 16-byte reads, 16 lanes x 36 floats apart cover all 64 banks once.  The MFMA's k-step j then contracts k = 16 h + j
// of both operands: a permutation of the sum's order, the same for A and B.  Row-contiguous operands (the gradient GEMM): [32 k][160]; a
// lane reads element [2 j + h][row] with 4-byte reads, 160 = 128 + 32 puts the two lane halves on different banks.
constexpr int PB_LDK = 36, PB_LDM = 160;
constexpr int PB_LDS_FLOATS = 2 * PB_S * PB_LDM;  // 10240 floats = 40 KiB (the k-contiguous images need 2 * 128 * 36 = 9216)

struct ProbeGemmArgs {
    const float* A; const float* B;
    int M, N, K, lda, ldb;
    const float* bias;  // NT only, may be null
    float* C; int ldc;  // TN: the partial tile sets [slices][M][N], ldc = N
    float* db_part;     // TN only, may be null: [slices][M]
    int kper;           // TN only: depth of one slice, a multiple of PB_S
    bool vecA, vecB;    // the operand's base and stride allow 16-byte loads
};

// four consecutive elements from p, of which the first nvalid (<= 0: none) lie inside the operand; the rest are zero
__device__ __forceinline__ f32x4 probe_ld4(const float* __restrict__ p, bool vec, int nvalid) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (nvalid >= 4 && vec) v = *(const f32x4*)p;
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < nvalid) v[j] = p[j];
    }
    return v;
}

// One operand's part of a K-step into registers.  r0 = first row (k-contiguous form) or column (row-contiguous form) of the tile in the
// 128-wide dimension of extent dim; k0 .. kend the depth left.
template <bool TN>
__device__ __forceinline__ void probe_load(const float* __restrict__ P, int ld, bool vec, int r0, int dim, int k0, int kend, f32x4 v[4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (!TN) {
            const int row = r0 + (t >> 3) + 32 * r, k = k0 + (t & 7) * 4;
            v[r] = probe_ld4(P + (size_t)row * ld + k, vec, row < dim ? kend - k : 0);
        } else {
            const int k = k0 + (t >> 5) + 8 * r, col = r0 + (t & 31) * 4;
            v[r] = probe_ld4(P + (size_t)k * ld + col, vec, k < kend ? dim - col : 0);
        }
    }
}
template <bool TN>
__device__ __forceinline__ void probe_store(float* __restrict__ img, const f32x4 v[4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (!TN) *(f32x4*)&img[((t >> 3) + 32 * r) * PB_LDK + (t & 7) * 4] = v[r];
        else *(f32x4*)&img[((t >> 5) + 8 * r) * PB_LDM + (t & 31) * 4] = v[r];
    }
}

template <bool TN>
__global__ __launch_bounds__(256) void probe_gemm_kernel(ProbeGemmArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[PB_LDS_FLOATS];
    float* As = lds;
    float* Bs = lds + (TN ? PB_S * PB_LDM : PB_T * PB_LDK);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, i = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * PB_T, n0 = blockIdx.x * PB_T, z = blockIdx.z;
    const int kbeg = TN ? z * a.kper : 0, kend = TN ? min(a.K, kbeg + a.kper) : a.K;
    const bool want_db = TN && a.db_part != nullptr && blockIdx.x == 0 && t < PB_T;

    f32x16 acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
    float dbsum = 0.f;

    f32x4 ga[4], gb[4];
    probe_load<TN>(a.A, a.lda, a.vecA, m0, a.M, kbeg, kend, ga);
    probe_load<TN>(a.B, a.ldb, a.vecB, n0, a.N, kbeg, kend, gb);
    for (int k0 = kbeg; k0 < kend; k0 += PB_S) {
        probe_store<TN>(As, ga);
        probe_store<TN>(Bs, gb);
        __syncthreads();
        if (k0 + PB_S < kend) {  // the next K-step's loads fly under this one's products
            probe_load<TN>(a.A, a.lda, a.vecA, m0, a.M, k0 + PB_S, kend, ga);
            probe_load<TN>(a.B, a.ldb, a.vecB, n0, a.N, k0 + PB_S, kend, gb);
        }
        if (!TN) {
            f32x4 ar[2][4], br[2][4];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    ar[tt][q] = *(const f32x4*)&As[(wm * 64 + tt * 32 + i) * PB_LDK + 16 * h + 4 * q];
                    br[tt][q] = *(const f32x4*)&Bs[(wn * 64 + tt * 32 + i) * PB_LDK + 16 * h + 4 * q];
                }
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[tm][j >> 2][j & 3], br[tn][j >> 2][j & 3], acc[tm][tn], 0, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float* ap = &As[(2 * j + h) * PB_LDM + wm * 64 + i];
                const float* bp = &Bs[(2 * j + h) * PB_LDM + wn * 64 + i];
                const float a0 = ap[0], a1 = ap[32], b0 = bp[0], b1 = bp[32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
            if (want_db) {  // column sums of this slice of A, k ascending (rows past the depth are zero in the image)
#pragma unroll 8
                for (int k = 0; k < PB_S; ++k) dbsum += As[k * PB_LDM + t];
            }
        }
        __syncthreads();
    }

    // C / D layout of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = n0 + wn * 64 + tn * 32 + i;
            if (col >= a.N) continue;
            const float bias = (!TN && a.bias) ? a.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row >= a.M) continue;
                if (!TN) a.C[(size_t)row * a.ldc + col] = acc[tm][tn][r] + bias;
                else a.C[((size_t)z * a.M + row) * a.N + col] = acc[tm][tn][r];
            }
        }
    if (want_db && m0 + t < a.M) a.db_part[(size_t)z * a.M + m0 + t] = dbsum;
}

// second stage of the gradient GEMM: the slices in ascending order, then beta W in one fma
__global__ __launch_bounds__(256) void probe_tn_reduce_kernel(const float* __restrict__ part, const float* __restrict__ db_part, int slices, int M, int N, float beta,
                                                              const float* __restrict__ W, int ldw, float* __restrict__ C, int ldc, float* __restrict__ db) {
    const size_t MN = (size_t)M * N, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < MN) {
        float s = part[idx];
        for (int z = 1; z < slices; ++z) s += part[(size_t)z * MN + idx];
        const int m = (int)(idx / N), n = (int)(idx % N);
        if (W) s = __builtin_fmaf(beta, W[(size_t)m * ldw + n], s);
        C[(size_t)m * ldc + n] = s;
    } else if (db && idx < MN + M) {
        const int m = (int)(idx - MN);
        float s = db_part[m];
        for (int z = 1; z < slices; ++z) s += db_part[(size_t)z * M + m];
        db[m] = s;
    }
}

int probe_tn_slices(int M, int N, int Kd, int want, int ncu) {
    if (M < 1 || N < 1 || Kd < 1) return -1;
    const int steps = (Kd + PB_S - 1) / PB_S;
    const long tiles = (long)((M + PB_T - 1) / PB_T) * ((N + PB_T - 1) / PB_T);
    if (want <= 0) {  // two workgroups per compute unit, and at least two K-steps in every slice
        want = (int)std::max(1L, std::min(1024L, (2L * std::max(ncu, 1) + tiles - 1) / tiles));
        want = std::min(want, std::max(1, steps / 2));
    }
    want = std::min(std::min(want, steps), 1024);
    const int per = (steps + want - 1) / want;
    return (steps + per - 1) / per;
}

static bool probe_vec_ok(const float* p, int ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

int launch_probe_gemm_nt(int M, int N, int K, const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc, hipStream_t s) {
    ARG_CHECK(A && B && C, "probe_gemm_nt: null argument");
    ARG_CHECK(M >= 1 && N >= 1 && K >= 1 && (M + PB_T - 1) / PB_T <= 65535, "probe_gemm_nt: bad sizes M=%d N=%d K=%d", M, N, K);
    ARG_CHECK(lda >= K && ldb >= K && ldc >= N, "probe_gemm_nt: a stride is shorter than its row: lda=%d ldb=%d ldc=%d (M=%d N=%d K=%d)", lda, ldb, ldc, M, N, K);
    ProbeGemmArgs a{A, B, M, N, K, lda, ldb, bias, C, ldc, nullptr, 0, probe_vec_ok(A, lda), probe_vec_ok(B, ldb)};
    hipLaunchKernelGGL(probe_gemm_kernel<false>, dim3((N + PB_T - 1) / PB_T, (M + PB_T - 1) / PB_T, 1), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

int launch_probe_gemm_tn(int M, int N, int Kd, const float* A, int lda, const float* B, int ldb, float beta, const float* W, int ldw, float* C, int ldc, float* db,
                         float* scratch, size_t scratch_numel, int slices, hipStream_t s) {
    ARG_CHECK(A && B && C && scratch, "probe_gemm_tn: null argument");
    ARG_CHECK(M >= 1 && N >= 1 && Kd >= 1 && (M + PB_T - 1) / PB_T <= 65535, "probe_gemm_tn: bad sizes M=%d N=%d K=%d", M, N, Kd);
    ARG_CHECK(lda >= M && ldb >= N && ldc >= N && (!W || ldw >= N), "probe_gemm_tn: a stride is shorter than its row: lda=%d ldb=%d ldw=%d ldc=%d (M=%d N=%d)", lda,
              ldb, ldw, ldc, M, N);
    ARG_CHECK(C != W && C != A && C != B && db != A, "probe_gemm_tn: an output aliases an input");
    if (slices <= 0) {
        const int ncu = device_cus(current_device());
        if (ncu <= 0) return MUDPT_ERR_HIP;
        slices = probe_tn_slices(M, N, Kd, 0, ncu);
    } else slices = probe_tn_slices(M, N, Kd, slices, 1);
    const size_t need = (size_t)slices * ((size_t)M * N + M);
    ARG_CHECK(scratch_numel >= need, "probe_gemm_tn: scratch of %zu elements, %d slices of %d x %d need %zu", scratch_numel, slices, M, N, need);
    const int steps = (Kd + PB_S - 1) / PB_S, per = (steps + slices - 1) / slices;
    float* db_part = scratch + (size_t)slices * M * N;
    ProbeGemmArgs a{A, B, M, N, Kd, lda, ldb, nullptr, scratch, N, db ? db_part : nullptr, per * PB_S, probe_vec_ok(A, lda), probe_vec_ok(B, ldb)};
    hipLaunchKernelGGL(probe_gemm_kernel<true>, dim3((N + PB_T - 1) / PB_T, (M + PB_T - 1) / PB_T, slices), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    const size_t total = (size_t)M * N + (db ? M : 0);
    hipLaunchKernelGGL(probe_tn_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, scratch, db_part, slices, M, N, beta, W, ldw, C, ldc, db);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

__device__ inline int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
// lowest index of the row's maximum: lane l looks at columns l, l + 64, ... in ascending order
__device__ inline int probe_row_argmax(const float* __restrict__ z, int C, int lane, float& m) {
    float mx = -INFINITY;
    for (int j = lane; j < C; j += 64) mx = fmaxf(mx, z[j]);
    m = wave_max(mx);
    int jm = INT_MAX;
    for (int j = lane; j < C; j += 64) if (z[j] == m) jm = min(jm, j);
    jm = wave_min_int(jm);
    return jm == INT_MAX ? 0 : jm;  // a row of NaN has no maximum
}

// exp(a - m) for a <= m without the rounding of the difference: d = fl(a - m) is off by up to half an ulp of |d| (2e-6 at |d| = 40, as a
// RELATIVE error of the exponential), but that error is itself an fp32 number (the two-sum), and exp(d + r) = exp(d) (1 + r) to r^2.
__device__ inline float probe_exp_diff(float a, float m) {
    const float c = -m, d = a + c, bp = d - a, ap = d - bp, r = (a - ap) + (c - bp);
    const float e = expf(d);
    return __builtin_fmaf(e, r, e);
}

// A wave per row.  With m the maximum at column jm, s = sum_{j != jm} exp(z_j - m) (lane l adds its columns in ascending order, then the fixed
// tree of wave_sum) and the row's sum of exponentials is 1 + s exactly as far as fp32 can say, so
//   row loss = logsumexp(z) - z_y = log1p(s) + (m - z_y)      -- no cancellation when the label's probability rounds to 1,
//   P_j = exp(z_j - m) / (1 + s) - [j == y], and for y == jm the difference is -s / (1 + s) instead of 1 / (1 + s) - 1.
// expf / log1pf are the full-precision library functions: the error of P steers the optimiser.  The labels are trusted (the host checks them once per fit).
__global__ __launch_bounds__(256) void probe_rows_kernel(float* __restrict__ Z, int ldz, const int* __restrict__ labels, int rows, int C, float inv_rows,
                                                         float* __restrict__ row_loss) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float* z = Z + (size_t)r * ldz;
    const int y = labels[r];
    float m;
    const int jm = probe_row_argmax(z, C, lane, m);
    float zy = z[y];
    float s = 0.f;
    for (int j = lane; j < C; j += 64) if (j != jm) s += probe_exp_diff(z[j], m);
    s = wave_sum(s);
    asm volatile("" : "+v"(zy));  // z[y] has arrived before any lane overwrites the row
    const float tot = 1.f + s;
    for (int j = lane; j < C; j += 64) {
        const float e = j == jm ? 1.f : probe_exp_diff(z[j], m);
        float p = e / tot;
        if (j == y) p = j == jm ? -s / tot : p - 1.f;
        z[j] = p * inv_rows;
    }
    if (lane == 0) row_loss[r] = log1pf(s) + (m - zy);
}

__global__ __launch_bounds__(256) void probe_loss_sum_kernel(const float* __restrict__ row_loss, int rows, double* __restrict__ out) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int r = t; r < rows; r += 256) s += (double)row_loss[r];
    part[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) out[0] = part[0];
}

int launch_probe_rows(float* Z, int ldz, const int* labels, int rows, int n_cls, float* row_loss, double* loss_sum, hipStream_t s) {
    ARG_CHECK(Z && labels && row_loss && loss_sum, "probe_rows: null argument");
    ARG_CHECK(rows >= 1 && n_cls >= 1 && ldz >= n_cls, "probe_rows: rows %d, n_cls %d, ldz %d", rows, n_cls, ldz);
    hipLaunchKernelGGL(probe_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, Z, ldz, labels, rows, n_cls, (float)(1.0 / (double)rows), row_loss);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(probe_loss_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)row_loss, rows, loss_sum);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

__global__ __launch_bounds__(256) void probe_argmax_kernel(const float* __restrict__ Z, int ldz, int rows, int C, int* __restrict__ pred, const int* __restrict__ labels,
                                                           int* __restrict__ count) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float m;
    const int jm = probe_row_argmax(Z + (size_t)r * ldz, C, lane, m);
    if (lane == 0) {
        pred[r] = jm;
        if (labels && count && labels[r] == jm) atomicAdd(count, 1);  // an integer count: the order of the adds does not change it
    }
}

int launch_probe_argmax(const float* Z, int ldz, int rows, int n_cls, int* pred, const int* labels, int* count, hipStream_t s) {
    ARG_CHECK(Z && pred, "probe_argmax: null argument");
    ARG_CHECK((labels == nullptr) == (count == nullptr), "probe_argmax: labels and count come together");
    ARG_CHECK(rows >= 1 && n_cls >= 1 && ldz >= n_cls, "probe_argmax: rows %d, n_cls %d, ldz %d", rows, n_cls, ldz);
    if (count) HIP_TRY(hipMemsetAsync(count, 0, sizeof(int), s));
    hipLaunchKernelGGL(probe_argmax_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, Z, ldz, rows, n_cls, pred, labels, count);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
