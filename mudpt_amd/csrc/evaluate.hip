// The test pass's evaluator on the device (Dassl's evaluation/evaluator.py Classification: accuracy, macro-F1, per-class results, confusion
// matrix).  The state is ONE int32 buffer (include/mudpt.h at mudpt_eval_accumulate):
//   [total, correct, invalid, reserved] [support: C] [predicted: C] [hit: C] [cmat: C x C, row = label, column = prediction; with_cmat only]
//   eval_accumulate_kernel   a wave per row: the prediction by torch.max(logits, 1)[1]'s CPU rule, every logit read ONCE, then integer atomics
//   eval_finalize_kernel     one workgroup: macro-F1 and the mean per-class accuracy over the classes with support, double sums in a fixed order
// Only integers are added atomically, so the order of the adds does not change the state: two runs give the same bits.
#include <climits>

#include "eval_order.h"  // eval_take: the first NaN wins, otherwise the lowest index of the largest value; shared with topk.hip
#include "kernels.h"

namespace mudpt {

constexpr int EV_HEAD = 4;  // total, correct, invalid, reserved

template <bool VEC>
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const float* __restrict__ Z, int ldz, const int64_t* __restrict__ labels, int rows, int C,
                                                              int* __restrict__ state, int with_cmat, int* __restrict__ pred) {
    __shared__ int tally[3][4];  // total, correct, invalid of the workgroup's four rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x * 4 + wave;
    int valid = 0, hit = 0, bad = 0;
    if (r < rows) {
        const float* z = Z + (size_t)r * ldz;
        const int64_t y = labels[r];  // in flight with the logits; only lane 0 uses it
        float v = -INFINITY;
        int i = INT_MAX;  // a lane without a column: loses against every column, -inf included
        if (VEC) {
            const int C4 = C & ~3;
            for (int j = 4 * lane; j < C4; j += 256) {
                const f32x4 q = *(const f32x4*)(z + j);
#pragma unroll
                for (int k = 0; k < 4; ++k) eval_take(v, i, q[k], j + k);
            }
            if (C4 + lane < C) eval_take(v, i, z[C4 + lane], C4 + lane);
        } else {
            for (int j = lane; j < C; j += 64) eval_take(v, i, z[j], j);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o);
            const int oi = __shfl_xor(i, o);
            eval_take(v, i, ov, oi);
        }
        if (lane == 0) {
            valid = y >= 0 && y < C;
            bad = !valid;
            if (valid) {  // the label indexes nothing before this test
                int* support = state + EV_HEAD;
                hit = (int64_t)i == y;
                atomicAdd(support + y, 1);
                atomicAdd(support + C + i, 1);
                if (hit) atomicAdd(support + 2 * C + y, 1);
                if (with_cmat) atomicAdd(support + 3 * (size_t)C + (size_t)y * C + i, 1);
            }
            if (pred) pred[r] = valid ? i : -1;
        }
    }
    if (lane == 0) { tally[0][wave] = valid; tally[1][wave] = hit; tally[2][wave] = bad; }
    __syncthreads();
    if (threadIdx.x < 3) {  // one global add per counter and workgroup
        const int t = threadIdx.x, n = tally[t][0] + tally[t][1] + tally[t][2] + tally[t][3];
        if (n) atomicAdd(state + t, n);
    }
}

__global__ __launch_bounds__(256) void eval_finalize_kernel(const int* __restrict__ state, int C, double* __restrict__ results) {
    __shared__ double part[3][256];
    const int t = threadIdx.x;
    const int* support = state + EV_HEAD;
    double f1 = 0.0, acc = 0.0, n = 0.0;
    for (int c = t; c < C; c += 256) {
        const int s = support[c];
        if (s > 0) {
            const double h = (double)support[2 * (size_t)C + c];
            f1 += 2.0 * h / ((double)s + (double)support[C + c]);
            acc += 100.0 * h / (double)s;
            n += 1.0;
        }
    }
    part[0][t] = f1; part[1][t] = acc; part[2][t] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < 3; ++k) part[k][t] += part[k][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double ns = part[2][0];
        results[0] = (double)state[0]; results[1] = (double)state[1]; results[2] = (double)state[2]; results[3] = ns;
        results[4] = ns > 0.0 ? 100.0 * (part[0][0] / ns) : 0.0;
        results[5] = ns > 0.0 ? part[1][0] / ns : 0.0;
    }
}

static bool eval_cmat_fits(int n_cls) { return (int64_t)n_cls * n_cls < ((int64_t)1 << 31); }

size_t eval_state_numel(int n_cls, int with_cmat) {
    if (n_cls < 1 || (with_cmat && !eval_cmat_fits(n_cls))) return 0;
    return EV_HEAD + 3 * (size_t)n_cls + (with_cmat ? (size_t)n_cls * n_cls : 0);
}

int launch_eval_reset(int* state, int n_cls, int with_cmat, hipStream_t s) {
    ARG_CHECK(state, "eval_reset: null argument");
    ARG_CHECK(n_cls >= 1, "eval_reset: n_cls %d", n_cls);
    ARG_CHECK(!with_cmat || eval_cmat_fits(n_cls), "eval_reset: a confusion matrix of %d x %d cells does not fit 2^31", n_cls, n_cls);
    HIP_TRY(hipMemsetAsync(state, 0, eval_state_numel(n_cls, with_cmat) * sizeof(int), s));
    return MUDPT_OK;
}

int launch_eval_accumulate(const float* logits, int ldz, const int64_t* labels, int rows, int n_cls, int* state, int with_cmat, int* pred, hipStream_t s) {
    ARG_CHECK(logits && labels && state, "eval_accumulate: null argument");
    ARG_CHECK(rows >= 1 && n_cls >= 1 && ldz >= n_cls, "eval_accumulate: rows %d, n_cls %d, ldz %d", rows, n_cls, ldz);
    ARG_CHECK(!with_cmat || eval_cmat_fits(n_cls), "eval_accumulate: a confusion matrix of %d x %d cells does not fit 2^31", n_cls, n_cls);
    const dim3 grid((rows + 3) / 4), block(256);
    if (((uintptr_t)logits & 15) == 0 && ldz % 4 == 0)
        hipLaunchKernelGGL(eval_accumulate_kernel<true>, grid, block, 0, s, logits, ldz, labels, rows, n_cls, state, with_cmat, pred);
    else
        hipLaunchKernelGGL(eval_accumulate_kernel<false>, grid, block, 0, s, logits, ldz, labels, rows, n_cls, state, with_cmat, pred);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

int launch_eval_finalize(const int* state, int n_cls, double* results, hipStream_t s) {
    ARG_CHECK(state && results, "eval_finalize: null argument");
    ARG_CHECK(n_cls >= 1, "eval_finalize: n_cls %d", n_cls);
    hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(256), 0, s, state, n_cls, results);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
