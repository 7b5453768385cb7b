// What comes right after the logits: the first k columns of every row in the evaluator's order (ranked predictions, with their logits and
// their softmax probabilities), and the rank of every row's label (top-k accuracy for every k at once).  include/mudpt.h at mudpt_topk.
//   topk_kernel             a wave per row, four rows per workgroup.  Selection without a sort and without LDS: round t takes, per lane and then
//                           over the __shfl_xor tree, the best column that the winner of round t - 1 strictly precedes (eval_order.h: the order
//                           is total and "the best of" associative, so the tree may group in any way).  Round 0 starts from a winner that
//                           precedes every column.  Lane t keeps the winner of round t, so that the k <= 64 outputs of a row leave as one store.
//                           A wave runs alone on its SIMD (256 rows are 64 workgroups on 256 compute units), so a launch takes as long as
//                           one wave's instructions: a column is therefore ranked by its 64-bit eval_rank_key, made once, and a round costs
//                           two integer comparisons per column where eval_precedes + eval_take cost about twenty instructions.
//                           Every logit is fetched from memory once: up to C = 1027 (TOPK_REG_GROUPS groups of four columns and one tail
//                           column per lane, 17 registers of keys) a lane loads its columns before round 0 and every round and the softmax
//                           sum read registers; above that round 0 fetches the row and the later walks find the same addresses in the
//                           cache.  The key gives the logit back but for a zero's sign, so `value` is read again at the k winners.
//                           prob: m = the logit of round 0's winner (the row maximum, or the first NaN), terms expf(z - m) with the accurate
//                           expf; a lane adds the terms of its columns in ascending column order, then the xor tree 32, 16, .. 1, then one
//                           division per output.  The columns of a lane do not depend on the load form (eval_for_columns), so the chain -- at
//                           most 4 ceil((C & ~3) / 256) + (C % 4 != 0) terms in a lane, then 6 tree adds -- is the same for a row wherever it
//                           lies.  A row with a NaN, a +inf or only -inf makes m - m or z - m a NaN, and with it every probability, as torch.
//   rank_accumulate_kernel  the same shape; one pass counts the columns that precede the label's, which is the label's rank.  Integer atomics
//                           only (one per counter and workgroup, one per row into the histogram): two runs give the same bits.
#include "eval_order.h"
#include "kernels.h"

namespace mudpt {

constexpr int TOPK_MAX = 64;    // a lane per output
constexpr int RANK_HEAD = 2;    // total, invalid
constexpr int TOPK_REG_GROUPS = 4;  // groups of four columns a lane keeps in registers: rows of up to 4 * 256 + 3 columns

// The columns of one row that belong to a lane as f(eval_key(z[j]), j), visited as eval_for_columns visits them.  REG: loaded once, then the
// keys in registers.
template <bool VEC, bool REG>
struct LaneColumns {
    const float* z;
    int C, lane;
    unsigned q[TOPK_REG_GROUPS][4], tail;
    __device__ __forceinline__ LaneColumns(const float* __restrict__ z_, int C_, int lane_) : z(z_), C(C_), lane(lane_) {
        if (!REG) return;
        const unsigned C4 = (unsigned)C & ~3u;
#pragma unroll
        for (int g = 0; g < TOPK_REG_GROUPS; ++g) {
            const unsigned j = 4u * lane + 256u * g;
            if (j < C4) {
                f32x4 v;
                if (VEC) {
                    v = *(const f32x4*)(z + j);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = z[j + k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) q[g][k] = eval_key(v[k]);
            }
        }
        if (C4 + lane < (unsigned)C) tail = eval_key(z[C4 + lane]);
    }
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
        if (!REG) {
            eval_for_columns<VEC>(z, C, lane, [&](float zj, int j) { f(eval_key(zj), j); });
            return;
        }
        const unsigned C4 = (unsigned)C & ~3u;
#pragma unroll
        for (int g = 0; g < TOPK_REG_GROUPS; ++g) {
            const unsigned j = 4u * lane + 256u * g;
            if (j < C4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) f(q[g][k], (int)(j + k));
            }
        }
        if (C4 + lane < (unsigned)C) f(tail, (int)(C4 + lane));
    }
};

template <bool VEC, bool REG>
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ Z, int ldz, int rows, int C, int k, int* __restrict__ index,
                                                   float* __restrict__ value, float* __restrict__ prob) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;  // the whole wave; nothing below synchronises across waves
    const float* z = Z + (size_t)r * ldz;
    const LaneColumns<VEC, REG> row(z, C, lane);
    unsigned long long prev = ~0ull, mine = 0ull;  // all ones precedes every column: round 0 takes the best of all
    float m = 0.f;
    for (int t = 0; t < k; ++t) {
        unsigned long long best = 0ull;  // a lane without a candidate: every column precedes it
        row.each([&](unsigned key, int j) {
            const unsigned long long c = eval_rank_key(key, j);
            if (c < prev && c > best) best = c;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if (t == 0) m = eval_key_value((unsigned)(best >> 32));
        if (lane == t) mine = best;
        prev = best;  // k <= C: every round finds a column
    }
    const size_t out = (size_t)r * k + lane;
    if (lane < k) {
        const int i = eval_rank_key_index(mine);
        index[out] = i;
        if (value) value[out] = z[i];  // bit for bit, a zero's sign included; from the cache
    }
    if (prob) {
        float s = 0.f;
        row.each([&](unsigned key, int) { s += expf(eval_key_value(key) - m); });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);  // a + b == b + a bit for bit: every lane ends with the same sum
        if (lane < k) prob[out] = expf(eval_key_value((unsigned)(mine >> 32)) - m) / s;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void rank_accumulate_kernel(const float* __restrict__ Z, int ldz, const int64_t* __restrict__ labels, int rows, int C,
                                                              int kmax, int* __restrict__ state, int* __restrict__ rank) {
    __shared__ int tally[RANK_HEAD][4];  // total, invalid of the workgroup's four rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x * 4 + wave;
    int valid = 0, bad = 0;
    if (r < rows) {
        const int64_t y = labels[r];  // the same in every lane
        valid = y >= 0 && y < C;
        bad = !valid;
        int n = -1;
        if (valid) {  // the label indexes nothing before this test
            const float* z = Z + (size_t)r * ldz;
            const float zy = z[y];
            const int yi = (int)y;
            n = 0;
            eval_for_columns<VEC>(z, C, lane, [&](float zj, int j) { n += eval_precedes(zj, j, zy, yi) ? 1 : 0; });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
            if (lane == 0 && n < kmax) atomicAdd(state + RANK_HEAD + n, 1);
        }
        if (lane == 0 && rank) rank[r] = n;
    }
    if (lane == 0) { tally[0][wave] = valid; tally[1][wave] = bad; }
    __syncthreads();
    if (threadIdx.x < RANK_HEAD) {  // one global add per counter and workgroup
        const int t = threadIdx.x, n = tally[t][0] + tally[t][1] + tally[t][2] + tally[t][3];
        if (n) atomicAdd(state + t, n);
    }
}

static bool loads_16_bytes(const float* logits, int ldz) { return ((uintptr_t)logits & 15) == 0 && ldz % 4 == 0; }

int launch_topk(const float* logits, int ldz, int rows, int n_cls, int k, int* index, float* value, float* prob, hipStream_t s) {
    ARG_CHECK(logits, "topk: null logits");
    ARG_CHECK(index, "topk: null index");
    ARG_CHECK(rows >= 1, "topk: rows %d", rows);
    ARG_CHECK(n_cls >= 1, "topk: n_cls %d", n_cls);
    ARG_CHECK(ldz >= n_cls, "topk: ldz %d is less than n_cls %d", ldz, n_cls);
    ARG_CHECK(k >= 1 && k <= TOPK_MAX, "topk: k %d is outside 1 .. %d", k, TOPK_MAX);
    ARG_CHECK(k <= n_cls, "topk: k %d is more than n_cls %d", k, n_cls);
    const dim3 grid((rows + 3) / 4), block(256);
    const bool vec = loads_16_bytes(logits, ldz), reg = (n_cls & ~3) <= 256 * TOPK_REG_GROUPS;
    auto kernel = vec ? (reg ? topk_kernel<true, true> : topk_kernel<true, false>) : (reg ? topk_kernel<false, true> : topk_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, logits, ldz, rows, n_cls, k, index, value, prob);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

int launch_rank_accumulate(const float* logits, int ldz, const int64_t* labels, int rows, int n_cls, int kmax, int* state, int* rank, hipStream_t s) {
    ARG_CHECK(logits, "rank_accumulate: null logits");
    ARG_CHECK(labels, "rank_accumulate: null labels");
    ARG_CHECK(state, "rank_accumulate: null state");
    ARG_CHECK(rows >= 1, "rank_accumulate: rows %d", rows);
    ARG_CHECK(n_cls >= 1, "rank_accumulate: n_cls %d", n_cls);
    ARG_CHECK(ldz >= n_cls, "rank_accumulate: ldz %d is less than n_cls %d", ldz, n_cls);
    ARG_CHECK(kmax >= 1 && kmax <= TOPK_MAX, "rank_accumulate: kmax %d is outside 1 .. %d", kmax, TOPK_MAX);
    const dim3 grid((rows + 3) / 4), block(256);
    if (loads_16_bytes(logits, ldz))
        hipLaunchKernelGGL(rank_accumulate_kernel<true>, grid, block, 0, s, logits, ldz, labels, rows, n_cls, kmax, state, rank);
    else
        hipLaunchKernelGGL(rank_accumulate_kernel<false>, grid, block, 0, s, logits, ldz, labels, rows, n_cls, kmax, state, rank);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
