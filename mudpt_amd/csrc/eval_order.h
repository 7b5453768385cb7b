// The one order the evaluator (evaluate.hip) and top-k (topk.hip) rank the columns of a row of logits by, and the walk both take over a row.
#pragma once
#include "common.h"

namespace mudpt {

// Does column (av, ai) precede column (bv, bi)?  The key is (is NaN, value, -index): NaNs first in index order, then the values descending,
// equal values (+0 == -0) in index order.  It is torch's CPU max carried to every place -- `if (!(value <= max)) { max = value; index = i;
// if (isnan(value)) break; }` takes the first NaN, otherwise the lowest index of the largest value -- and equals torch.sort(descending=True,
// stable=True) on the CPU.  A strict total order on distinct indices, so "the best of" is associative: lanes and the wave tree may combine
// their candidates in any grouping.
__device__ __forceinline__ bool eval_precedes(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    return an ? (!bn || ai < bi) : (!bn && (av > bv || (av == bv && ai < bi)));
}

// (v, i) becomes the better of itself and (ov, oi)
__device__ __forceinline__ void eval_take(float& v, int& i, float ov, int oi) {
    if (eval_precedes(ov, oi, v, i)) { v = ov; i = oi; }
}

// The same order as ONE unsigned comparison, for code that ranks a row more than once: a precedes b iff eval_rank_key(eval_key(z[a]), a)
// > eval_rank_key(eval_key(z[b]), b).  The high word is eval_key(z): all ones for a NaN, 0x80000000 for either zero, else the float's bits made monotonic
// (sign bit set on a positive value, all bits flipped on a negative one); integer tests only, so no floating-point mode has a say.  The low
// word falls with the index.  No column has the key 0 (a lane without a candidate) or all ones (what precedes every column).
__device__ __forceinline__ unsigned eval_key(float z) {
    const unsigned u = __float_as_uint(z);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if ((u << 1) == 0u) return 0x80000000u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// z again from eval_key(z), but for the sign of a zero and the payload of a NaN
__device__ __forceinline__ float eval_key_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }
__device__ __forceinline__ unsigned long long eval_rank_key(unsigned key, int index) {
    return ((unsigned long long)key << 32) | (0xfffffffeu - (unsigned)index);
}
__device__ __forceinline__ int eval_rank_key_index(unsigned long long k) { return (int)(0xfffffffeu - (unsigned)k); }

// f(z[j], j) for the columns of one row that belong to `lane` of a wave, in ascending j: the groups of four from column 4 * lane on, every
// 256 columns, then column (C & ~3) + lane of the ragged tail.  VEC: a group is one 16-byte load (z 16-byte aligned); else four scalar
// loads of the SAME columns, so that a per-lane result does not depend on the form.  unsigned: j + 256 must not wrap for C near 2^31.
template <bool VEC, class F>
__device__ __forceinline__ void eval_for_columns(const float* __restrict__ z, int C, int lane, F&& f) {
    const unsigned C4 = (unsigned)C & ~3u;
    for (unsigned j = 4u * lane; j < C4; j += 256u) {
        f32x4 q;
        if (VEC) {
            q = *(const f32x4*)(z + j);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = z[j + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) f(q[k], (int)(j + k));
    }
    if (C4 + lane < (unsigned)C) f(z[C4 + lane], (int)(C4 + lane));
}

}  // namespace mudpt
