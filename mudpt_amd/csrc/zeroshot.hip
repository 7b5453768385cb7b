// Zero-shot CLIP (trainers/zsclip.py): the two kernels a frozen handle (mudpt_create_frozen) adds to the text side.
//   embed_tokens      block 0's input of one prompt template straight from token ids: token_embedding(tokenized) + positional_embedding
//                     (clip/model.py:827) for the packed (length-bucketed) token rows, with no host-side [n_cls, 77, d] embedding
//   feature_ensemble  prompt ensembling (zsclip.py:107-115): normalise each template's features, average over the templates, normalise
//                     again; one template (zsclip.py:67-71): the plain normalisation
// Both are streaming kernels: no LDS, no atomics, every result a function of its own row alone, so the grid size never changes a bit.
#include <algorithm>

#include "kernels.h"

namespace mudpt {

// out[r, :] = table[tok[r], :] + pos[p[r], :].  A wave per row, grid-stride over the rows; 16-byte loads and stores (d % 4 == 0).  The two
// indices of a row are wave-uniform: they are read once per row, the next row's while this row streams, and held in scalar registers, so the
// inner loop is two loads, an add and a store at addresses that advance by one stride.  One fp32 add, one rounding: bit-exact.
__global__ __launch_bounds__(256) void embed_tokens_kernel(const float* __restrict__ table, const int* __restrict__ tok, const int* __restrict__ p,
                                                           const float* __restrict__ pos, float* __restrict__ out, int rows, int d) {
    const int lane = threadIdx.x & 63, stride = gridDim.x * 4, n4 = d >> 2;
    int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    int t = __builtin_amdgcn_readfirstlane(tok[r]), q = __builtin_amdgcn_readfirstlane(p[r]);
    while (true) {
        const int rn = r + stride;
        int tn = 0, qn = 0;
        if (rn < rows) { tn = tok[rn]; qn = p[rn]; }  // in flight under this row's copy
        const f32x4* a = (const f32x4*)(table + (size_t)t * d);
        const f32x4* b = (const f32x4*)(pos + (size_t)q * d);
        f32x4* o = (f32x4*)(out + (size_t)r * d);
        for (int k = lane; k < n4; k += 64) o[k] = a[k] + b[k];
        if (rn >= rows) return;
        r = rn; t = __builtin_amdgcn_readfirstlane(tn); q = __builtin_amdgcn_readfirstlane(qn);
    }
}

// Grid cap of the embed launch: 2048 workgroups of 4 waves (8 per CU); rows beyond one pass are reached by the grid stride
static constexpr int kEmbedMaxBlocks = 2048;

int launch_embed_tokens(const float* table, int vocab, const int* tokens, const int* positions, const float* pos, float* out, int rows, int d, hipStream_t s) {
    ARG_CHECK(table && tokens && positions && pos && out, "embed_tokens: null argument");
    ARG_CHECK(vocab >= 1 && rows >= 1 && d >= 1 && d % 4 == 0, "embed_tokens: vocab %d, rows %d, d %d: sizes must be >= 1 and d a multiple of 4", vocab, rows, d);
    const int blocks = std::min((rows + 3) / 4, kEmbedMaxBlocks);
    hipLaunchKernelGGL(embed_tokens_kernel, dim3(blocks), dim3(256), 0, s, table, tokens, positions, pos, out, rows, d);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

// A wave per class row c.  v = f[c] / |f[c]| (the sum of squares: lane l adds elements 4 l .. 4 l + 3, 256 + 4 l .., in ascending order, then
// the fixed DPP tree of wave_sum); acc[c] = v on the first template, acc[c] + v otherwise; on the last template out[c] = m / |m| with
// m = acc[c] / T -- and, with a single template, out[c] = v itself (zsclip.py:71 normalises once).  acc is not written on the last template.
__global__ __launch_bounds__(256) void feature_ensemble_kernel(const float* __restrict__ f, float* __restrict__ acc, float* __restrict__ out, int C, int e,
                                                               int first, int last, float T) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), n4 = e >> 2;
    if (c >= C) return;
    const f32x4* x = (const f32x4*)(f + (size_t)c * e);
    f32x4* a = (f32x4*)(acc + (size_t)c * e);
    f32x4* o = (f32x4*)(out + (size_t)c * e);
    float ss = 0.f;
    for (int k = lane; k < n4; k += 64) { const f32x4 v = x[k]; ss += v[0] * v[0]; ss += v[1] * v[1]; ss += v[2] * v[2]; ss += v[3] * v[3]; }
    const float inv = 1.0f / sqrtf(wave_sum(ss));
    if (first && last) {
        for (int k = lane; k < n4; k += 64) o[k] = x[k] * inv;
        return;
    }
    if (!last) {
        for (int k = lane; k < n4; k += 64) a[k] = first ? x[k] * inv : a[k] + x[k] * inv;
        return;
    }
    float s2 = 0.f;
    for (int k = lane; k < n4; k += 64) {
        const f32x4 m = (a[k] + x[k] * inv) / T;
        s2 += m[0] * m[0]; s2 += m[1] * m[1]; s2 += m[2] * m[2]; s2 += m[3] * m[3];
        o[k] = m;
    }
    const float inv2 = 1.0f / sqrtf(wave_sum(s2));
    for (int k = lane; k < n4; k += 64) o[k] = o[k] * inv2;  // each lane re-reads what it wrote itself
}

int launch_feature_ensemble(const float* f, float* acc, float* out, int C, int e, bool first, bool last, int n_templates, hipStream_t s) {
    ARG_CHECK(f && acc && out, "feature_ensemble: null argument");
    ARG_CHECK(f != acc && f != out && acc != out, "feature_ensemble: f, acc and out must be three different tables");
    ARG_CHECK(C >= 1 && e >= 1 && e % 4 == 0 && n_templates >= 1, "feature_ensemble: C %d, e %d, n_templates %d: sizes must be >= 1 and e a multiple of 4", C, e, n_templates);
    ARG_CHECK((n_templates == 1) == (first && last), "feature_ensemble: a call is both the first and the last of exactly one template");
    hipLaunchKernelGGL(feature_ensemble_kernel, dim3((C + 3) / 4), dim3(256), 0, s, f, acc, out, C, e, (int)first, (int)last, (float)n_templates);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
