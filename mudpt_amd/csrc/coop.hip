// CoOp (trainers/coop.py): the prompt splice of the learnable context and its gradient.  CoOp's context rows sit at a different row of
// every class prompt (CLASS_TOKEN_POSITION middle / front, coop.py:99-164) and, with CSC, every class has its own context; both are
// encoded in two host-built tables in the CALLER's class order (mudpt_set_class_prompts):
//   rows[c * n + j]  token row, inside the text tower's packed (length-bucketed) layout, that context row j of class c occupies
//   pos[c * n + j]   its position inside the prompt (the row of the positional embedding it receives, coop.py:187-190)
// so one code path serves every (position, CSC) combination and every bucket layout.  Both kernels are memory-trivial.
#include "kernels.h"

namespace mudpt {

// x[rows[c n + j]] = ctx[csc ? c : 0][j] + tpos[pos[c n + j]]  (16-byte accesses; the frozen rows were uploaded with tpos added)
__global__ __launch_bounds__(128) void coop_splice_kernel(float* __restrict__ x, const float* __restrict__ ctx, const float* __restrict__ tpos,
                                                          const int* __restrict__ rows, const int* __restrict__ pos, int n, int d, int csc) {
    const int cj = blockIdx.x, c = cj / n, j = cj % n;
    f32x4* dst = (f32x4*)(x + (size_t)rows[cj] * d);
    const f32x4* src = (const f32x4*)(ctx + ((size_t)(csc ? c : 0) * n + j) * d);
    const f32x4* p = (const f32x4*)(tpos + (size_t)pos[cj] * d);
    for (int k = threadIdx.x; k < d / 4; k += blockDim.x) dst[k] = src[k] + p[k];
}

int launch_coop_splice(float* x, const float* ctx, const float* tpos, const int* rows, const int* pos, int C, int n, int d, bool csc, hipStream_t s) {
    ARG_CHECK(x && ctx && tpos && rows && pos && C > 0 && n > 0 && d > 0 && d % 4 == 0, "coop_splice: bad arguments");
    hipLaunchKernelGGL(coop_splice_kernel, dim3(C * n), dim3(128), 0, s, x, ctx, tpos, rows, pos, n, d, (int)csc);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

// Context gradient.  Workgroup = 8 column groups of 8 columns x 32 class lanes, over context row j = blockIdx.x and columns
// blockIdx.y * 64 ..; each thread reads 8 consecutive columns of one token row (two 16-byte fp32 loads or one 16-byte T load).
//   shared (csc = 0, gridDim.z = 1): lane l accumulates classes l, l + 32, l + 64, ... in ascending order; the 32 lane partials are then
//                                    added in ascending lane order.  The order depends on C only -- not on the bucket layout, the timing or
//                                    the run: bit-identical results (no float atomics).
//   CSC (csc = 1):                   lane l of z-block z handles class 32 z + l alone: dctx[c][j] = scale * dx[rows[c n + j]].
template <typename T>
__global__ __launch_bounds__(256) void coop_dctx_kernel(const float* __restrict__ dx, const typename T::elem* __restrict__ dx_lp,
                                                        const int* __restrict__ rows, float* __restrict__ out, int C, int n, int d, float scale, int csc) {
    __shared__ float part[32][65];
    const int cg = threadIdx.x & 7, lane = threadIdx.x >> 3;
    const int j = blockIdx.x, col = blockIdx.y * 64 + cg * 8;
    const int c0 = blockIdx.z * 32 + lane, c1 = csc ? (c0 + 1 < C ? c0 + 1 : C) : C;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = c0; c < c1; c += 32) {
        const size_t o = (size_t)rows[c * n + j] * d + col;
        if (dx) {
            const f32x4 a = *(const f32x4*)(dx + o), b = *(const f32x4*)(dx + o + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc[k] += a[k]; acc[4 + k] += b[k]; }
        } else {  // the gradient stream lives in T only (lp_grad)
            const typename T::vec8 v = *(const typename T::vec8*)(dx_lp + o);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += (float)v[k];
        }
    }
    if (csc) {
        if (c0 < C) {
            float* dst = out + ((size_t)c0 * n + j) * d + col;
            *(f32x4*)dst = f32x4{acc[0], acc[1], acc[2], acc[3]} * scale;
            *(f32x4*)(dst + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]} * scale;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) part[lane][cg * 8 + k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 64) {
        float t = 0.f;
        for (int l = 0; l < 32; ++l) t += part[l][threadIdx.x];
        out[(size_t)j * d + blockIdx.y * 64 + threadIdx.x] = t * scale;
    }
}

int launch_coop_dctx(int dtype, const float* dx, const void* dx_lp, const int* rows, float* dctx, int C, int n, int d, bool csc, float scale, hipStream_t s) {
    ARG_CHECK((dx || dx_lp) && rows && dctx && C > 0 && n > 0 && d > 0 && d % 64 == 0, "coop_dctx: bad arguments");
    const dim3 grid(n, d / 64, csc ? (C + 31) / 32 : 1);
    if (dtype == DT_BF16) hipLaunchKernelGGL(coop_dctx_kernel<BF16>, grid, dim3(256), 0, s, dx, (const __bf16*)dx_lp, rows, dctx, C, n, d, scale, (int)csc);
    else if (dtype == DT_F16) hipLaunchKernelGGL(coop_dctx_kernel<F16>, grid, dim3(256), 0, s, dx, (const _Float16*)dx_lp, rows, dctx, C, n, d, scale, (int)csc);
    else { set_error("coop_dctx: unknown dtype %d", dtype); return MUDPT_ERR_ARG; }
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
