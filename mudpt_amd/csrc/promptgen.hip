// UMuDPT's prompt generator (trainers/umudpt.py:56-76,161-178): ln_pre -> one pre-LN transformer block -> ln_post -> visual_proj over the
// R = depth * n_ctx prompt rows, forward and backward, in fp32 end to end.  Unlike everything else in the library the generator's weights
// TRAIN: its backward produces weight, bias, gamma and beta gradients.  R is 16 at the defaults and a few hundred at most, so every kernel
// here is a latency problem, not a throughput one: the forward's GEMMs are launch_sgemm, a Linear's three gradients one launch_linear_bwd, and the three kernels of
// this file -- LayerNorm backward with dgamma / dbeta, attention over the n_ctx <= 16 rows of one layer, QuickGELU -- keep every sum in a
// fixed order (no atomics), so two runs agree bit for bit.
#include "kernels.h"

namespace mudpt {

// ---- LayerNorm backward with the affine gradients -------------------------------------------------------------------------------------
// Blocks 0 .. ceil(rows / 4) - 1: one wave per row, dx = (dres +) rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma (as ln_bwd_kernel).
// The blocks behind them: one thread per column, dgamma[j] = sum_r dy[r][j] xhat[r][j] and dbeta[j] = sum_r dy[r][j] in row order.
constexpr int LNA_MAXV = 4;  // float4 per lane: d <= 1024
__global__ __launch_bounds__(256) void ln_bwd_affine_kernel(LnBwdAffineArgs p, int row_blocks) {
    if ((int)blockIdx.x >= row_blocks) {
        const int j = ((int)blockIdx.x - row_blocks) * 256 + threadIdx.x;
        if (j >= p.d) return;
        float sg = 0.f, sb = 0.f;
        for (int r = 0; r < p.rows; ++r) {
            const float dy = p.dy[(size_t)r * p.lddy + j];
            const float xh = (p.x[(size_t)r * p.ldx + j] - p.mean[r]) * p.rstd[r];
            sg += dy * xh;
            sb += dy;
        }
        p.dgamma[j] = p.accumulate ? p.dgamma[j] + sg : sg;
        p.dbeta[j] = p.accumulate ? p.dbeta[j] + sb : sb;
        return;
    }
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.rows) return;
    const int d4 = p.d >> 2;
    const f32x4* x = (const f32x4*)(p.x + (size_t)r * p.ldx);
    const f32x4* dyr = (const f32x4*)(p.dy + (size_t)r * p.lddy);
    const float mean = p.mean[r], rstd = p.rstd[r];
    f32x4 xh[LNA_MAXV], g[LNA_MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < LNA_MAXV; ++k) {
        const int i = lane + 64 * k;
        xh[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        g[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < d4) {
            const f32x4 xv = x[i], dy = dyr[i], gm = ((const f32x4*)p.gamma)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xh[k][j] = (xv[j] - mean) * rstd;
                g[k][j] = dy[j] * gm[j];
                s1 += g[k][j];
                s2 += g[k][j] * xh[k][j];
            }
        }
    }
    const float c1 = wave_sum(s1) / p.d, c2 = wave_sum(s2) / p.d;
#pragma unroll
    for (int k = 0; k < LNA_MAXV; ++k) {
        const int i = lane + 64 * k;
        if (i < d4) {
            f32x4 dx;
#pragma unroll
            for (int j = 0; j < 4; ++j) dx[j] = rstd * (g[k][j] - c1 - xh[k][j] * c2);
            if (p.dres) dx += ((const f32x4*)(p.dres + (size_t)r * p.lddres))[i];
            ((f32x4*)(p.dx + (size_t)r * p.lddx))[i] = dx;
        }
    }
}

int launch_ln_bwd_affine(const LnBwdAffineArgs& a, hipStream_t s) {
    ARG_CHECK(a.x && a.mean && a.rstd && a.gamma && a.dy && a.dx && a.dgamma && a.dbeta, "ln_bwd_affine: null operand");
    ARG_CHECK(a.rows > 0 && a.d > 0 && a.d % 4 == 0 && a.d <= 256 * LNA_MAXV, "ln_bwd_affine: bad shape rows=%d d=%d", a.rows, a.d);
    ARG_CHECK(a.ldx % 4 == 0 && a.lddy % 4 == 0 && a.lddx % 4 == 0 && a.ldx >= a.d && a.lddy >= a.d && a.lddx >= a.d,
              "ln_bwd_affine: a row stride is shorter than d=%d or no multiple of 4 (%d/%d/%d)", a.d, a.ldx, a.lddy, a.lddx);
    ARG_CHECK(!a.dres || (a.lddres % 4 == 0 && a.lddres >= a.d), "ln_bwd_affine: bad dres stride %d", a.lddres);
    const int row_blocks = (a.rows + 3) / 4;
    hipLaunchKernelGGL(ln_bwd_affine_kernel, dim3(row_blocks + (a.d + 255) / 256), dim3(256), 0, s, a, row_blocks);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

// ---- attention over the n_ctx rows of one layer ------------------------------------------------------------------------------------------
// One wave per (sequence, head); q, k, v of the pair (L <= 16 rows of 64) live in LDS.  Scores and their gradients are computed by
// (query, key) pair -- pair t + 64 c on lane t -- the softmax by query row on lanes 0 .. L - 1, and everything with a head-dim index by
// lane = that index.  nn.MultiheadAttention scaling: q / sqrt(64) (F.multi_head_attention_forward), no mask.
constexpr int PG_LMAX = 16;
constexpr float PG_SCALE = 0.125f;

__global__ __launch_bounds__(64) void pg_attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ probs, int L, int H) {
    __shared__ float q[PG_LMAX][65], k[PG_LMAX][65], v[PG_LMAX][65], S[PG_LMAX][PG_LMAX + 1];
    const int lane = threadIdx.x, h = blockIdx.x % H, n = blockIdx.x / H;
    const size_t ld = (size_t)3 * H * 64;
    const float* base = qkv + (size_t)n * L * ld + (size_t)h * 64 + lane;
    for (int i = 0; i < L; ++i) {
        q[i][lane] = base[i * ld] * PG_SCALE;
        k[i][lane] = base[i * ld + (size_t)H * 64];
        v[i][lane] = base[i * ld + (size_t)2 * H * 64];
    }
    __syncthreads();
    for (int pr = lane; pr < L * L; pr += 64) {
        const int i = pr / L, j = pr % L;
        float acc = 0.f;
#pragma unroll 16
        for (int c = 0; c < 64; ++c) acc += q[i][c] * k[j][c];
        S[i][j] = acc;
    }
    __syncthreads();
    if (lane < L) {
        float mx = S[lane][0];
        for (int j = 1; j < L; ++j) mx = fmaxf(mx, S[lane][j]);
        float sum = 0.f;
        for (int j = 0; j < L; ++j) { const float e = expf(S[lane][j] - mx); S[lane][j] = e; sum += e; }
        const float inv = 1.f / sum;
        float* pw = probs + (((size_t)n * H + h) * L + lane) * L;
        for (int j = 0; j < L; ++j) { const float pv = S[lane][j] * inv; S[lane][j] = pv; pw[j] = pv; }
    }
    __syncthreads();
    float* o = out + (size_t)n * L * H * 64 + (size_t)h * 64 + lane;
    for (int i = 0; i < L; ++i) {
        float acc = 0.f;
        for (int j = 0; j < L; ++j) acc += S[i][j] * v[j][lane];
        o[(size_t)i * H * 64] = acc;
    }
}

__global__ __launch_bounds__(64) void pg_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ probs, const float* __restrict__ dout,
                                                         float* __restrict__ dqkv, int L, int H) {
    __shared__ float q[PG_LMAX][65], k[PG_LMAX][65], v[PG_LMAX][65], dO[PG_LMAX][65], Pm[PG_LMAX][PG_LMAX + 1], dS[PG_LMAX][PG_LMAX + 1];
    const int lane = threadIdx.x, h = blockIdx.x % H, n = blockIdx.x / H;
    const size_t ld = (size_t)3 * H * 64;
    const size_t off = (size_t)n * L * ld + (size_t)h * 64 + lane;
    const float* base = qkv + off;
    const float* dob = dout + (size_t)n * L * H * 64 + (size_t)h * 64 + lane;
    for (int i = 0; i < L; ++i) {
        q[i][lane] = base[i * ld] * PG_SCALE;
        k[i][lane] = base[i * ld + (size_t)H * 64];
        v[i][lane] = base[i * ld + (size_t)2 * H * 64];
        dO[i][lane] = dob[(size_t)i * H * 64];
    }
    const float* pb = probs + ((size_t)n * H + h) * L * L;
    for (int pr = lane; pr < L * L; pr += 64) Pm[pr / L][pr % L] = pb[pr];
    __syncthreads();
    for (int pr = lane; pr < L * L; pr += 64) {  // dP = dO V^T
        const int i = pr / L, j = pr % L;
        float acc = 0.f;
#pragma unroll 16
        for (int c = 0; c < 64; ++c) acc += dO[i][c] * v[j][c];
        dS[i][j] = acc;
    }
    __syncthreads();
    if (lane < L) {  // dS = P (dP - sum_j P dP), row by row
        float dot = 0.f;
        for (int j = 0; j < L; ++j) dot += Pm[lane][j] * dS[lane][j];
        for (int j = 0; j < L; ++j) dS[lane][j] = Pm[lane][j] * (dS[lane][j] - dot);
    }
    __syncthreads();
    float* dq = dqkv + off;
    for (int i = 0; i < L; ++i) {
        float aq = 0.f, ak = 0.f, av = 0.f;
        for (int j = 0; j < L; ++j) {
            aq += dS[i][j] * k[j][lane];   // dQ[i] = scale sum_j dS[i][j] K[j]
            ak += dS[j][i] * q[j][lane];   // dK[i] = sum_j dS[j][i] (scale Q[j]): q holds the scaled rows
            av += Pm[j][i] * dO[j][lane];  // dV[i] = sum_j P[j][i] dO[j]
        }
        dq[i * ld] = aq * PG_SCALE;
        dq[i * ld + (size_t)H * 64] = ak;
        dq[i * ld + (size_t)2 * H * 64] = av;
    }
}

static int pg_attn_check(const char* what, const void* a, const void* b, const void* c, const void* d, int N, int L, int H, int d_model) {
    ARG_CHECK(a && b && c && d, "%s: null operand", what);
    ARG_CHECK(d_model % 64 == 0 && H >= 1 && d_model == H * 64, "%s: needs H >= 1 heads of 64 (H=%d, d_t=%d: d_t %% 64 must be 0)", what, H, d_model);
    ARG_CHECK(L >= 1 && L <= PG_LMAX, "%s: L=%d outside 1..%d", what, L, PG_LMAX);
    ARG_CHECK(N >= 1 && (long long)N * H <= 0x7fffffffLL, "%s: bad batch N=%d", what, N);
    return MUDPT_OK;
}
int launch_pg_attn_fwd(const float* qkv, float* out, float* probs, int N, int L, int H, int d_model, hipStream_t s) {
    if (int r = pg_attn_check("pg_attn_fwd", qkv, out, probs, qkv, N, L, H, d_model)) return r;
    hipLaunchKernelGGL(pg_attn_fwd_kernel, dim3(N * H), dim3(64), 0, s, qkv, out, probs, L, H);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}
int launch_pg_attn_bwd(const float* qkv, const float* probs, const float* dout, float* dqkv, int N, int L, int H, int d_model, hipStream_t s) {
    if (int r = pg_attn_check("pg_attn_bwd", qkv, probs, dout, dqkv, N, L, H, d_model)) return r;
    hipLaunchKernelGGL(pg_attn_bwd_kernel, dim3(N * H), dim3(64), 0, s, qkv, probs, dout, dqkv, L, H);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

// ---- QuickGELU in fp32 (clip/model.py:173-175) --------------------------------------------------------------------------------------
// expf and an IEEE division, not the two-transcendental form of the GEMM epilogues (common.h sigmoid_1702): that one is rounded to T
// right away, this one is held to fp32 against float64 at |u| = 12, where the exponent's argument is 20 times its own rounding.
__device__ inline float pg_sigmoid(float u) { return 1.0f / (1.0f + expf(-1.702f * u)); }
__global__ __launch_bounds__(256) void quickgelu_fwd_kernel(const float* __restrict__ u, float* __restrict__ y, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = u[i] * pg_sigmoid(u[i]);
}
__global__ __launch_bounds__(256) void quickgelu_bwd_kernel(const float* dy, const float* __restrict__ u, float* du, size_t n) {  // du may be dy
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float x = u[i], sg = pg_sigmoid(x);
        du[i] = dy[i] * (sg * (1.0f + 1.702f * x * (1.0f - sg)));
    }
}
int launch_quickgelu_fwd(const float* u, float* y, size_t n, hipStream_t s) {
    ARG_CHECK(u && y && n > 0, "quickgelu_fwd: bad arguments");
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(quickgelu_fwd_kernel, dim3(grid), dim3(256), 0, s, u, y, n);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}
int launch_quickgelu_bwd(const float* dy, const float* u, float* du, size_t n, hipStream_t s) {
    ARG_CHECK(dy && u && du && n > 0, "quickgelu_bwd: bad arguments");
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(quickgelu_bwd_kernel, dim3(grid), dim3(256), 0, s, dy, u, du, n);
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

// ---- the whole generator ----------------------------------------------------------------------------------------------------------------
#define PG_TRY(expr)                    \
    do {                                \
        if (int _e = (expr)) return _e; \
    } while (0)

int pg_check_shape(const char* what, int depth, int n_ctx, int d_t, int d_v) {
    ARG_CHECK(depth >= 1, "%s: PROMPT_DEPTH should be > 0 (got %d)", what, depth);  // trainers/umudpt.py:91
    ARG_CHECK(n_ctx >= 1 && n_ctx <= PG_LMAX, "%s: n_ctx %d outside 1..%d (the generator's attention runs over the n_ctx rows of one layer)", what, n_ctx, PG_LMAX);
    ARG_CHECK(d_t >= 64 && d_t % 64 == 0 && d_t <= 1024, "%s: t_width %d must be a multiple of 64 (heads of 64: trainers/umudpt.py:122), <= 1024", what, d_t);
    ARG_CHECK(d_v >= 4 && d_v % 4 == 0, "%s: v_width %d must be a positive multiple of 4", what, d_v);
    return MUDPT_OK;
}

PgParams pg_params(const float* base, int d, int dv) {
    PgParams p;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += n; return at; };
    const size_t D = (size_t)d;
    p.off[PG_LN_PRE_G] = take(D); p.off[PG_LN_PRE_B] = take(D);
    p.off[PG_W_IN] = take(3 * D * D); p.off[PG_B_IN] = take(3 * D); p.off[PG_W_OUT] = take(D * D); p.off[PG_B_OUT] = take(D);
    p.off[PG_LN1_G] = take(D); p.off[PG_LN1_B] = take(D);
    p.off[PG_W_FC] = take(4 * D * D); p.off[PG_B_FC] = take(4 * D); p.off[PG_W_PROJ] = take(4 * D * D); p.off[PG_B_PROJ] = take(D);
    p.off[PG_LN2_G] = take(D); p.off[PG_LN2_B] = take(D); p.off[PG_LN_POST_G] = take(D); p.off[PG_LN_POST_B] = take(D);
    p.off[PG_W_VIS] = take((size_t)dv * D); p.off[PG_B_VIS] = take((size_t)dv);
    p.total = o;
    p.base = base;
    return p;
}

PgWork pg_carve(float* ws, int depth, int n_ctx, int d, size_t* numel) {
    const size_t R = (size_t)depth * n_ctx, D = (size_t)d;
    PgWork w;
    size_t o = 0;
    auto take = [&](size_t n) { float* at = ws ? ws + o : nullptr; o += n; return at; };
    w.h0 = take(R * D); w.a1 = take(R * D); w.qkv = take(3 * R * D); w.attn = take(R * D); w.o = take(R * D); w.y = take(R * D); w.a2 = take(R * D);
    w.u = take(4 * R * D); w.g = take(4 * R * D); w.p = take(R * D); w.z = take(R * D); w.a3 = take(R * D);
    w.da3 = take(R * D); w.dz = take(R * D); w.dg = take(4 * R * D); w.da2 = take(R * D); w.dy = take(R * D); w.dattn = take(R * D);
    w.dqkv = take(3 * R * D); w.da1 = take(R * D); w.dh0 = take(R * D);
    w.probs = take(R * (size_t)n_ctx * (D / 64));
    for (int i = 0; i < 4; ++i) { w.mean[i] = take(R); w.rstd[i] = take(R); }
    if (numel) *numel = o;
    return w;
}

static int pg_ln(const float* x, const float* add, float* xout, const float* gamma, const float* beta, float* out, float* mean, float* rstd, int R, int d,
                 hipStream_t s) {
    LnFwdArgs a; a.x = x; a.ldx = d; a.add = add; a.ldadd = d; a.xout = xout; a.ldxout = d; a.gamma = gamma; a.beta = beta; a.out = out; a.ldo = d;
    a.out_f32 = true; a.mean = mean; a.rstd = rstd; a.rows = R; a.d = d;
    return launch_ln_fwd(DT_F16, a, s);  // fp32 in and out: the operand type only names the (unused) T of the kernel's template
}

// G [R, dv] = visual_proj(ln_post(Block(ln_pre(X))))  (trainers/umudpt.py:170-176); sequences = the depth layers, rows of one = its n_ctx prompts
int pg_forward(int depth, int n_ctx, int d, int dv, const PgParams& P, const float* X, float* G, const PgWork& w, hipStream_t s) {
    PG_TRY(pg_check_shape("promptgen_forward", depth, n_ctx, d, dv));
    ARG_CHECK(P.base && X && G && w.h0, "promptgen_forward: null argument");
    const int R = depth * n_ctx, H = d / 64;
    PG_TRY(pg_ln(X, nullptr, nullptr, P.at(PG_LN_PRE_G), P.at(PG_LN_PRE_B), w.h0, w.mean[0], w.rstd[0], R, d, s));
    PG_TRY(pg_ln(w.h0, nullptr, nullptr, P.at(PG_LN1_G), P.at(PG_LN1_B), w.a1, w.mean[1], w.rstd[1], R, d, s));
    PG_TRY(launch_sgemm(false, true, R, 3 * d, d, 1.f, w.a1, d, P.at(PG_W_IN), d, 0.f, w.qkv, 3 * d, P.at(PG_B_IN), s));
    PG_TRY(launch_pg_attn_fwd(w.qkv, w.attn, w.probs, depth, n_ctx, H, d, s));
    PG_TRY(launch_sgemm(false, true, R, d, d, 1.f, w.attn, d, P.at(PG_W_OUT), d, 0.f, w.o, d, P.at(PG_B_OUT), s));
    // y = h0 + attention (the residual add rides on ln_2's load), a2 = ln_2(y)
    PG_TRY(pg_ln(w.h0, w.o, w.y, P.at(PG_LN2_G), P.at(PG_LN2_B), w.a2, w.mean[2], w.rstd[2], R, d, s));
    PG_TRY(launch_sgemm(false, true, R, 4 * d, d, 1.f, w.a2, d, P.at(PG_W_FC), d, 0.f, w.u, 4 * d, P.at(PG_B_FC), s));
    PG_TRY(launch_quickgelu_fwd(w.u, w.g, (size_t)R * 4 * d, s));
    PG_TRY(launch_sgemm(false, true, R, d, 4 * d, 1.f, w.g, 4 * d, P.at(PG_W_PROJ), 4 * d, 0.f, w.p, d, P.at(PG_B_PROJ), s));
    // z = y + mlp, a3 = ln_post(z)
    PG_TRY(pg_ln(w.y, w.p, w.z, P.at(PG_LN_POST_G), P.at(PG_LN_POST_B), w.a3, w.mean[3], w.rstd[3], R, d, s));
    PG_TRY(launch_sgemm(false, true, R, dv, d, 1.f, w.a3, d, P.at(PG_W_VIS), d, 0.f, G, dv, P.at(PG_B_VIS), s));
    return MUDPT_OK;
}

static int pg_ln_bwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* dy, const float* dres, float* dx, float* dgamma,
                     float* dbeta, int R, int d, hipStream_t s) {
    LnBwdAffineArgs a; a.x = x; a.ldx = d; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.dy = dy; a.lddy = d; a.dres = dres; a.lddres = d; a.dx = dx; a.lddx = d;
    a.dgamma = dgamma; a.dbeta = dbeta; a.rows = R; a.d = d;
    return launch_ln_bwd_affine(a, s);
}

// Backward of pg_forward from the activations it left in w: WRITES the 18 gradients to grads (laid out as the parameters) and dX [R, d].
int pg_backward(int depth, int n_ctx, int d, int dv, const PgParams& P, const float* X, const float* dG, float* dX, float* grads, const PgWork& w, hipStream_t s) {
    PG_TRY(pg_check_shape("promptgen_backward", depth, n_ctx, d, dv));
    ARG_CHECK(P.base && X && dG && dX && grads && w.h0, "promptgen_backward: null argument");
    const int R = depth * n_ctx, H = d / 64;
    auto g = [&](int i) { return grads + P.off[i]; };
    // a trained Linear y = x W^T + b, W [out, in]: dW = dy^T x, db = column sums of dy, dx = dy W in ONE launch_linear_bwd (elementwise.hip)
    PG_TRY(launch_linear_bwd(R, dv, d, dG, w.a3, P.at(PG_W_VIS), g(PG_W_VIS), g(PG_B_VIS), w.da3, s));
    PG_TRY(pg_ln_bwd(w.z, w.mean[3], w.rstd[3], P.at(PG_LN_POST_G), w.da3, nullptr, w.dz, g(PG_LN_POST_G), g(PG_LN_POST_B), R, d, s));
    PG_TRY(launch_linear_bwd(R, d, 4 * d, w.dz, w.g, P.at(PG_W_PROJ), g(PG_W_PROJ), g(PG_B_PROJ), w.dg, s));
    PG_TRY(launch_quickgelu_bwd(w.dg, w.u, w.dg, (size_t)R * 4 * d, s));
    PG_TRY(launch_linear_bwd(R, 4 * d, d, w.dg, w.a2, P.at(PG_W_FC), g(PG_W_FC), g(PG_B_FC), w.da2, s));
    PG_TRY(pg_ln_bwd(w.y, w.mean[2], w.rstd[2], P.at(PG_LN2_G), w.da2, w.dz, w.dy, g(PG_LN2_G), g(PG_LN2_B), R, d, s));  // + the residual branch
    PG_TRY(launch_linear_bwd(R, d, d, w.dy, w.attn, P.at(PG_W_OUT), g(PG_W_OUT), g(PG_B_OUT), w.dattn, s));
    PG_TRY(launch_pg_attn_bwd(w.qkv, w.probs, w.dattn, w.dqkv, depth, n_ctx, H, d, s));
    PG_TRY(launch_linear_bwd(R, 3 * d, d, w.dqkv, w.a1, P.at(PG_W_IN), g(PG_W_IN), g(PG_B_IN), w.da1, s));
    PG_TRY(pg_ln_bwd(w.h0, w.mean[1], w.rstd[1], P.at(PG_LN1_G), w.da1, w.dy, w.dh0, g(PG_LN1_G), g(PG_LN1_B), R, d, s));
    return pg_ln_bwd(X, w.mean[0], w.rstd[0], P.at(PG_LN_PRE_G), w.dh0, nullptr, dX, g(PG_LN_PRE_G), g(PG_LN_PRE_B), R, d, s);
}

}  // namespace mudpt
