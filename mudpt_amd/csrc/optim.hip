// The fused optimizer step: Adam, AMSGrad, AdamW and RMSprop over one flat fp32 bucket in ONE launch (trainers/mudpt.py:251
// model_backward_and_update's optimizer step for every OPTIM.NAME but "sgd", which keeps launch_sgd).  torch.optim's default path is a
// chain of foreach launches per step; here p[n] is read and written, g[n] read and up to three state buffers s0 / s1 / s2 [n] read and
// written once each (Adam: 28 bytes per element).
//
// The update rules are those of torch 2.10's single-tensor paths, statement by statement, in fp32:
//   torch/optim/adam.py::_single_tensor_adam, the non-capturable branch (:414-430, :457-476, :528-546)
//     :419  AdamW     param.mul_(1 - lr * weight_decay)                          (decoupled decay)
//     :429  Adam      grad = grad.add(param, alpha=weight_decay)                 (L2 decay)
//     :457            exp_avg.lerp_(grad, 1 - beta1)                             (ATen's lerp: w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w))
//     :476            exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//     :530-535        bias_correction1 = 1 - beta1**step, bias_correction2 = 1 - beta2**step, step_size = lr / bias_correction1,
//                     bias_correction2_sqrt = bias_correction2**0.5              (Python floats: computed HERE on the host, in double)
//     :539  amsgrad   torch.maximum(max_exp_avg_sq, exp_avg_sq, out=max_exp_avg_sq)   (a NaN in either operand is kept)
//     :542-544        denom = (sqrt(v) / bias_correction2_sqrt).add_(eps), v = max_exp_avg_sq under amsgrad, else exp_avg_sq
//     :546            param.addcdiv_(exp_avg, denom, value=-step_size)
//   torch/optim/rmsprop.py::_single_tensor_rmsprop (:305-339)
//     :308            grad = grad.add(param, alpha=weight_decay)
//     :316            square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
//     :322-323 centered   grad_avg.lerp_(grad, 1 - alpha); avg = square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_()
//     :325            avg = square_avg.sqrt()
//     :330            avg = avg.add_(eps)
//     :336-337 momentum > 0   buf.mul_(momentum).addcdiv_(grad, avg); param.add_(buf, alpha=-lr)
//     :339            param.addcdiv_(grad, avg, value=-lr)
// State slots: Adam / AdamW s0 = exp_avg, s1 = exp_avg_sq, s2 = max_exp_avg_sq (amsgrad); RMSprop s0 = square_avg, s1 = momentum_buffer
// (momentum > 0), s2 = grad_avg (centered); SGD s0 = momentum_buffer (momentum != 0).
//
// Every scalar that depends on `step` or on a difference of hyper-parameters is computed on the host in double, as torch's Python does, and
// rounded to fp32 ONCE (1 - 0.999f is 1.3e-5 off 0.001: the hyper-parameters therefore arrive as doubles); the device never calls powf.
// Square root and division are the correctly rounded ones (the compiler's default for HIP): the kernel is memory-bound, they cost nothing.
// The kernel has no LDS, no atomics and no cross-lane traffic: element i of every buffer depends on element i of the others alone.
#include "kernels.h"

#include <cmath>

namespace mudpt {

struct OptimConsts {
    float wd;         // weight_decay
    float decay;      // AdamW: 1 - lr * weight_decay
    float w1;         // Adam: 1 - beta1 (lerp weight of exp_avg); RMSprop: 1 - alpha (lerp weight of grad_avg)
    float b2, omb2;   // Adam: beta2, 1 - beta2; RMSprop: alpha, 1 - alpha
    float bc2_sqrt;   // Adam: sqrt(1 - beta2^step)
    float neg_step;   // Adam: -lr / (1 - beta1^step); RMSprop: -lr
    float eps;
    float momentum;   // RMSprop
};

enum : int { OPT_AMSGRAD = 1, OPT_DECOUPLED = 2, OPT_CENTERED = 1, OPT_MOMENTUM = 2 };

__device__ __forceinline__ float lerp_f32(float a, float b, float w) {  // ATen/native/Lerp.h
    const float d = b - a;
    return w < 0.5f ? a + w * d : b - d * (1.f - w);
}

// One element of the Adam family.  FLAGS: OPT_AMSGRAD, OPT_DECOUPLED (AdamW)
template <int FLAGS>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vmax, const OptimConsts& c) {
    if (c.wd != 0.f) {
        if (FLAGS & OPT_DECOUPLED) p *= c.decay;
        else g = g + c.wd * p;
    }
    m = lerp_f32(m, g, c.w1);
    v = v * c.b2 + c.omb2 * g * g;
    float u = v;
    if (FLAGS & OPT_AMSGRAD) {
        vmax = (v > vmax || v != v) ? v : vmax;  // torch.maximum: a NaN on either side stays
        u = vmax;
    }
    const float denom = sqrtf(u) / c.bc2_sqrt + c.eps;
    p = p + c.neg_step * (m / denom);
}

// One element of RMSprop.  FLAGS: OPT_CENTERED, OPT_MOMENTUM
template <int FLAGS>
__device__ __forceinline__ void rmsprop_elem(float& p, float g, float& sq, float& buf, float& gavg, const OptimConsts& c) {
    if (c.wd != 0.f) g = g + c.wd * p;
    sq = sq * c.b2 + c.omb2 * g * g;
    float avg;
    if (FLAGS & OPT_CENTERED) {
        gavg = lerp_f32(gavg, g, c.w1);
        avg = sqrtf(sq + -1.f * gavg * gavg);
    } else {
        avg = sqrtf(sq);
    }
    avg += c.eps;
    if (FLAGS & OPT_MOMENTUM) {
        buf = buf * c.momentum + g / avg;
        p = p + c.neg_step * buf;
    } else {
        p = p + c.neg_step * (g / avg);
    }
}

template <bool ADAM, int FLAGS>
__device__ __forceinline__ void optim_elem(float& p, float g, float& s0, float& s1, float& s2, const OptimConsts& c) {
    if (ADAM) adam_elem<FLAGS>(p, g, s0, s1, s2, c);
    else rmsprop_elem<FLAGS>(p, g, s0, s1, s2, c);
}

// 16 bytes per lane and access, a grid-stride loop over the n / 4 whole vectors; the last n % 4 elements in scalar form by the first
// lanes of block 0.  A state slot the instantiation does not use is never dereferenced (its pointer may be null).
template <bool ADAM, int FLAGS>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                                                    float* __restrict__ s2, size_t n, OptimConsts c) {
    constexpr bool use1 = ADAM || (FLAGS & OPT_MOMENTUM), use2 = ADAM ? (FLAGS & OPT_AMSGRAD) != 0 : (FLAGS & OPT_CENTERED) != 0;
    const size_t n4 = n / 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        f32x4 pv = ((f32x4*)p)[i];
        const f32x4 gv = ((const f32x4*)g)[i];
        f32x4 a = ((f32x4*)s0)[i], b = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
        if (use1) b = ((f32x4*)s1)[i];
        if (use2) d = ((f32x4*)s2)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pe = pv[k], ae = a[k], be = b[k], de = d[k];
            optim_elem<ADAM, FLAGS>(pe, gv[k], ae, be, de, c);
            pv[k] = pe; a[k] = ae; b[k] = be; d[k] = de;
        }
        ((f32x4*)p)[i] = pv;
        ((f32x4*)s0)[i] = a;
        if (use1) ((f32x4*)s1)[i] = b;
        if (use2) ((f32x4*)s2)[i] = d;
    }
    const size_t t = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < n) {
        float pe = p[t], ae = s0[t], be = use1 ? s1[t] : 0.f, de = use2 ? s2[t] : 0.f;
        optim_elem<ADAM, FLAGS>(pe, g[t], ae, be, de, c);
        p[t] = pe;
        s0[t] = ae;
        if (use1) s1[t] = be;
        if (use2) s2[t] = de;
    }
}

template <bool ADAM, int FLAGS>
static void launch_form(const OptimArgs& a, const OptimConsts& c, hipStream_t s) {
    const size_t n = (size_t)a.n, blocks = (n / 4 + 255) / 256;
    const int grid = (int)(blocks < 1 ? 1 : blocks < 2048 ? blocks : 2048);
    hipLaunchKernelGGL((optim_kernel<ADAM, FLAGS>), dim3(grid), dim3(256), 0, s, a.p, a.g, a.state[0], a.state[1], a.state[2], n, c);
}

int launch_optim(const OptimArgs& a, hipStream_t s) {
    static const char* const ALGO[4] = {"sgd", "adam", "adamw", "rmsprop"};
    ARG_CHECK(a.algo >= MUDPT_OPTIM_SGD && a.algo <= MUDPT_OPTIM_RMSPROP, "optim: unknown algo %d", a.algo);
    const bool adam = a.algo == MUDPT_OPTIM_ADAM || a.algo == MUDPT_OPTIM_ADAMW, rms = a.algo == MUDPT_OPTIM_RMSPROP;
    ARG_CHECK(a.p && a.g, "optim: null parameters / gradients");
    ARG_CHECK(a.n >= 1, "optim: n = %lld must be >= 1", (long long)a.n);
    ARG_CHECK(a.step >= 1, "optim: step = %lld is the 1-based count of this update, it must be >= 1", (long long)a.step);
    ARG_CHECK(a.lr >= 0.0 && std::isfinite(a.lr) && a.weight_decay >= 0.0 && std::isfinite(a.weight_decay), "optim: lr %g / weight_decay %g must be finite and >= 0",
              a.lr, a.weight_decay);
    if (adam || rms) ARG_CHECK(a.eps > 0.0 && std::isfinite(a.eps), "optim: eps = %g must be > 0 (it alone keeps a zero second moment from dividing by zero)", a.eps);
    if (adam) ARG_CHECK(a.beta1 >= 0.0 && a.beta1 < 1.0 && a.beta2 >= 0.0 && a.beta2 < 1.0, "optim: beta1 %g / beta2 %g must lie in [0, 1)", a.beta1, a.beta2);
    if (rms) ARG_CHECK(a.alpha >= 0.0 && std::isfinite(a.alpha) && a.momentum >= 0.0 && std::isfinite(a.momentum), "optim: alpha %g / momentum %g must be finite and >= 0",
                       a.alpha, a.momentum);
    // the buffers this algorithm and these flags touch: p, g and the state slots listed in the header
    const bool need[3] = {adam || rms || a.momentum != 0.0, adam || (rms && a.momentum > 0.0), adam ? a.amsgrad : (rms && a.centered)};
    static const char* const SLOT[4][3] = {{"momentum_buffer", "", ""}, {"exp_avg", "exp_avg_sq", "max_exp_avg_sq"}, {"exp_avg", "exp_avg_sq", "max_exp_avg_sq"},
                                           {"square_avg", "momentum_buffer", "grad_avg"}};
    struct { const float* ptr; const char* name; } buf[5] = {{a.p, "p"}, {a.g, "g"}};
    int nbuf = 2;
    for (int k = 0; k < 3; ++k) {
        if (!need[k]) continue;
        ARG_CHECK(a.state[k], "optim: %s needs state[%d] (%s), which is null", ALGO[a.algo], k, SLOT[a.algo][k]);
        buf[nbuf].ptr = a.state[k];
        buf[nbuf++].name = SLOT[a.algo][k];
    }
    const uintptr_t bytes = (uintptr_t)a.n * 4;
    for (int i = 0; i < nbuf; ++i) {
        ARG_CHECK(a.algo == MUDPT_OPTIM_SGD || (uintptr_t)buf[i].ptr % 16 == 0, "optim: %s is not 16-byte aligned", buf[i].name);
        for (int j = 0; j < i; ++j)
            ARG_CHECK((uintptr_t)buf[i].ptr >= (uintptr_t)buf[j].ptr + bytes || (uintptr_t)buf[j].ptr >= (uintptr_t)buf[i].ptr + bytes, "optim: %s overlaps %s", buf[i].name,
                      buf[j].name);
    }
    if (a.algo == MUDPT_OPTIM_SGD)
        return launch_sgd(a.p, a.g, need[0] ? a.state[0] : nullptr, (size_t)a.n, (float)a.lr, (float)a.momentum, (float)a.weight_decay, (float)a.dampening, a.nesterov,
                          a.step == 1, s);
    OptimConsts c = {};
    c.wd = (float)a.weight_decay;
    c.eps = (float)a.eps;
    if (adam) {
        const double bc1 = 1.0 - std::pow(a.beta1, (double)a.step), bc2 = 1.0 - std::pow(a.beta2, (double)a.step);
        c.decay = (float)(1.0 - a.lr * a.weight_decay);
        c.w1 = (float)(1.0 - a.beta1);
        c.b2 = (float)a.beta2;
        c.omb2 = (float)(1.0 - a.beta2);
        c.bc2_sqrt = (float)std::sqrt(bc2);
        c.neg_step = (float)-(a.lr / bc1);
        const int flags = (a.amsgrad ? OPT_AMSGRAD : 0) | (a.algo == MUDPT_OPTIM_ADAMW ? OPT_DECOUPLED : 0);
        switch (flags) {
            case 0: launch_form<true, 0>(a, c, s); break;
            case 1: launch_form<true, 1>(a, c, s); break;
            case 2: launch_form<true, 2>(a, c, s); break;
            default: launch_form<true, 3>(a, c, s); break;
        }
    } else {
        c.w1 = c.omb2 = (float)(1.0 - a.alpha);
        c.b2 = (float)a.alpha;
        c.neg_step = (float)-a.lr;
        c.momentum = (float)a.momentum;
        const int flags = (a.centered ? OPT_CENTERED : 0) | (a.momentum > 0.0 ? OPT_MOMENTUM : 0);
        switch (flags) {
            case 0: launch_form<false, 0>(a, c, s); break;
            case 1: launch_form<false, 1>(a, c, s); break;
            case 2: launch_form<false, 2>(a, c, s); break;
            default: launch_form<false, 3>(a, c, s); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return MUDPT_OK;
}

}  // namespace mudpt
