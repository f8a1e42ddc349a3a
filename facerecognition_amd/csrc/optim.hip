// Optimiser step (include/frhip.h "Optimiser step"; DESIGN.md §4 "Optimiser step and training loop"): the global L2
// norm of a list of f32 gradients, torch's clip coefficient, and one SGD / Adam / AdamW update pass, with the tensor
// table in the kernel arguments.  Built with -ffp-contract=off: every product below is rounded before it is added, as
// torch's single-tensor formulas (and tests/optim_ref.py) round them; sqrt and / are the correctly rounded ones.
//
// Determinism: a gradient is cut into chunks of FR_OPTIM_CHUNK elements counted from its first element.  Inside a
// chunk, thread t of 256 owns the elements 1024 k + 4 t .. + 3 (k = 0 .. 63) and adds their squares in that order; the
// 256 thread sums meet in a fixed binary tree in LDS.  The sum of chunk c lands in partials[c], c counted over the whole
// tensor list, and one workgroup adds the partials (thread t takes t, t + 256, ... in order, then the same tree).  Which
// launch a tensor travels in, how a pointer is aligned and how large the workspace is change none of these orders.
// The squares and all sums are double: the square of a float is exact in double.
#include <hip/hip_runtime.h>

#include "../../include/frhip.h"
#include "kernels.h"

namespace fr {

namespace {

constexpr int THREADS = 256;
constexpr int VEC_STRIDE = THREADS * 4;  // elements one sweep of the workgroup covers

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The tensor of this launch that owns chunk c (chunk0 is an exclusive prefix sum; all lanes agree).
template <int N>
__device__ __forceinline__ int find_tensor(const int32_t (&chunk0)[N], int n, int c) {
    int i = 0;
    while (i + 1 < n && chunk0[i + 1] <= c) ++i;
    return i;
}

__device__ __forceinline__ double tree256(double v, double* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

__device__ __forceinline__ void load4(const float* p, int64_t e, int64_t n, bool vec, float (&x)[4]) {
    if (e + 3 < n) {
        if (vec) {
            const float4 v = *reinterpret_cast<const float4*>(p + e);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            x[0] = p[e]; x[1] = p[e + 1]; x[2] = p[e + 2]; x[3] = p[e + 3];
        }
    } else {
        for (int j = 0; j < 4; ++j) x[j] = e + j < n ? p[e + j] : 0.f;
    }
}

__device__ __forceinline__ void store4(float* p, int64_t e, int64_t n, bool vec, const float (&x)[4]) {
    if (e + 3 < n) {
        if (vec) {
            *reinterpret_cast<float4*>(p + e) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
            p[e] = x[0]; p[e + 1] = x[1]; p[e + 2] = x[2]; p[e + 3] = x[3];
        }
    } else {
        for (int j = 0; j < 4; ++j)
            if (e + j < n) p[e + j] = x[j];
    }
}

__global__ __launch_bounds__(THREADS) void optim_sumsq_kernel(OptimNormTable t, int64_t chunk_base,
                                                              const float* __restrict__ grad_scale,
                                                              double* __restrict__ partials) {
    __shared__ double lds[THREADS];
    const int c = blockIdx.x;
    const int i = find_tensor(t.chunk0, t.n, c);
    const float* g = t.g[i];
    const int64_t n = t.numel[i];
    const int64_t base = (int64_t)(c - t.chunk0[i]) * FR_OPTIM_CHUNK;
    const bool vec = aligned16(g);
    const bool scaled = grad_scale != nullptr;
    const float scale = scaled ? *grad_scale : 1.f;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < FR_OPTIM_CHUNK / VEC_STRIDE; ++k) {
        const int64_t e = base + (int64_t)k * VEC_STRIDE + threadIdx.x * 4;
        if (e >= n) break;
        float x[4];
        load4(g, e, n, vec, x);
        for (int j = 0; j < 4; ++j) {
            const float v = scaled ? x[j] / scale : x[j];
            acc = acc + (double)v * (double)v;
        }
    }
    const double sum = tree256(acc, lds);
    if (threadIdx.x == 0) partials[chunk_base + c] = sum;
}

__global__ __launch_bounds__(THREADS) void optim_norm_finish_kernel(const double* __restrict__ partials, int64_t n_chunks,
                                                                    float max_norm, int skip_nonfinite,
                                                                    const float* __restrict__ found_inf,
                                                                    OptimGroupBetas betas, int64_t attempt,
                                                                    char* __restrict__ ctrl) {
    __shared__ double lds[THREADS];
    __shared__ int skip_s;
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < n_chunks; c += THREADS) acc = acc + partials[c];
    const double total = tree256(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        float clip = 1.f;
        if (max_norm > 0.f) {
            const float c = max_norm / (norm + 1e-6f);
            clip = c > 1.f ? 1.f : c;  // a NaN norm stays NaN, as torch's clamp(max=1) leaves it
        }
        int skip = 0;
        if (found_inf != nullptr && *found_inf != 0.f) skip = 1;
        if (skip_nonfinite && !(fabsf(norm) <= 3.402823466e38f)) skip = 1;
        fr_optim_ctrl_head* h = reinterpret_cast<fr_optim_ctrl_head*>(ctrl);
        h->norm = norm;
        h->clip = clip;
        h->skip = skip;
        skip_s = skip;
    }
    __syncthreads();
    if (!skip_s && (int)threadIdx.x < betas.n) {
        fr_optim_group_state* s = reinterpret_cast<fr_optim_group_state*>(ctrl + sizeof(fr_optim_ctrl_head)) + threadIdx.x;
        s->step = s->step + 1.0;
        s->beta1_pow = s->beta1_pow * betas.beta1[threadIdx.x];
        s->beta2_pow = s->beta2_pow * betas.beta2[threadIdx.x];
        s->prev_ok = s->last_ok;
        s->last_ok = attempt;
    }
}

// The f32 constants of one update, as torch casts its Python doubles when a kernel takes them.
struct StepConst {
    float wd, mom, one_minus_damp, neg_lr;                              // SGD
    float w, one_minus_w, beta2, one_minus_beta2, neg_step, bc2_sqrt, eps, decay;  // Adam / AdamW
    bool has_wd, has_mom, nesterov, maximize;
};

template <int KIND>
__device__ __forceinline__ void update1(const StepConst& k, bool init, float& p, float g, float& s1, float& s2) {
    if (k.maximize) g = -g;
    if (KIND == FR_OPTIM_SGD) {
        if (k.has_wd) g = g + k.wd * p;
        if (k.has_mom) {
            s1 = init ? g : s1 * k.mom + k.one_minus_damp * g;
            g = k.nesterov ? g + k.mom * s1 : s1;
        }
        p = p + k.neg_lr * g;
    } else {
        if (k.has_wd) {
            if (KIND == FR_OPTIM_ADAMW) p = p * k.decay;
            else g = g + k.wd * p;
        }
        const float diff = g - s1;
        s1 = k.w < 0.5f ? s1 + k.w * diff : g - diff * k.one_minus_w;  // torch's lerp
        s2 = s2 * k.beta2 + (k.one_minus_beta2 * g) * g;
        const float denom = __builtin_sqrtf(s2) / k.bc2_sqrt + k.eps;
        p = p + (k.neg_step * s1) / denom;
    }
}

template <int KIND>
__global__ __launch_bounds__(THREADS) void optim_step_kernel(OptimStepTable t, OptimHyper h, const char* __restrict__ ctrl,
                                                             int group, const float* __restrict__ grad_scale) {
    const fr_optim_ctrl_head* head = reinterpret_cast<const fr_optim_ctrl_head*>(ctrl);
    if (head->skip) return;
    const fr_optim_group_state* gs =
        reinterpret_cast<const fr_optim_group_state*>(ctrl + sizeof(fr_optim_ctrl_head)) + group;
    StepConst k = {};
    k.has_wd = h.weight_decay != 0.0;
    k.wd = (float)h.weight_decay;
    k.maximize = (h.flags & FR_OPTIM_MAXIMIZE) != 0;
    if (KIND == FR_OPTIM_SGD) {
        k.has_mom = h.momentum != 0.0;
        k.mom = (float)h.momentum;
        k.one_minus_damp = (float)(1.0 - h.dampening);
        k.neg_lr = (float)(-h.lr);
        k.nesterov = (h.flags & FR_OPTIM_NESTEROV) != 0;
    } else {
        k.w = (float)(1.0 - h.beta1);
        k.one_minus_w = 1.f - k.w;
        k.beta2 = (float)h.beta2;
        k.one_minus_beta2 = (float)(1.0 - h.beta2);
        const double bc1 = 1.0 - gs->beta1_pow;
        const double bc2 = 1.0 - gs->beta2_pow;
        k.neg_step = (float)(-(h.lr / bc1));
        k.bc2_sqrt = (float)sqrt(bc2);
        k.eps = (float)h.eps;
        const double lw = h.lr * h.weight_decay;
        k.decay = (float)(1.0 - lw);
    }
    const float clip = head->clip;
    const bool scaled = grad_scale != nullptr;
    const float scale = scaled ? *grad_scale : 1.f;

    const int c = blockIdx.x;
    const int i = find_tensor(t.chunk0, t.n, c);
    float* p = t.p[i];
    const float* g = t.g[i];
    float* s1 = t.s1[i];
    float* s2 = t.s2[i];
    const int64_t n = t.numel[i];
    // the momentum buffer starts as the gradient in the first applied step since this tensor's state was created
    const bool init = KIND == FR_OPTIM_SGD && gs->prev_ok < t.born[i];
    const bool use1 = KIND != FR_OPTIM_SGD || k.has_mom;
    const bool use2 = KIND != FR_OPTIM_SGD;
    // 16-byte accesses per pointer: a view at a storage offset (4-byte aligned only) does not slow its neighbours down
    const bool vp = aligned16(p), vg = aligned16(g), v1 = aligned16(s1), v2 = aligned16(s2);
    const int64_t base = (int64_t)(c - t.chunk0[i]) * FR_OPTIM_STEP_CHUNK;
#pragma unroll 2
    for (int it = 0; it < FR_OPTIM_STEP_CHUNK / VEC_STRIDE; ++it) {
        const int64_t e = base + (int64_t)it * VEC_STRIDE + threadIdx.x * 4;
        if (e >= n) break;
        float pv[4], gv[4], av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
        load4(p, e, n, vp, pv);
        load4(g, e, n, vg, gv);
        if (use1 && !init) load4(s1, e, n, v1, av);
        if (use2) load4(s2, e, n, v2, bv);
        for (int j = 0; j < 4; ++j) {
            float x = scaled ? gv[j] / scale : gv[j];
            x = x * clip;
            update1<KIND>(k, init, pv[j], x, av[j], bv[j]);
        }
        store4(p, e, n, vp, pv);
        if (use1) store4(s1, e, n, v1, av);
        if (use2) store4(s2, e, n, v2, bv);
    }
}

}  // namespace

hipError_t launch_optim_sumsq(const OptimNormTable& t, int64_t chunk_base, const float* grad_scale, double* partials,
                              hipStream_t s) {
    const int chunks = t.chunk0[t.n];
    if (chunks <= 0) return hipSuccess;
    optim_sumsq_kernel<<<dim3(chunks), dim3(THREADS), 0, s>>>(t, chunk_base, grad_scale, partials);
    return hipGetLastError();
}

hipError_t launch_optim_norm_finish(const double* partials, int64_t n_chunks, float max_norm, bool skip_nonfinite,
                                    const float* found_inf, const OptimGroupBetas& betas, int64_t attempt, void* ctrl,
                                    hipStream_t s) {
    optim_norm_finish_kernel<<<dim3(1), dim3(THREADS), 0, s>>>(partials, n_chunks, max_norm, skip_nonfinite ? 1 : 0,
                                                              found_inf, betas, attempt, (char*)ctrl);
    return hipGetLastError();
}

hipError_t launch_optim_step(int kind, const OptimStepTable& t, const OptimHyper& h, const void* ctrl, int group,
                             const float* grad_scale, hipStream_t s) {
    const int chunks = t.chunk0[t.n];
    if (chunks <= 0) return hipSuccess;
    const dim3 grid(chunks), block(THREADS);
    const char* c = (const char*)ctrl;
    if (kind == FR_OPTIM_SGD) optim_step_kernel<FR_OPTIM_SGD><<<grid, block, 0, s>>>(t, h, c, group, grad_scale);
    else if (kind == FR_OPTIM_ADAM) optim_step_kernel<FR_OPTIM_ADAM><<<grid, block, 0, s>>>(t, h, c, group, grad_scale);
    else optim_step_kernel<FR_OPTIM_ADAMW><<<grid, block, 0, s>>>(t, h, c, group, grad_scale);
    return hipGetLastError();
}

}  // namespace fr
