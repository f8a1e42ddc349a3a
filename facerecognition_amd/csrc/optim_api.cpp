// C ABI of the optimiser step (include/frhip.h "Optimiser step"): the argument checks in front of optim.hip's launches
// and the cutting of the tensor list into kernel-argument tables.  Handle-free.  Every argument is checked before the
// first HIP call.
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

static_assert(sizeof(fr_optim_ctrl_head) == 64 && sizeof(fr_optim_group_state) == 64, "control block layout");
static_assert(OPTIM_MAX_GROUPS == FR_OPTIM_MAX_GROUPS, "group limit");

static bool optim_fail(const char* fn, const std::string& what) {
    set_error(std::string(fn) + ": " + what);
    return false;
}

constexpr int64_t OPTIM_MAX_NUMEL = int64_t(1) << 40;
constexpr int64_t OPTIM_MAX_CHUNKS = int64_t(1) << 24;

static size_t optim_ws_bytes(int64_t n_chunks) {
    const size_t b = (size_t)(n_chunks < 1 ? 1 : n_chunks) * sizeof(double);
    return (b + 255) & ~(size_t)255;
}

static bool optim_beta_ok(double b) { return b >= 0.0 && b < 1.0; }  // false for NaN

// The list's tensors: counts in range, pointers aligned; *chunks = the chunks of `per` elements the live ones make.
static bool optim_list_ok(const char* fn, const float* const* grads, const int64_t* numel, int n, int64_t per,
                          int64_t* chunks) {
    if (n < 0) return optim_fail(fn, "n_tensors must be >= 0");
    if (n > 0 && (!grads || !numel)) return optim_fail(fn, "null grads or numel array");
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0 || numel[i] > OPTIM_MAX_NUMEL)
            return optim_fail(fn, "numel[" + std::to_string(i) + "] must be in [0, 2^40]");
        if ((uintptr_t)grads[i] & 3) return optim_fail(fn, "grads[" + std::to_string(i) + "] must be 4-byte aligned");
        if (grads[i] && numel[i] > 0) total += (numel[i] + per - 1) / per;
    }
    if ((total * per) / FR_OPTIM_CHUNK > OPTIM_MAX_CHUNKS) return optim_fail(fn, "more than 2^24 chunks in one call");
    *chunks = total;
    return true;
}

}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_optim_workspace(int64_t n_chunks) {
    if (n_chunks < 0 || n_chunks > OPTIM_MAX_CHUNKS) {
        optim_fail("fr_optim_workspace", "n_chunks must be in [0, 2^24]");
        return 0;
    }
    return optim_ws_bytes(n_chunks);
}

int fr_optim_grad_norm(const float* const* grads, const int64_t* numel, int n_tensors, double max_norm, int flags,
                       const float* found_inf, const float* grad_scale, int n_groups, const double* beta1,
                       const double* beta2, int64_t attempt, void* ctrl, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "fr_optim_grad_norm";
    int64_t n_chunks = 0;
    if (!optim_list_ok(fn, grads, numel, n_tensors, FR_OPTIM_CHUNK, &n_chunks)) return FR_ERR_ARG;
    if (std::isnan(max_norm)) { optim_fail(fn, "max_norm must not be NaN"); return FR_ERR_ARG; }
    if (flags & ~FR_OPTIM_SKIP_NONFINITE) { optim_fail(fn, "unknown flag bits"); return FR_ERR_ARG; }
    if (n_groups < 0 || n_groups > FR_OPTIM_MAX_GROUPS) {
        optim_fail(fn, "n_groups must be in [0, 32]");
        return FR_ERR_ARG;
    }
    if (n_groups > 0 && (!beta1 || !beta2)) { optim_fail(fn, "null beta1 or beta2 array"); return FR_ERR_ARG; }
    for (int g = 0; g < n_groups; ++g)
        if (!optim_beta_ok(beta1[g]) || !optim_beta_ok(beta2[g])) {
            optim_fail(fn, "betas of group " + std::to_string(g) + " must be in [0, 1)");
            return FR_ERR_ARG;
        }
    if (attempt < 1) { optim_fail(fn, "attempt must be >= 1"); return FR_ERR_ARG; }
    if (!ctrl || !ws) { optim_fail(fn, "null ctrl or ws"); return FR_ERR_ARG; }
    if (((uintptr_t)ctrl & 7) || ((uintptr_t)ws & 7)) { optim_fail(fn, "ctrl and ws must be 8-byte aligned"); return FR_ERR_ARG; }
    if (((uintptr_t)found_inf & 3) || ((uintptr_t)grad_scale & 3)) {
        optim_fail(fn, "found_inf and grad_scale must be 4-byte aligned");
        return FR_ERR_ARG;
    }
    if (ws_bytes < optim_ws_bytes(n_chunks)) {
        optim_fail(fn, "workspace smaller than fr_optim_workspace(n_chunks)");
        return FR_ERR_ARG;
    }

    hipStream_t s = (hipStream_t)stream;
    double* partials = (double*)ws;
    OptimNormTable t = {};
    int64_t chunk_base = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (grads[i] && numel[i] > 0) {
            t.g[t.n] = grads[i];
            t.numel[t.n] = numel[i];
            t.chunk0[t.n + 1] = t.chunk0[t.n] + (int32_t)((numel[i] + FR_OPTIM_CHUNK - 1) / FR_OPTIM_CHUNK);
            ++t.n;
        }
        if (t.n == OPTIM_NORM_TENSORS || (i == n_tensors - 1 && t.n > 0)) {
            FR_HIP_CHECK(launch_optim_sumsq(t, chunk_base, grad_scale, partials, s));
            chunk_base += t.chunk0[t.n];
            t = OptimNormTable{};
        }
    }
    OptimGroupBetas b = {};
    b.n = n_groups;
    for (int g = 0; g < n_groups; ++g) { b.beta1[g] = beta1[g]; b.beta2[g] = beta2[g]; }
    const float mn = max_norm > 0.0 ? (float)max_norm : 0.f;
    FR_HIP_CHECK(launch_optim_norm_finish(partials, n_chunks, mn, (flags & FR_OPTIM_SKIP_NONFINITE) != 0, found_inf, b,
                                          attempt, ctrl, s));
    return FR_OK;
}

int fr_optim_step(int kind, float* const* params, const float* const* grads, float* const* state1, float* const* state2,
                  const int64_t* numel, const int64_t* born, int n_tensors, double lr, double weight_decay,
                  double momentum, double dampening, double beta1, double beta2, double eps, int flags, const void* ctrl,
                  int group, const float* grad_scale, void* stream) {
    const char* fn = "fr_optim_step";
    if (kind != FR_OPTIM_SGD && kind != FR_OPTIM_ADAM && kind != FR_OPTIM_ADAMW) {
        optim_fail(fn, "kind must be FR_OPTIM_SGD, FR_OPTIM_ADAM or FR_OPTIM_ADAMW");
        return FR_ERR_ARG;
    }
    if (flags & FR_OPTIM_AMSGRAD) { optim_fail(fn, "amsgrad is not supported"); return FR_ERR_ARG; }
    if (flags & ~(FR_OPTIM_NESTEROV | FR_OPTIM_MAXIMIZE)) { optim_fail(fn, "unknown flag bits"); return FR_ERR_ARG; }
    const bool adam = kind != FR_OPTIM_SGD;
    if (!(lr >= 0.0) || !std::isfinite(lr)) { optim_fail(fn, "lr must be finite and >= 0"); return FR_ERR_ARG; }
    if (!(weight_decay >= 0.0) || !std::isfinite(weight_decay)) {
        optim_fail(fn, "weight_decay must be finite and >= 0");
        return FR_ERR_ARG;
    }
    if (adam) {
        if (!(eps >= 0.0) || !std::isfinite(eps)) { optim_fail(fn, "eps must be finite and >= 0"); return FR_ERR_ARG; }
        if (!optim_beta_ok(beta1) || !optim_beta_ok(beta2)) { optim_fail(fn, "betas must be in [0, 1)"); return FR_ERR_ARG; }
        if (flags & FR_OPTIM_NESTEROV) { optim_fail(fn, "FR_OPTIM_NESTEROV belongs to FR_OPTIM_SGD"); return FR_ERR_ARG; }
    } else {
        if (!(momentum >= 0.0) || !std::isfinite(momentum)) {
            optim_fail(fn, "momentum must be finite and >= 0");
            return FR_ERR_ARG;
        }
        if (!std::isfinite(dampening)) { optim_fail(fn, "dampening must be finite"); return FR_ERR_ARG; }
        if ((flags & FR_OPTIM_NESTEROV) && (!(momentum > 0.0) || dampening != 0.0)) {
            optim_fail(fn, "nesterov needs momentum > 0 and dampening = 0");
            return FR_ERR_ARG;
        }
    }
    int64_t n_chunks = 0;
    if (!optim_list_ok(fn, grads, numel, n_tensors, FR_OPTIM_STEP_CHUNK, &n_chunks)) return FR_ERR_ARG;
    if (n_tensors > 0 && !params) { optim_fail(fn, "null params array"); return FR_ERR_ARG; }
    const bool need1 = adam || momentum != 0.0, need2 = adam;
    if (n_tensors > 0 && ((need1 && !state1) || (need2 && !state2))) {
        optim_fail(fn, "null state array (state1: momentum_buffer / exp_avg, state2: exp_avg_sq)");
        return FR_ERR_ARG;
    }
    for (int i = 0; i < n_tensors; ++i) {
        if (!grads[i] || numel[i] == 0) continue;
        const std::string at = "[" + std::to_string(i) + "]";
        if (!params[i] || ((uintptr_t)params[i] & 3)) {
            optim_fail(fn, "params" + at + " must be non-null and 4-byte aligned");
            return FR_ERR_ARG;
        }
        if (need1 && (!state1[i] || ((uintptr_t)state1[i] & 3))) {
            optim_fail(fn, "state1" + at + " must be non-null and 4-byte aligned");
            return FR_ERR_ARG;
        }
        if (need2 && (!state2[i] || ((uintptr_t)state2[i] & 3))) {
            optim_fail(fn, "state2" + at + " must be non-null and 4-byte aligned");
            return FR_ERR_ARG;
        }
        if (born && born[i] < 0) { optim_fail(fn, "born" + at + " must be >= 0"); return FR_ERR_ARG; }
    }
    if (group < 0 || group >= FR_OPTIM_MAX_GROUPS) { optim_fail(fn, "group must be in [0, 32)"); return FR_ERR_ARG; }
    if (!ctrl || ((uintptr_t)ctrl & 7)) { optim_fail(fn, "ctrl must be non-null and 8-byte aligned"); return FR_ERR_ARG; }
    if ((uintptr_t)grad_scale & 3) { optim_fail(fn, "grad_scale must be 4-byte aligned"); return FR_ERR_ARG; }

    OptimHyper h = {lr, weight_decay, momentum, dampening, beta1, beta2, eps, flags};
    hipStream_t s = (hipStream_t)stream;
    OptimStepTable t = {};
    for (int i = 0; i < n_tensors; ++i) {
        if (grads[i] && numel[i] > 0) {
            t.p[t.n] = params[i];
            t.g[t.n] = grads[i];
            t.s1[t.n] = need1 ? state1[i] : nullptr;
            t.s2[t.n] = need2 ? state2[i] : nullptr;
            t.numel[t.n] = numel[i];
            t.born[t.n] = born ? born[i] : 0;
            t.chunk0[t.n + 1] = t.chunk0[t.n] + (int32_t)((numel[i] + FR_OPTIM_STEP_CHUNK - 1) / FR_OPTIM_STEP_CHUNK);
            ++t.n;
        }
        if (t.n == OPTIM_STEP_TENSORS || (i == n_tensors - 1 && t.n > 0)) {
            FR_HIP_CHECK(launch_optim_step(kind, t, h, ctrl, group, grad_scale, s));
            t = OptimStepTable{};
        }
    }
    return FR_OK;
}

}  // extern "C"
