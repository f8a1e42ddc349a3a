// C ABI of head training (include/frhip.h "Head training"): the argument checks in front of head_train.hip's
// launches.  Handle-free, like the fr_arcmargin_* ops.  Every argument is checked before the first HIP call.
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

static bool head_fail(const char* fn, const char* what) {
    set_error(std::string(fn) + ": " + what);
    return false;
}

static bool head_shape_ok(const char* fn, int B, int K, int N) {
    constexpr int64_t LIM = int64_t(1) << 40;
    constexpr int DIM = 65535 * 64;  // a launch grid's second dimension holds 65535 tiles of 64
    if (B < 1) return head_fail(fn, "B must be at least 1");
    if (K < 4 || K % 4 != 0) return head_fail(fn, "K must be a positive multiple of 4");
    if (N < 4 || N % 4 != 0) return head_fail(fn, "N must be a positive multiple of 4");
    if ((int64_t)B * K > LIM) return head_fail(fn, "B * K must be at most 2^40");
    if ((int64_t)N * K > LIM) return head_fail(fn, "N * K must be at most 2^40");
    if ((int64_t)B * N > LIM) return head_fail(fn, "B * N must be at most 2^40");
    if (B > (1 << 24) || K > DIM || N > DIM) return head_fail(fn, "B must be at most 2^24, K and N at most 4194240");
    return true;
}

// What the forward and the backward share: S, the flags, p and the presence of the input BN.
static bool head_common_ok(const char* fn, int B, int K, int S, int flags, float p, const float* gamma1,
                           const float* beta1) {
    if (S < 1 || K % S != 0) return head_fail(fn, "S must be at least 1 and divide K");
    if (flags & ~(FR_HEAD_BATCH_STATS | FR_HEAD_DROPOUT)) return head_fail(fn, "unknown flag bits");
    if (!(p >= 0.f && p < 1.f)) return head_fail(fn, "p must be in [0, 1)");
    if ((gamma1 != nullptr) != (beta1 != nullptr)) return head_fail(fn, "gamma1 and beta1 must both be given or both be NULL");
    if (flags & FR_HEAD_BATCH_STATS) {
        if (gamma1 && (int64_t)B * S < 2) return head_fail(fn, "batch statistics of the input BN need B * S >= 2");
        if (B < 2) return head_fail(fn, "batch statistics of the output BN need B >= 2");
    }
    return true;
}

static HeadArgs head_args(const float* X, int B, int K, int S, const float* W, int N, const float* gamma1,
                          const float* beta1, int flags, float p, uint64_t seed, uint64_t offset) {
    HeadArgs a = {};
    a.X = X; a.W = W; a.B = B; a.K = K; a.S = S; a.N = N;
    a.gamma1 = gamma1; a.beta1 = beta1;
    a.batch_stats = (flags & FR_HEAD_BATCH_STATS) != 0;
    a.dropout = (flags & FR_HEAD_DROPOUT) != 0 && p > 0.f;
    a.thresh = a.dropout ? (uint32_t)std::floor((double)p * 4294967296.0) : 0u;
    a.keep_scale = a.dropout ? 1.0f / (1.0f - p) : 1.f;
    a.seed = seed; a.offset = offset;
    return a;
}

}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_head_workspace(int B, int K, int N) {
    if (!head_shape_ok("fr_head_workspace", B, K, N)) return 0;
    return head_workspace(B, K, N);
}

int fr_head_forward(const float* X, int B, int K, int S, const float* W, int N, const float* bias, const float* gamma1,
                    const float* beta1, float* running_mean1, float* running_var1, const float* gamma2,
                    const float* beta2, float* running_mean2, float* running_var2, int flags, float p, float eps,
                    float momentum, uint64_t seed, uint64_t offset, float* Y, float* Z, float* mean1, float* rstd1,
                    float* mean2, float* rstd2, float* A, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "fr_head_forward";
    if (!head_shape_ok(fn, B, K, N) || !head_common_ok(fn, B, K, S, flags, p, gamma1, beta1)) return FR_ERR_ARG;
    if (!std::isfinite(eps) || !(eps > 0.f)) { head_fail(fn, "eps must be finite and positive"); return FR_ERR_ARG; }
    if (!(momentum >= 0.f && momentum <= 1.f)) { head_fail(fn, "momentum must be in [0, 1]"); return FR_ERR_ARG; }
    if (!X || !W || !gamma2 || !beta2 || !Y || !Z || !mean2 || !rstd2 || !ws) {
        head_fail(fn, "null X, W, gamma2, beta2, Y, Z, mean2, rstd2 or ws");
        return FR_ERR_ARG;
    }
    if (!running_mean2 || !running_var2) { head_fail(fn, "null running statistics of the output BN"); return FR_ERR_ARG; }
    if (gamma1 && (!running_mean1 || !running_var1)) {
        head_fail(fn, "null running statistics of the input BN");
        return FR_ERR_ARG;
    }
    if (gamma1 && (!mean1 || !rstd1)) { head_fail(fn, "null mean1 or rstd1 with the input BN"); return FR_ERR_ARG; }
    if (ws_bytes < head_workspace(B, K, N)) { head_fail(fn, "workspace smaller than fr_head_workspace"); return FR_ERR_ARG; }
    const HeadArgs a = head_args(X, B, K, S, W, N, gamma1, beta1, flags, p, seed, offset);
    FR_HIP_CHECK(launch_head_train_forward(a, bias, running_mean1, running_var1, gamma2, beta2, running_mean2, running_var2,
                                           eps, momentum, Y, Z, mean1, rstd1, mean2, rstd2, A, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_head_backward(const float* X, int B, int K, int S, const float* W, int N, const float* gamma1, const float* beta1,
                     const float* gamma2, int flags, float p, uint64_t seed, uint64_t offset, const float* mean1,
                     const float* rstd1, const float* mean2, const float* rstd2, const float* Z, const float* dY, float* dX,
                     float* dW, float* dbias, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, void* ws,
                     size_t ws_bytes, void* stream) {
    const char* fn = "fr_head_backward";
    if (!head_shape_ok(fn, B, K, N) || !head_common_ok(fn, B, K, S, flags, p, gamma1, beta1)) return FR_ERR_ARG;
    if (!X || !W || !gamma2 || !mean2 || !rstd2 || !Z || !dY || !ws) {
        head_fail(fn, "null X, W, gamma2, mean2, rstd2, Z, dY or ws");
        return FR_ERR_ARG;
    }
    if (gamma1 && (!mean1 || !rstd1)) { head_fail(fn, "null mean1 or rstd1 with the input BN"); return FR_ERR_ARG; }
    if (!gamma1 && (dgamma1 || dbeta1)) { head_fail(fn, "dgamma1 or dbeta1 without the input BN"); return FR_ERR_ARG; }
    if (!dX && !dW && !dbias && !dgamma1 && !dbeta1 && !dgamma2 && !dbeta2) {
        head_fail(fn, "at least one gradient must be requested");
        return FR_ERR_ARG;
    }
    if (ws_bytes < head_workspace(B, K, N)) { head_fail(fn, "workspace smaller than fr_head_workspace"); return FR_ERR_ARG; }
    HeadArgs a = head_args(X, B, K, S, W, N, gamma1, beta1, flags, p, seed, offset);
    a.mean1 = mean1; a.rstd1 = rstd1;
    FR_HIP_CHECK(launch_head_train_backward(a, gamma2, mean2, rstd2, Z, dY, dX, dW, dbias, dgamma1, dbeta1, dgamma2, dbeta2,
                                            ws, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
