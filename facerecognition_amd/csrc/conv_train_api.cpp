// C ABI of backbone training (include/frhip.h "Backbone training"): the argument checks in front of conv_train.hip's
// launches.  Handle-free, like the fr_head_* ops.  Every argument is checked before the first HIP call.
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

static bool ct_fail(const char* fn, const char* what) {
    set_error(std::string(fn) + ": " + what);
    return false;
}

// The convolution's shape and input transform; fills a (without X and Wt).
static bool conv_shape_ok(const char* fn, int B, int H, int W, int Cin, int Cout, int k, int stride, const float* scale,
                          const float* shift, int flags, ConvTrainArgs* a) {
    constexpr int64_t LIM = int64_t(1) << 40;
    constexpr int CH = 1 << 18;  // 9 Cin / 64 column tiles fit a launch grid's second dimension
    if (B < 1 || H < 1 || W < 1) return ct_fail(fn, "B, H and W must be at least 1");
    if (H > 32768 || W > 32768) return ct_fail(fn, "H and W must be at most 32768");
    if (Cin < 4 || Cin % 4 != 0 || Cin > CH) return ct_fail(fn, "Cin must be a positive multiple of 4, at most 262144");
    if (Cout < 4 || Cout % 4 != 0 || Cout > CH) return ct_fail(fn, "Cout must be a positive multiple of 4, at most 262144");
    if (k != 1 && k != 3) return ct_fail(fn, "the kernel must be 1x1 (pad 0) or 3x3 (pad 1)");
    if (stride != 1 && stride != 2) return ct_fail(fn, "stride must be 1 or 2");
    if (flags & ~FR_CONV_IN_RELU) return ct_fail(fn, "unknown flag bits");
    if ((scale != nullptr) != (shift != nullptr)) return ct_fail(fn, "scale and shift must both be given or both be NULL");
    if ((flags & FR_CONV_IN_RELU) && !scale) return ct_fail(fn, "FR_CONV_IN_RELU needs the input transform (scale and shift)");
    const int pad = k == 3 ? 1 : 0;
    const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
    const int64_t pix = (int64_t)B * H * W, M = (int64_t)B * OH * OW;  // Cout k k Cin <= 9 * 2^36 by the limits above
    if (pix > INT32_MAX) return ct_fail(fn, "B * H * W must be below 2^31");
    if (pix * Cin > LIM) return ct_fail(fn, "B * H * W * Cin must be at most 2^40");
    if (M * Cout > LIM) return ct_fail(fn, "B * OH * OW * Cout must be at most 2^40");
    *a = ConvTrainArgs{nullptr, nullptr, scale, shift, (flags & FR_CONV_IN_RELU) != 0, B, H, W, Cin, Cout, k, stride, pad, OH, OW};
    return true;
}

static bool bn_shape_ok(const char* fn, int64_t M, int C, int flags) {
    if (M < 1 || M > (1 << 24)) return ct_fail(fn, "M must be in [1, 2^24]");
    if (C < 4 || C % 4 != 0 || C > (1 << 24)) return ct_fail(fn, "C must be a positive multiple of 4, at most 2^24");
    if (flags & ~(FR_BN_BATCH_STATS | FR_BN_RELU)) return ct_fail(fn, "unknown flag bits");
    if ((flags & FR_BN_BATCH_STATS) && M < 2) return ct_fail(fn, "batch statistics need M >= 2");
    return true;
}

}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_conv_train_workspace(int B, int H, int W, int Cin, int Cout, int k, int stride) {
    ConvTrainArgs a;
    if (!conv_shape_ok("fr_conv_train_workspace", B, H, W, Cin, Cout, k, stride, nullptr, nullptr, 0, &a)) return 0;
    return conv_train_workspace(a);
}

int fr_conv_train_forward(const float* X, int B, int H, int W, int Cin, const float* scale, const float* shift, int flags,
                          const float* Wt, int Cout, int k, int stride, float* Z, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "fr_conv_train_forward";
    ConvTrainArgs a;
    if (!conv_shape_ok(fn, B, H, W, Cin, Cout, k, stride, scale, shift, flags, &a)) return FR_ERR_ARG;
    if (!X || !Wt || !Z || !ws) { ct_fail(fn, "null X, Wt, Z or ws"); return FR_ERR_ARG; }
    if (ws_bytes < conv_train_workspace(a)) { ct_fail(fn, "workspace smaller than fr_conv_train_workspace"); return FR_ERR_ARG; }
    a.X = X; a.Wt = Wt;
    FR_HIP_CHECK(launch_conv_train_forward(a, Z, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_conv_train_backward(const float* X, int B, int H, int W, int Cin, const float* scale, const float* shift, int flags,
                           const float* Wt, int Cout, int k, int stride, const float* dZ, float* dA, float* dW,
                           void* stream) {
    const char* fn = "fr_conv_train_backward";
    ConvTrainArgs a;
    if (!conv_shape_ok(fn, B, H, W, Cin, Cout, k, stride, scale, shift, flags, &a)) return FR_ERR_ARG;
    if (!X || !Wt || !dZ) { ct_fail(fn, "null X, Wt or dZ"); return FR_ERR_ARG; }
    if (!dA && !dW) { ct_fail(fn, "at least one of dA and dW must be requested"); return FR_ERR_ARG; }
    a.X = X; a.Wt = Wt;
    FR_HIP_CHECK(launch_conv_train_backward(a, dZ, dA, dW, (hipStream_t)stream));
    return FR_OK;
}

int fr_bn2d_train_stats(const float* Z, int64_t M, int C, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, int flags, float eps, float momentum, float* mean, float* rstd, float* scale,
                        float* shift, void* stream) {
    const char* fn = "fr_bn2d_train_stats";
    if (!bn_shape_ok(fn, M, C, flags)) return FR_ERR_ARG;
    if (flags & FR_BN_RELU) { ct_fail(fn, "unknown flag bits"); return FR_ERR_ARG; }
    if (!std::isfinite(eps) || !(eps > 0.f)) { ct_fail(fn, "eps must be finite and positive"); return FR_ERR_ARG; }
    if (!(momentum >= 0.f && momentum <= 1.f)) { ct_fail(fn, "momentum must be in [0, 1]"); return FR_ERR_ARG; }
    if (!Z || !gamma || !beta || !running_mean || !running_var || !mean || !rstd || !scale || !shift) {
        ct_fail(fn, "null Z, gamma, beta, running statistics, mean, rstd, scale or shift");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_bn2d_train_stats(Z, M, C, gamma, beta, running_mean, running_var, (flags & FR_BN_BATCH_STATS) != 0,
                                         eps, momentum, mean, rstd, scale, shift, (hipStream_t)stream));
    return FR_OK;
}

int fr_bn_act_forward(const float* Z, int64_t M, int C, const float* scale, const float* shift, const float* Res, int flags,
                      float* Y, void* stream) {
    const char* fn = "fr_bn_act_forward";
    if (!bn_shape_ok(fn, M, C, flags & ~FR_BN_BATCH_STATS)) return FR_ERR_ARG;
    if (flags & FR_BN_BATCH_STATS) { ct_fail(fn, "unknown flag bits"); return FR_ERR_ARG; }
    if (!Z || !scale || !shift || !Y) { ct_fail(fn, "null Z, scale, shift or Y"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_bn_act_forward(Z, M, C, scale, shift, Res, (flags & FR_BN_RELU) != 0, Y, (hipStream_t)stream));
    return FR_OK;
}

int fr_bn_act_backward(const float* dY, const float* Z, int64_t M, int C, const float* mean, const float* rstd,
                       const float* gamma, const float* scale, const float* shift, const float* Res, int flags, float* dZ,
                       float* dRes, float* dgamma, float* dbeta, void* stream) {
    const char* fn = "fr_bn_act_backward";
    if (!bn_shape_ok(fn, M, C, flags)) return FR_ERR_ARG;
    if (!dY || !Z || !mean || !rstd || !gamma || !scale || !shift) {
        ct_fail(fn, "null dY, Z, mean, rstd, gamma, scale or shift");
        return FR_ERR_ARG;
    }
    if (!dZ && !dRes && !dgamma && !dbeta) { ct_fail(fn, "at least one gradient must be requested"); return FR_ERR_ARG; }
    if (dRes && !Res) { ct_fail(fn, "dRes without Res"); return FR_ERR_ARG; }
    if (dRes && (dRes == dY || dRes == dZ)) { ct_fail(fn, "dRes must not alias dY or dZ"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_bn_act_backward(dY, Z, M, C, (flags & FR_BN_BATCH_STATS) != 0, (flags & FR_BN_RELU) != 0, gamma, mean,
                                        rstd, scale, shift, Res, dZ, dRes, dgamma, dbeta, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
