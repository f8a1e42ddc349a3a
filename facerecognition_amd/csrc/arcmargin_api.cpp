// C ABI of the ArcFace margin loss (include/frhip.h "ArcFace margin loss"): the argument checks in front of
// arcmargin.hip's launches.  Handle-free, like the fr_tsne_* ops.  Every argument is checked before the first HIP call.
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

static bool arc_fail(const char* fn, const char* what) {
    set_error(std::string(fn) + ": " + what);
    return false;
}

static bool arc_shape_ok(const char* fn, int B, int C, int D) {
    constexpr int64_t LIM = int64_t(1) << 40;
    if (B < 1) return arc_fail(fn, "B must be at least 1");
    if (C < 2) return arc_fail(fn, "C must be at least 2");
    if (D < 4 || D % 4 != 0) return arc_fail(fn, "D must be a positive multiple of 4");
    if ((int64_t)B * C > LIM) return arc_fail(fn, "B * C must be at most 2^40");
    if ((int64_t)C * D > LIM) return arc_fail(fn, "C * D must be at most 2^40");
    if ((int64_t)B * D > LIM) return arc_fail(fn, "B * D must be at most 2^40");
    return true;
}

static bool arc_scalars_ok(const char* fn, float lam, float scale, float margin, float label_smoothing) {
    if (!std::isfinite(scale) || !(scale > 0.f)) return arc_fail(fn, "scale must be finite and positive");
    if (!(margin >= 0.f) || !((double)margin < M_PI)) return arc_fail(fn, "margin must be in [0, pi)");
    if (!(lam >= 0.f && lam <= 1.f)) return arc_fail(fn, "lam must be in [0, 1]");
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return arc_fail(fn, "label_smoothing must be in [0, 1)");
    return true;
}

static ArcArgs arc_args(const float* E, int B, int D, const float* W, int C, const int32_t* label,
                        const int32_t* label_b, float lam, float scale, float margin, int easy_margin,
                        float label_smoothing) {
    ArcArgs a = {};
    a.E = E; a.W = W; a.B = B; a.C = C; a.D = D;
    a.label = label; a.label_b = label_b;
    a.lam = label_b ? lam : 1.f;
    a.scale = scale;
    a.label_smoothing = label_smoothing;
    const double m = (double)margin;
    a.cos_m = (float)std::cos(m);
    a.sin_m = (float)std::sin(m);
    a.th = (float)std::cos(M_PI - m);
    a.mm = (float)(std::sin(M_PI - m) * m);
    a.easy_margin = easy_margin != 0;
    return a;
}

}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_arcmargin_workspace(int B, int C, int D) {
    if (!arc_shape_ok("fr_arcmargin_workspace", B, C, D)) return 0;
    return arcmargin_workspace(B, C, D);
}

int fr_arcmargin_forward(const float* E, int B, int D, const float* W, int C, const int32_t* label,
                         const int32_t* label_b, float lam, float scale, float margin, int easy_margin,
                         float label_smoothing, float* loss, float* lse, float* inv_e, float* inv_w, float* logits,
                         void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "fr_arcmargin_forward";
    if (!arc_shape_ok(fn, B, C, D) || !arc_scalars_ok(fn, lam, scale, margin, label_smoothing)) return FR_ERR_ARG;
    if (!E || !W || !label || !loss || !lse || !inv_e || !inv_w || !ws) {
        arc_fail(fn, "null E, W, label, loss, lse, inv_e, inv_w or ws");
        return FR_ERR_ARG;
    }
    if (ws_bytes < arcmargin_workspace(B, C, D)) {
        arc_fail(fn, "workspace smaller than fr_arcmargin_workspace");
        return FR_ERR_ARG;
    }
    ArcArgs a = arc_args(E, B, D, W, C, label, label_b, lam, scale, margin, easy_margin, label_smoothing);
    a.inv_e_out = inv_e; a.inv_w_out = inv_w;
    a.loss = loss; a.lse = lse; a.logits = logits;
    FR_HIP_CHECK(launch_arcmargin_forward(a, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_arcmargin_backward(const float* E, int B, int D, const float* W, int C, const int32_t* label,
                          const int32_t* label_b, float lam, float scale, float margin, int easy_margin,
                          float label_smoothing, const float* lse, const float* inv_e, const float* inv_w,
                          const float* u, const float* dlogits, float* dE, float* dW, void* ws, size_t ws_bytes,
                          void* stream) {
    const char* fn = "fr_arcmargin_backward";
    if (!arc_shape_ok(fn, B, C, D) || !arc_scalars_ok(fn, lam, scale, margin, label_smoothing)) return FR_ERR_ARG;
    if (!E || !W || !label || !inv_e || !inv_w || !ws) {
        arc_fail(fn, "null E, W, label, inv_e, inv_w or ws");
        return FR_ERR_ARG;
    }
    if ((u != nullptr) == (dlogits != nullptr)) {
        arc_fail(fn, "exactly one of u and dlogits must be given");
        return FR_ERR_ARG;
    }
    if (u && !lse) { arc_fail(fn, "null lse with u"); return FR_ERR_ARG; }
    if (!dE && !dW) { arc_fail(fn, "at least one of dE and dW must be given"); return FR_ERR_ARG; }
    if (ws_bytes < arcmargin_workspace(B, C, D)) {
        arc_fail(fn, "workspace smaller than fr_arcmargin_workspace");
        return FR_ERR_ARG;
    }
    ArcArgs a = arc_args(E, B, D, W, C, label, label_b, lam, scale, margin, easy_margin, label_smoothing);
    a.inv_e = inv_e; a.inv_w = inv_w;
    a.lse = const_cast<float*>(lse);
    a.u = u; a.dlogits = dlogits;
    FR_HIP_CHECK(launch_arcmargin_backward(a, dE, dW, ws, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
