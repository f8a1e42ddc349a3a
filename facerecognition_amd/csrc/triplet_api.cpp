// C ABI of the triplet mining and loss (include/frhip.h "Triplet mining and loss"): the argument checks in front of
// triplet.hip's launches.  Handle-free, like the fr_arcmargin_* ops.  Every argument is checked before the first HIP call.
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

static bool trip_fail(const char* fn, const char* what) {
    set_error(std::string(fn) + ": " + what);
    return false;
}

static bool trip_rows_ok(const char* fn, int N) {
    if (N < 2 || N > 32768) return trip_fail(fn, "N must be in [2, 32768]");
    return true;
}

static bool trip_shape_ok(const char* fn, int N, int D) {
    if (!trip_rows_ok(fn, N)) return false;
    if (D < 4 || D % 4 != 0) return trip_fail(fn, "D must be a positive multiple of 4");
    return true;
}

static bool trip_mode_ok(const char* fn, int mode) {
    if (mode != FR_TRIPLET_SEMI_HARD && mode != FR_TRIPLET_BATCH_HARD && mode != FR_TRIPLET_FIRST)
        return trip_fail(fn, "mode must be FR_TRIPLET_SEMI_HARD, FR_TRIPLET_BATCH_HARD or FR_TRIPLET_FIRST");
    return true;
}

static bool trip_margin_ok(const char* fn, float margin) {
    if (!std::isfinite(margin) || !(margin > 0.f)) return trip_fail(fn, "margin must be finite and positive");
    return true;
}

static bool trip_count_ok(const char* fn, int64_t T) {
    if (T < 1 || T > (int64_t(1) << 40)) return trip_fail(fn, "T must be in [1, 2^40]");
    return true;
}

}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_triplet_workspace(int N, int D) {
    if (!trip_shape_ok("fr_triplet_workspace", N, D)) return 0;
    return triplet_workspace(N);
}

int fr_triplet_count(const int32_t* labels, int N, int mode, int64_t* lims, void* stream) {
    const char* fn = "fr_triplet_count";
    if (!trip_rows_ok(fn, N) || !trip_mode_ok(fn, mode)) return FR_ERR_ARG;
    if (!labels || !lims) {
        trip_fail(fn, "null labels or lims");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_triplet_count(labels, N, mode, lims, (hipStream_t)stream));
    return FR_OK;
}

int fr_triplet_mine(const float* E, int N, int D, const int32_t* labels, int mode, float margin, const int64_t* lims,
                    int32_t* a_idx, int32_t* p_idx, int32_t* n_idx, int64_t capacity, uint8_t* semi, void* ws,
                    size_t ws_bytes, void* stream) {
    const char* fn = "fr_triplet_mine";
    if (!trip_shape_ok(fn, N, D) || !trip_mode_ok(fn, mode) || !trip_margin_ok(fn, margin)) return FR_ERR_ARG;
    if (!E || !labels || !lims || !a_idx || !p_idx || !n_idx || !ws) {
        trip_fail(fn, "null E, labels, lims, a_idx, p_idx, n_idx or ws");
        return FR_ERR_ARG;
    }
    if (capacity < 0) {
        trip_fail(fn, "capacity must not be negative");
        return FR_ERR_ARG;
    }
    if (ws_bytes < triplet_min_workspace(N)) {
        trip_fail(fn, "workspace smaller than one band of 64 anchors (64 N floats and the norms)");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_triplet_mine(E, N, D, labels, mode, margin, lims, a_idx, p_idx, n_idx, capacity, semi, ws, ws_bytes,
                                     (hipStream_t)stream));
    return FR_OK;
}

int fr_triplet_loss_forward(const float* E, int N, int D, const int32_t* a, const int32_t* p, const int32_t* n, int64_t T,
                            float margin, float* terms, float* stats, void* stream) {
    const char* fn = "fr_triplet_loss_forward";
    if (!trip_shape_ok(fn, N, D) || !trip_count_ok(fn, T) || !trip_margin_ok(fn, margin)) return FR_ERR_ARG;
    if (!E || !a || !p || !n || !terms || !stats) {
        trip_fail(fn, "null E, a, p, n, terms or stats");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_triplet_loss_forward(E, D, a, p, n, T, margin, terms, stats, (hipStream_t)stream));
    return FR_OK;
}

int fr_triplet_loss_backward(const float* E, int N, int D, const int32_t* a, const int32_t* p, const int32_t* n, int64_t T,
                             float margin, float u, float* dE, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "fr_triplet_loss_backward";
    if (!trip_shape_ok(fn, N, D) || !trip_count_ok(fn, T) || !trip_margin_ok(fn, margin)) return FR_ERR_ARG;
    if (!std::isfinite(u)) {
        trip_fail(fn, "u must be finite");
        return FR_ERR_ARG;
    }
    if (!E || !a || !p || !n || !dE || !ws) {
        trip_fail(fn, "null E, a, p, n, dE or ws");
        return FR_ERR_ARG;
    }
    if (ws_bytes / 8 < (size_t)T) {
        trip_fail(fn, "workspace smaller than 8 T bytes");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_triplet_loss_backward(E, N, D, a, p, n, T, margin, u, dE, ws, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
