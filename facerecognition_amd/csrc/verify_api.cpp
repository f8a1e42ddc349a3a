// C ABI of the all-pairs verification (include/frhip.h "All-pairs verification"): the argument checks in front of
// verify.hip's launches.  Handle-free, like the fr_triplet_* ops.  Every argument is checked before the first HIP call.
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

static bool ver_fail(const char* fn, const char* what) {
    set_error(std::string(fn) + ": " + what);
    return false;
}

static bool ver_shape_ok(const char* fn, int N, int D) {
    if (N < 2 || N > (1 << 22)) return ver_fail(fn, "N must be in [2, 2^22]");
    if (D < 4 || D % 4 != 0) return ver_fail(fn, "D must be a positive multiple of 4");
    return true;
}

}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_verify_workspace(int N, int D) {
    if (!ver_shape_ok("fr_verify_workspace", N, D)) return 0;
    return verify_workspace(N);
}

int fr_verify_pairs(const float* E, int N, int D, const int32_t* labels, int normalize, const float* thresholds, int T,
                    uint64_t* counts, uint64_t* totals, uint64_t* hist, int nbins, float lo, float hi, float* row_score,
                    int32_t* row_idx, float* row_sum, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "fr_verify_pairs";
    if (!ver_shape_ok(fn, N, D)) return FR_ERR_ARG;
    if (normalize != 0 && normalize != 1) {
        ver_fail(fn, "normalize must be 0 or 1");
        return FR_ERR_ARG;
    }
    if (T < 0 || T > FR_VERIFY_MAX_THRESHOLDS) {
        ver_fail(fn, "T must be in [0, 64]");
        return FR_ERR_ARG;
    }
    if (T > 0 && (!thresholds || !counts)) {
        ver_fail(fn, "null thresholds or counts with T > 0");
        return FR_ERR_ARG;
    }
    for (int t = 0; t < T; ++t)
        if (!std::isfinite(thresholds[t])) {
            ver_fail(fn, "every threshold must be finite");
            return FR_ERR_ARG;
        }
    if (!E || !labels || !totals || !ws) {
        ver_fail(fn, "null E, labels, totals or ws");
        return FR_ERR_ARG;
    }
    if (hist && (nbins < 1 || nbins > 2048)) {
        ver_fail(fn, "nbins must be in [1, 2048]");
        return FR_ERR_ARG;
    }
    if (hist && !(std::isfinite(lo) && std::isfinite(hi) && hi > lo)) {
        ver_fail(fn, "lo and hi must be finite with hi > lo");
        return FR_ERR_ARG;
    }
    if ((row_score == nullptr) != (row_idx == nullptr)) {
        ver_fail(fn, "row_score and row_idx come together or not at all");
        return FR_ERR_ARG;
    }
    if (ws_bytes < verify_min_workspace(N)) {
        ver_fail(fn, "workspace smaller than the norms and one band of 64 rows (4 ceil64(N) + 2048 ceil(N / 1024) bytes)");
        return FR_ERR_ARG;
    }
    const float inv_w = hist ? (float)nbins / (hi - lo) : 0.f;  // rounded once, here (as fr_match_eval does)
    FR_HIP_CHECK(launch_verify_pairs(E, N, D, labels, normalize, thresholds, T, counts, totals, hist, nbins, lo, inv_w,
                                     row_score, row_idx, row_sum, ws, ws_bytes, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
