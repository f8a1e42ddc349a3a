// C ABI of the LBPH ops (include/frhip.h "LBPH"): the host-side neighbour table of OpenCV's extended LBP and the
// argument checks in front of lbph.hip's launches.  Handle-free, like the fr_mtcnn_* ops.  Every argument is
// checked before the first HIP call.  Built with -ffp-contract=off (the table's float32 weights are a contract).
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

// lbph.cpp of opencv_contrib's face module, elbp_(): x and y from a double product cast to float, the
// weights in float.
void lbph_table(int radius, int neighbors, LbphTable* t) {
    *t = LbphTable{};
    for (int n = 0; n < neighbors; ++n) {
        const float x = static_cast<float>(radius * cos(2.0 * M_PI * n / static_cast<float>(neighbors)));
        const float y = static_cast<float>(-radius * sin(2.0 * M_PI * n / static_cast<float>(neighbors)));
        const int fx = static_cast<int>(floor(x)), fy = static_cast<int>(floor(y));
        const int cx = static_cast<int>(ceil(x)), cy = static_cast<int>(ceil(y));
        const float ty = y - fy, tx = x - fx;
        t->off[n][0] = fx, t->off[n][1] = fy, t->off[n][2] = cx, t->off[n][3] = cy;
        t->w[n][0] = (1 - tx) * (1 - ty);
        t->w[n][1] = tx * (1 - ty);
        t->w[n][2] = (1 - tx) * ty;
        t->w[n][3] = tx * ty;
    }
}

static bool lbph_params_ok(const char* fn, int radius, int neighbors) {
    if (radius < 1 || radius > 4 || neighbors < 1 || neighbors > 8) {
        set_error(std::string(fn) + ": radius must be 1..4 and neighbors 1..8");
        return false;
    }
    return true;
}

}  // namespace fr

using namespace fr;

extern "C" {

int fr_lbph_table(int radius, int neighbors, int32_t* offs, float* w) {
    if (!lbph_params_ok("fr_lbph_table", radius, neighbors)) return FR_ERR_ARG;
    if (!offs || !w) { set_error("fr_lbph_table: null output"); return FR_ERR_ARG; }
    LbphTable t;
    lbph_table(radius, neighbors, &t);
    for (int n = 0; n < neighbors; ++n)
        for (int e = 0; e < 4; ++e) offs[n * 4 + e] = t.off[n][e], w[n * 4 + e] = t.w[n][e];
    return FR_OK;
}

int fr_lbph_hist(const uint8_t* img, int B, int H, int W, int radius, int neighbors, int grid_x, int grid_y,
                 uint16_t* counts, void* stream) {
    if (!lbph_params_ok("fr_lbph_hist", radius, neighbors)) return FR_ERR_ARG;
    if (!img || !counts || ((uintptr_t)counts & 3)) {
        set_error("fr_lbph_hist: null image or counts, or counts not 4-byte aligned");
        return FR_ERR_ARG;
    }
    if (B < 1 || B > (1 << 24)) { set_error("fr_lbph_hist: B must be 1..2^24"); return FR_ERR_ARG; }
    if (grid_x < 1 || grid_x > 16 || grid_y < 1 || grid_y > 16) {
        set_error("fr_lbph_hist: grid_x and grid_y must be 1..16");
        return FR_ERR_ARG;
    }
    if (H < 1 || H > 512 || W < 1 || W > 512) { set_error("fr_lbph_hist: H and W must be 1..512"); return FR_ERR_ARG; }
    const int cw = (W - 2 * radius) / grid_x, ch = (H - 2 * radius) / grid_y;
    if (W <= 2 * radius || H <= 2 * radius || cw < 1 || ch < 1) {
        set_error("fr_lbph_hist: image too small for the radius and grid (a cell needs at least one pixel)");
        return FR_ERR_ARG;
    }
    if (cw * ch > 65535) { set_error("fr_lbph_hist: more than 65535 pixels per cell (u16 counts)"); return FR_ERR_ARG; }
    LbphTable t;
    lbph_table(radius, neighbors, &t);
    FR_HIP_CHECK(launch_lbph_hist(img, B, H, W, radius, neighbors, grid_x, grid_y, t, counts, (hipStream_t)stream));
    return FR_OK;
}

static bool lbph_match_shape_ok(const char* fn, int B, int64_t N, int D, int k) {
    if (B < 1 || B > 65535 || N < 1 || N > (int64_t(1) << 30) || D < 1 || D > 16 * 16 * 256) {  // 32-bit row math
        set_error(std::string(fn) + ": B must be 1..65535, N 1..2^30, D 1..65536");
        return false;
    }
    if (k < 1 || k > 32) { set_error(std::string(fn) + ": k must be 1..32"); return false; }
    return true;
}

size_t fr_lbph_match_workspace(int B, int64_t N, int D, int k) {
    if (!lbph_match_shape_ok("fr_lbph_match_workspace", B, N, D, k)) return 0;
    return lbph_match_workspace(B, N, k);
}

int fr_lbph_match(const uint16_t* Q, int B, const uint16_t* G, int64_t N, int D, int cell_pixels, int k, double* dist,
                  int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
    if (!lbph_match_shape_ok("fr_lbph_match", B, N, D, k)) return FR_ERR_ARG;
    if (cell_pixels < 1 || cell_pixels > 65535) {
        set_error("fr_lbph_match: cell_pixels must be 1..65535");
        return FR_ERR_ARG;
    }
    if (!Q || !G || !dist || !idx || !ws || ((uintptr_t)Q & 1) || ((uintptr_t)G & 1) || ((uintptr_t)dist & 7) ||
        ((uintptr_t)idx & 3) || ((uintptr_t)ws & 7)) {
        set_error("fr_lbph_match: null or misaligned buffer");
        return FR_ERR_ARG;
    }
    if (ws_bytes < lbph_match_workspace(B, N, k)) {
        set_error("fr_lbph_match: workspace smaller than fr_lbph_match_workspace");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_lbph_match(Q, B, G, N, D, cell_pixels, k, dist, idx, ws, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
