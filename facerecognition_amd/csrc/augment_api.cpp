// C ABI of the augmentation (include/frhip.h "Augmentation"): the argument checks in front of augment.hip's launch and
// the staging of the host op lists.  Handle-free.  Every argument, every opcode and every op argument is checked before
// the first HIP call: nothing the kernel turns into an index is left unchecked here unless the kernel range-checks it
// per pixel (the source coordinates of the two transforms).
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "engine_internal.h"

namespace fr {

static bool aug_fail(const char* fn, const std::string& what) {
    set_error(std::string(fn) + ": " + what);
    return false;
}

static size_t aug_align(size_t v) { return (v + 255) & ~(size_t)255; }

// ws: args f64 [B][n][8] | ops i32 [B][n] | norm f32 [256], each part 256-byte aligned
static size_t aug_args_bytes(int B, int n) { return aug_align((size_t)B * n * FR_AUGMENT_ARGS * sizeof(double)); }
static size_t aug_ops_bytes(int B, int n) { return aug_align((size_t)B * n * sizeof(int32_t)); }
static size_t aug_ws_bytes(int B, int n) { return aug_args_bytes(B, n) + aug_ops_bytes(B, n) + 256 * sizeof(float); }

static bool aug_batch_ok(const char* fn, int B, int n_ops) {
    if (B < 1 || B > (1 << 24)) return aug_fail(fn, "B must be in [1, 2^24]");
    if (n_ops < 0 || n_ops > FR_AUGMENT_MAX_OPS) return aug_fail(fn, "n_ops must be in [0, 16]");
    return true;
}

static bool aug_is_int(double v) { return v == std::floor(v); }

static bool aug_box_ok(const double* a, int H, int W) {
    for (int t = 0; t < 4; ++t)
        if (!aug_is_int(a[t]) || a[t] < 0 || a[t] > 65536) return false;
    return a[2] >= 1 && a[3] >= 1 && a[0] + a[2] <= H && a[1] + a[3] <= W;
}

// one image's row of the op list
static bool aug_row_ok(const char* fn, int b, const int32_t* ops, const double* args, int n_ops, int H, int W) {
    bool erased = false;
    for (int k = 0; k < n_ops; ++k) {
        const int op = ops[k];
        const double* a = args + (size_t)k * FR_AUGMENT_ARGS;
        const std::string at = " (image " + std::to_string(b) + ", op " + std::to_string(k) + ")";
        if (op < FR_AUG_NOP || op > FR_AUG_ERASE) return aug_fail(fn, "unknown opcode " + std::to_string(op) + at);
        for (int t = 0; t < FR_AUGMENT_ARGS; ++t)
            if (!std::isfinite(a[t])) return aug_fail(fn, "every argument must be finite" + at);
        if (op == FR_AUG_NOP) continue;
        if (erased) return aug_fail(fn, "FR_AUG_ERASE must be the last op of its row, once" + at);
        switch (op) {
            case FR_AUG_AFFINE_NEAREST:
                for (int c = 0; c < 4; ++c) {
                    const double x = (c & 1) ? W : 0, y = (c & 2) ? H : 0;
                    if (!(std::fabs(x * a[0] + y * a[1] + a[2]) < 32768.0 && std::fabs(x * a[3] + y * a[4] + a[5]) < 32768.0))
                        return aug_fail(fn, "affine source coordinates must stay inside +-32768" + at);
                }
                // FIX(m2 + m0/2 + m1/2) itself must fit an int as well
                if (!(std::fabs(a[2] + a[0] * 0.5 + a[1] * 0.5) < 32767.0 && std::fabs(a[5] + a[3] * 0.5 + a[4] * 0.5) < 32767.0 &&
                      std::fabs(a[0]) < 32767.0 && std::fabs(a[1]) < 32767.0 && std::fabs(a[3]) < 32767.0 && std::fabs(a[4]) < 32767.0))
                    return aug_fail(fn, "affine coefficients must stay inside +-32767" + at);
                break;
            case FR_AUG_CROP_RESIZE:
                if (!aug_box_ok(a, H, W)) return aug_fail(fn, "the crop box must be non-empty integers inside the image" + at);
                break;
            case FR_AUG_BRIGHTNESS:
            case FR_AUG_CONTRAST:
            case FR_AUG_SATURATION:
                if (a[0] < 0) return aug_fail(fn, "an enhancement factor must be >= 0" + at);
                break;
            case FR_AUG_HUE:
                if (a[0] < -0.5 || a[0] > 0.5) return aug_fail(fn, "the hue factor must be in [-0.5, 0.5]" + at);
                break;
            case FR_AUG_GAUSS_BLUR: {
                if (!(a[0] == 3 || a[0] == 5 || a[0] == 7)) return aug_fail(fn, "blur k must be 3, 5 or 7" + at);
                const int r = (int)a[0] / 2;
                if (r >= H || r >= W) return aug_fail(fn, "blur k / 2 must be below H and W (reflect padding)" + at);
                break;
            }
            case FR_AUG_ERASE:
                if (!aug_box_ok(a, H, W)) return aug_fail(fn, "the erase box must be non-empty integers inside the image" + at);
                erased = true;
                break;
            default:
                break;
        }
    }
    return true;
}

// Pinned staging, one buffer per device, reused by every call: the copy out of it is asynchronous, so the next call
// waits for the previous copy's event before it overwrites the buffer.
struct AugStage {
    void* host = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
};
static std::mutex g_aug_mu;
static std::map<int, AugStage> g_aug_stage;

}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_augment_workspace(int B, int n_ops) {
    if (!aug_batch_ok("fr_augment_workspace", B, n_ops)) return 0;
    return aug_ws_bytes(B, n_ops);
}

int fr_augment(const uint8_t* in, int B, int H, int W, const int32_t* ops, const double* args, int n_ops, float* out_f32,
               uint8_t* out_u8, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "fr_augment";
    if (!aug_batch_ok(fn, B, n_ops)) return FR_ERR_ARG;
    if (H < 1 || W < 1) {
        aug_fail(fn, "H and W must be >= 1");
        return FR_ERR_ARG;
    }
    if ((int64_t)H * W * 6 > 153600 || (int64_t)H + W > 512) {
        aug_fail(fn, "the image exceeds the LDS budget: 6 H W <= 153600 and H + W <= 512 (160 x 160 is the largest square)");
        return FR_ERR_ARG;
    }
    if (!in || !ws || (n_ops > 0 && (!ops || !args))) {
        aug_fail(fn, "null in, ops, args or ws");
        return FR_ERR_ARG;
    }
    if ((uintptr_t)ws & 7) {
        aug_fail(fn, "ws must be 8-byte aligned");
        return FR_ERR_ARG;
    }
    if (!out_f32 && !out_u8) {
        aug_fail(fn, "out_f32 and out_u8 are both null");
        return FR_ERR_ARG;
    }
    if (ws_bytes < aug_ws_bytes(B, n_ops)) {
        aug_fail(fn, "workspace smaller than fr_augment_workspace(B, n_ops)");
        return FR_ERR_ARG;
    }
    for (int b = 0; b < B; ++b)
        if (!aug_row_ok(fn, b, ops + (size_t)b * n_ops, args + (size_t)b * n_ops * FR_AUGMENT_ARGS, n_ops, H, W))
            return FR_ERR_ARG;

    const size_t na = aug_args_bytes(B, n_ops), no = aug_ops_bytes(B, n_ops), total = aug_ws_bytes(B, n_ops);
    int device = 0;
    FR_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(g_aug_mu);
    AugStage& st = g_aug_stage[device];
    if (!st.copied) FR_HIP_CHECK(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    else FR_HIP_CHECK(hipEventSynchronize(st.copied));  // the previous copy out of the buffer has finished
    if (st.bytes < total) {
        if (st.host) FR_HIP_CHECK(hipHostFree(st.host));
        st.host = nullptr;
        st.bytes = 0;
        FR_HIP_CHECK(hipHostMalloc(&st.host, total, hipHostMallocDefault));
        st.bytes = total;
    }
    char* h = (char*)st.host;
    if (n_ops > 0) {
        std::memcpy(h, args, (size_t)B * n_ops * FR_AUGMENT_ARGS * sizeof(double));
        std::memcpy(h + na, ops, (size_t)B * n_ops * sizeof(int32_t));
    }
    float* norm = (float*)(h + na + no);
    for (int u = 0; u < 256; ++u) norm[u] = ((float)u / 255.0f - 0.5f) / 0.5f;  // ToTensor, then Normalize(0.5, 0.5)
    hipStream_t s = (hipStream_t)stream;
    FR_HIP_CHECK(hipMemcpyAsync(ws, h, total, hipMemcpyHostToDevice, s));
    FR_HIP_CHECK(hipEventRecord(st.copied, s));
    char* d = (char*)ws;
    FR_HIP_CHECK(launch_augment(in, B, H, W, (const int32_t*)(d + na), (const double*)d, n_ops,
                                (const float*)(d + na + no), out_f32, out_u8, s));
    return FR_OK;
}

}  // extern "C"
