// The box stages of the batched device MTCNN (face_detector.py DeviceMTCNN.detect_batch, include/frhip.h "box
// stages"): what detect_face does in numpy between the P/R/O-nets, as launches whose inputs and outputs stay on the
// device.  Every formula is face_detector.py's, in float32 with every product rounded before its add (this file is
// built with -ffp-contract=off), so the results are bit-identical to the host path.
//
// Selection keeps the input order (np.nonzero / boolean-mask order) through an ordered two-pass compaction:
//   count:  a workgroup counts the passing items of its 2048 consecutive items;
//   scan:   one workgroup turns the counts into exclusive offsets behind a base (0, or the running total a device
//           counter holds) and leaves base + total in the counter;
//   write:  the workgroup walks its items again, 256 at a time; an item's position is the workgroup's offset + the
//           passing items of earlier rounds and waves + the passing lanes below it (a ballot prefix).
// No atomics, no unordered appends.  Positions at or past the capacity are counted and not written.
#include <cmath>

#include "engine_internal.h"

namespace fr {
namespace {

constexpr int CT = 256, CWAVES = 4, CIT = 8, CBLK = CT * CIT;

template <class F>
__global__ __launch_bounds__(CT) void k_compact_count(F f, int64_t total, int32_t* blk) {
    __shared__ int red[CWAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * CBLK;
    int c = 0;
    for (int r = 0; r < CIT; ++r) {
        const int64_t i = base + r * CT + tid;
        c += (i < total && f.pred(i)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) red[wave] = c;
    __syncthreads();
    if (tid == 0) blk[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One workgroup: blk[0..nblk) -> base + exclusive sum, *counter = base + total; base = reset ? 0 : *counter
__global__ __launch_bounds__(1024) void k_compact_scan(int32_t* blk, int nblk, int32_t* counter, int reset) {
    __shared__ int wsum[16];
    __shared__ int s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = reset ? 0 : *counter;
    __syncthreads();
    for (int c0 = 0; c0 < nblk; c0 += 1024) {
        const int i = c0 + tid;
        const int v = i < nblk ? blk[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) woff += wsum[w];
            tot += wsum[w];
        }
        const int run = s_run;
        if (i < nblk) blk[i] = run + woff + incl - v;
        __syncthreads();
        if (tid == 0) s_run = run + tot;
        __syncthreads();
    }
    if (tid == 0) *counter = s_run;
}

template <class F>
__global__ __launch_bounds__(CT) void k_compact_write(F f, int64_t total, const int32_t* __restrict__ blk_off,
                                                      int64_t capacity) {
    __shared__ int wtot[CWAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * CBLK;
    int64_t run = blk_off[blockIdx.x];
    for (int r = 0; r < CIT; ++r) {
        const int64_t i = base + r * CT + tid;
        const bool p = i < total && f.pred(i);
        const unsigned long long b = __ballot(p);
        if (lane == 0) wtot[wave] = __popcll(b);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < CWAVES; ++w) {
            if (w < wave) woff += wtot[w];
            tot += wtot[w];
        }
        const int64_t pos = run + woff + __popcll(b & ((1ull << lane) - 1ull));
        if (p && pos < capacity) f.write(i, pos);
        run += tot;
        __syncthreads();
    }
}

inline int64_t compact_blocks(int64_t total) { return (total + CBLK - 1) / CBLK; }

template <class F>
hipError_t run_compact(const F& f, int64_t total, int64_t capacity, int32_t* counter, int reset, void* ws,
                       hipStream_t s) {
    const int64_t nblk = compact_blocks(total);
    int32_t* blk = (int32_t*)ws;
    hipLaunchKernelGGL(k_compact_count<F>, dim3((unsigned)nblk), dim3(CT), 0, s, f, total, blk);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, s, blk, (int)nblk, counter, reset);
    hipLaunchKernelGGL(k_compact_write<F>, dim3((unsigned)nblk), dim3(CT), 0, s, f, total, (const int32_t*)blk, capacity);
    return hipGetLastError();
}

// ---- P-net candidates: detect_face's np.nonzero(prob >= th0) and generateBoundingBox lines
struct CandF {
    const float* map;  // [B][hh][ww][6]
    int hh, ww, B, level;
    float scale, th;
    float4* box;
    float* score;
    float4* reg;
    int32_t* seg;
    __device__ bool pred(int64_t i) const { return map[i * 6 + 1] >= th; }
    __device__ void write(int64_t i, int64_t pos) const {
        const int x = (int)(i % ww), y = (int)((i / ww) % hh), b = (int)(i / ((int64_t)ww * hh));
        const float cx = (float)x, cy = (float)y;
        const float* m = map + i * 6;
        box[pos] = make_float4(floorf((2.f * cx + 1.f) / scale), floorf((2.f * cy + 1.f) / scale),
                               floorf((2.f * cx + 12.f) / scale), floorf((2.f * cy + 12.f) / scale));
        score[pos] = m[1];
        reg[pos] = make_float4(m[2], m[3], m[4], m[5]);
        seg[pos] = level * B + b;
    }
};

// ---- R-net / O-net selection: score > th (strict), rows gathered
struct SelectF {
    const float* out;  // [n][C]
    int C;
    float th;
    const float4* box;
    const int32_t* img;
    float4* obox;
    float* oscore;
    float4* oreg;
    int32_t* oimg;
    float* opts;  // C == 16: [.][10]
    __device__ bool pred(int64_t i) const { return out[i * C + 1] > th; }
    __device__ void write(int64_t i, int64_t pos) const {
        const float* o = out + i * C;
        obox[pos] = box[i];
        oscore[pos] = o[1];
        oreg[pos] = make_float4(o[2], o[3], o[4], o[5]);
        oimg[pos] = img[i];
        if (opts)
            for (int k = 0; k < 10; ++k) opts[pos * 10 + k] = o[6 + k];
    }
};

// ---- regression, _rerec, _pad and the ok filter behind a kept list
struct CropF {
    const float4* box;
    const float* score;
    const float4* reg;
    const int32_t* img;
    int64_t n;
    int B;
    const int64_t* keep;    // NULL: row i itself
    const int64_t* n_keep;  // NULL: n rows
    int plus1, W, H;
    float4* obox;
    float* oscore;
    int32_t* oimg;
    int32_t* regions;  // [.][5]
    __device__ bool eval(int64_t i, float4* ob, int64_t* src, int* r) const {
        if (n_keep && i >= *n_keep) return false;
        const int64_t g = keep ? keep[i] : i;
        if (g < 0 || g >= n) return false;
        const float4 b = box[g], m = reg[g];
        // the P stage: b + reg (x2 - x1); _bbreg: b + reg (x2 - x1 + 1)
        const float bw = plus1 ? b.z - b.x + 1.f : b.z - b.x, bh = plus1 ? b.w - b.y + 1.f : b.w - b.y;
        const float x1 = b.x + m.x * bw, y1 = b.y + m.y * bh, x2 = b.z + m.z * bw, y2 = b.w + m.w * bh;
        // _rerec
        const float h = y2 - y1, w = x2 - x1;
        const float l = (w >= h || w != w) ? w : h;  // np.maximum
        float4 q;
        q.x = (x1 + w * 0.5f) - l * 0.5f;
        q.y = (y1 + h * 0.5f) - l * 0.5f;
        q.z = q.x + l;
        q.w = q.y + l;
        // _pad: np.trunc(.).astype(int32), clamped
        int x = (int)truncf(q.x), y = (int)truncf(q.y), ex = (int)truncf(q.z), ey = (int)truncf(q.w);
        if (x < 1) x = 1;
        if (y < 1) y = 1;
        if (ex > W) ex = W;
        if (ey > H) ey = H;
        *ob = q;
        *src = g;
        r[0] = y - 1; r[1] = x - 1; r[2] = ey - y + 1; r[3] = ex - x + 1;
        return ey > y - 1 && ex > x - 1;
    }
    __device__ bool pred(int64_t i) const {
        float4 q;
        int64_t g;
        int r[4];
        return eval(i, &q, &g, r);
    }
    __device__ void write(int64_t i, int64_t pos) const {
        float4 q;
        int64_t g;
        int r[4];
        eval(i, &q, &g, r);
        const int im = img[g] % B;
        obox[pos] = q;
        oscore[pos] = score[g];
        oimg[pos] = im;
        int32_t* o = regions + pos * 5;
        o[0] = im; o[1] = r[0]; o[2] = r[1]; o[3] = r[2]; o[4] = r[3];
    }
};

// ---- the O stage's landmark points and _bbreg, one thread per box
__global__ __launch_bounds__(256) void k_final_boxes(const float4* __restrict__ box, const float4* __restrict__ reg,
                                                     const float* __restrict__ pts, int64_t n,
                                                     const int32_t* __restrict__ n_dev, float4* obox, float* opts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (n_dev && i >= *n_dev)) return;
    const float4 b = box[i], m = reg[i];
    const float w = b.z - b.x + 1.f, h = b.w - b.y + 1.f;
    for (int k = 0; k < 5; ++k) {
        opts[i * 10 + 2 * k] = (w * pts[i * 10 + k] + b.x) - 1.f;
        opts[i * 10 + 2 * k + 1] = (h * pts[i * 10 + 5 + k] + b.y) - 1.f;
    }
    obox[i] = make_float4(b.x + m.x * w, b.y + m.y * h, b.z + m.z * w, b.w + m.w * h);
}

constexpr int64_t MAX_ITEMS = int64_t(1) << 30;

bool ws_ok(const char* fn, int64_t total, void* ws, size_t ws_bytes) {
    if (!ws || ((uintptr_t)ws & 3) || ws_bytes < (size_t)compact_blocks(total) * sizeof(int32_t)) {
        set_error(std::string(fn) + ": null, misaligned or too small workspace (fr_mtcnn_compact_workspace)");
        return false;
    }
    return true;
}

inline bool mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }
inline bool mis4(const void* p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace
}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_mtcnn_compact_workspace(int64_t total) {
    if (total < 1 || total > MAX_ITEMS) {
        set_error("fr_mtcnn_compact_workspace: total must be 1..2^30");
        return 0;
    }
    return (size_t)compact_blocks(total) * sizeof(int32_t);
}

int fr_mtcnn_candidates(const float* map, int B, int hh, int ww, float scale, float thresh, int level,
                        int64_t capacity, float* box, float* score, float* reg, int32_t* seg, int32_t* counter,
                        void* ws, size_t ws_bytes, void* stream) {
    if (B < 1 || hh < 1 || ww < 1 || (int64_t)B * hh * ww > MAX_ITEMS) {
        set_error("fr_mtcnn_candidates: B, hh and ww must be positive with B hh ww <= 2^30");
        return FR_ERR_ARG;
    }
    if (!std::isfinite(scale) || scale <= 0.f || !std::isfinite(thresh) || thresh < 0.f) {
        set_error("fr_mtcnn_candidates: scale must be finite and positive, thresh finite and not negative");
        return FR_ERR_ARG;
    }
    if (level < 0 || level > 4095 || (int64_t)(level + 1) * B > (int64_t(1) << 30)) {
        set_error("fr_mtcnn_candidates: level must be 0..4095 with (level + 1) B <= 2^30");
        return FR_ERR_ARG;
    }
    if (capacity <= 0 || capacity > MAX_ITEMS) {
        set_error("fr_mtcnn_candidates: capacity must be 1..2^30");
        return FR_ERR_ARG;
    }
    if (!map || !box || !score || !reg || !seg || !counter || mis4(map) || mis16(box) || mis4(score) || mis16(reg) ||
        mis4(seg) || mis4(counter)) {
        set_error("fr_mtcnn_candidates: null or misaligned buffer");
        return FR_ERR_ARG;
    }
    const int64_t total = (int64_t)B * hh * ww;
    if (!ws_ok("fr_mtcnn_candidates", total, ws, ws_bytes)) return FR_ERR_ARG;
    CandF f{map, hh, ww, B, level, scale, thresh, (float4*)box, score, (float4*)reg, seg};
    FR_HIP_CHECK(run_compact(f, total, capacity, counter, 0, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_mtcnn_select(const float* out, int64_t n, int C, float thresh, const float* box, const int32_t* img,
                    float* obox, float* oscore, float* oreg, int32_t* oimg, float* opts, int32_t* counter, void* ws,
                    size_t ws_bytes, void* stream) {
    if (n < 1 || n > MAX_ITEMS) { set_error("fr_mtcnn_select: n must be 1..2^30"); return FR_ERR_ARG; }
    if (C != 6 && C != 16) { set_error("fr_mtcnn_select: C must be 6 (R-net) or 16 (O-net)"); return FR_ERR_ARG; }
    if (!std::isfinite(thresh) || thresh < 0.f) {
        set_error("fr_mtcnn_select: thresh must be finite and not negative");
        return FR_ERR_ARG;
    }
    if (!out || !box || !img || !obox || !oscore || !oreg || !oimg || !counter || (C == 16) != (opts != nullptr) ||
        mis4(out) || mis16(box) || mis4(img) || mis16(obox) || mis4(oscore) || mis16(oreg) || mis4(oimg) || mis4(opts) ||
        mis4(counter)) {
        set_error("fr_mtcnn_select: null or misaligned buffer (opts exactly when C = 16)");
        return FR_ERR_ARG;
    }
    if (!ws_ok("fr_mtcnn_select", n, ws, ws_bytes)) return FR_ERR_ARG;
    SelectF f{out, C, thresh, (const float4*)box, img, (float4*)obox, oscore, (float4*)oreg, oimg, opts};
    FR_HIP_CHECK(run_compact(f, n, n, counter, 1, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_mtcnn_crop_boxes(const float* box, const float* score, const float* reg, const int32_t* img, int64_t n, int B,
                        const int64_t* keep, const int64_t* n_keep, int plus1, int W, int H, float* obox,
                        float* oscore, int32_t* oimg, int32_t* regions, int32_t* counter, void* ws, size_t ws_bytes,
                        void* stream) {
    if (n < 1 || n > MAX_ITEMS) { set_error("fr_mtcnn_crop_boxes: n must be 1..2^30"); return FR_ERR_ARG; }
    if (B < 1 || W < 1 || H < 1 || W > (1 << 24) || H > (1 << 24) || (plus1 != 0 && plus1 != 1)) {
        set_error("fr_mtcnn_crop_boxes: B, W and H must be positive (W, H <= 2^24) and plus1 0 or 1");
        return FR_ERR_ARG;
    }
    if (!box || !score || !reg || !img || !obox || !oscore || !oimg || !regions || !counter || mis16(box) ||
        mis4(score) || mis16(reg) || mis4(img) || mis16(obox) || mis4(oscore) || mis4(oimg) || mis4(regions) ||
        mis4(counter) || ((uintptr_t)keep & 7) || ((uintptr_t)n_keep & 7)) {
        set_error("fr_mtcnn_crop_boxes: null or misaligned buffer");
        return FR_ERR_ARG;
    }
    if (!ws_ok("fr_mtcnn_crop_boxes", n, ws, ws_bytes)) return FR_ERR_ARG;
    CropF f{(const float4*)box, score, (const float4*)reg, img, n, B, keep, n_keep, plus1, W, H, (float4*)obox, oscore,
            oimg, regions};
    FR_HIP_CHECK(run_compact(f, n, n, counter, 1, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_mtcnn_final_boxes(const float* box, const float* reg, const float* pts, int64_t n, const int32_t* n_dev,
                         float* obox, float* opts, void* stream) {
    if (n < 1 || n > MAX_ITEMS) { set_error("fr_mtcnn_final_boxes: n must be 1..2^30"); return FR_ERR_ARG; }
    if (!box || !reg || !pts || !obox || !opts || mis16(box) || mis16(reg) || mis4(pts) || mis16(obox) || mis4(opts) ||
        mis4(n_dev)) {
        set_error("fr_mtcnn_final_boxes: null or misaligned buffer");
        return FR_ERR_ARG;
    }
    hipLaunchKernelGGL(k_final_boxes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)box, (const float4*)reg, pts, n, n_dev, (float4*)obox, opts);
    FR_HIP_CHECK(hipGetLastError());
    return FR_OK;
}

}  // extern "C"
