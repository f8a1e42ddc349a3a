// Greedy non-maximum suppression on the device for the batched MTCNN box logic (face_detector.py detect_batch,
// include/frhip.h fr_nms).  The contract is nms.cpp's fr_nms_host: in a given visiting order a box is dropped when a
// box KEPT earlier in that order overlaps it above the threshold, with suppressed()'s float32 operations in the same
// order and IEEE division (this file is built with -ffp-contract=off).  The kept lists are equal element for element.
//
// One workgroup of sixteen waves owns one segment of the order (segments never interact: one (pyramid level, image)
// or one image each).  The segment is walked in chunks of 64 candidates, one lane each:
//   1. every wave tests the chunk against its sixteenth of the boxes kept so far (the kept list is in the global
//      workspace; 1024 of them at a time are staged in LDS, and a kept box is read as an LDS broadcast by the 64
//      lanes); the sixteen verdicts per candidate are OR-ed through LDS;
//   2. wave 0 resolves the chunk: lane l builds the 64-bit mask of the earlier lanes whose box would suppress l's,
//      then the lanes are settled in order (lane j survives when it passed step 1 and no surviving earlier lane is
//      in its mask), and the survivors are appended to the kept list in lane order.
// Most pairs are disjoint: when no lane of the wave has a non-zero intersection the quotient is 0 / den, whose
// verdict needs no division (below); otherwise every lane divides, as the host does.
// No n x n mask exists.  Work is O(n x kept / 1024) per segment with n / 64 sequential steps: right for the 10^2..10^4
// boxes per segment of a working detector, not for 10^5-box levels (those stay on fr_nms_host).
// A second launch sums the per-segment counts into the CSR seg_kept and packs the kept indices segment by segment.
#include <cmath>

#include "engine_internal.h"

namespace fr {
namespace {

struct NBox {
    float x1, y1, x2, y2, area;
};

template <bool MIN_MODE>
__device__ __forceinline__ NBox make_box(const float4& b) {
    NBox q;
    q.x1 = b.x; q.y1 = b.y; q.x2 = b.z; q.y2 = b.w;
    const float w = MIN_MODE ? q.x2 - q.x1 + 1.f : q.x2 - q.x1, h = MIN_MODE ? q.y2 - q.y1 + 1.f : q.y2 - q.y1;
    q.area = w * h;
    return q;
}

// nms.cpp suppressed(): IoU mode drops when ov > t (NaN keeps); 'Min' mode keeps when ov <= t (NaN drops)
template <bool MIN_MODE>
__device__ __forceinline__ bool suppressed(const NBox& k, const NBox& c, float t) {
    const float xx1 = k.x1 > c.x1 ? k.x1 : c.x1, yy1 = k.y1 > c.y1 ? k.y1 : c.y1;
    const float xx2 = k.x2 < c.x2 ? k.x2 : c.x2, yy2 = k.y2 < c.y2 ? k.y2 : c.y2;
    const float iw = MIN_MODE ? xx2 - xx1 + 1.f : xx2 - xx1, ih = MIN_MODE ? yy2 - yy1 + 1.f : yy2 - yy1;
    const float inter = (iw > 0.f ? iw : 0.f) * (ih > 0.f ? ih : 0.f);  // +0, positive or NaN
    const float den = MIN_MODE ? (k.area < c.area ? k.area : c.area) : (k.area + c.area) - inter;
    // Called by whole waves.  inter == 0 in every lane: ov = 0 / den is +-0, or NaN when den is 0 or NaN.  With
    // t >= 0 (fr_nms refuses another), ov > t is false either way, and !(ov <= t) is true exactly for the NaN.
    if (!__any(!(inter == 0.f))) return MIN_MODE ? (!(den == den) || den == 0.f) : false;
    const float ov = inter / den;
    return MIN_MODE ? !(ov <= t) : ov > t;
}

constexpr int NMS_THREADS = 1024, NMS_WAVES = 16, NMS_TILE = 1024;
constexpr int PACK_THREADS = 256, PACK_WAVES = 4;

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool MIN_MODE>
__global__ __launch_bounds__(NMS_THREADS) void k_nms_segments(const float4* __restrict__ boxes, int64_t n,
                                                              const int64_t* __restrict__ order,
                                                              const int64_t* __restrict__ seg_start, float thresh,
                                                              float4* kbox_all, int64_t* kidx_all, int32_t* counts) {
    __shared__ float4 tb[NMS_TILE];
    __shared__ float ta[NMS_TILE];
    __shared__ float4 cb[64];
    __shared__ unsigned char verdict[NMS_WAVES][64];
    __shared__ int s_nk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x;
    // a malformed CSR can make segments overlap, never leave [0, n]
    const int64_t s0 = clamp64(seg_start[seg], 0, n), s1 = clamp64(seg_start[seg + 1], s0, n);
    const int64_t m = s1 - s0;
    if (m <= 0) {
        if (tid == 0) counts[seg] = 0;
        return;
    }
    float4* kbox = kbox_all + s0;   // this segment's kept boxes and indices: at most m of them
    int64_t* kidx = kidx_all + s0;
    int nk = 0;
    for (int64_t c0 = 0; c0 < m; c0 += 64) {
        const int64_t p = c0 + lane;
        bool valid = p < m;
        int64_t idx = -1;
        float4 raw = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) {
            idx = order[s0 + p];
            if (idx < 0 || idx >= n) valid = false;  // an index outside the boxes is skipped
            else raw = boxes[idx];
        }
        const NBox c = make_box<MIN_MODE>(raw);
        bool sup = false;
        for (int t0 = 0; t0 < nk; t0 += NMS_TILE) {
            const int tn = nk - t0 < NMS_TILE ? nk - t0 : NMS_TILE;
            __syncthreads();  // the previous tile has been read
            if (tid < tn) {
                const float4 b = kbox[t0 + tid];
                tb[tid] = b;
                ta[tid] = make_box<MIN_MODE>(b).area;
            }
            __syncthreads();
            for (int j = wave; j < tn; j += NMS_WAVES) {
                const float4 b = tb[j];
                NBox k;
                k.x1 = b.x; k.y1 = b.y; k.x2 = b.z; k.y2 = b.w; k.area = ta[j];
                sup |= suppressed<MIN_MODE>(k, c, thresh);  // every lane calls it (a wave-wide vote inside)
            }
        }
        verdict[wave][lane] = sup ? 1 : 0;
        if (wave == 0) cb[lane] = raw;
        __syncthreads();
        if (wave == 0) {
            int v = 0;
#pragma unroll
            for (int w = 0; w < NMS_WAVES; ++w) v |= verdict[w][lane];
            const bool alive = valid && !v;
            unsigned long long mask = 0;
            for (int j = 0; j < 63; ++j) {
                const NBox k = make_box<MIN_MODE>(cb[j]);
                const bool hit = suppressed<MIN_MODE>(k, c, thresh);
                if (j < lane && hit) mask |= 1ull << j;
            }
            const unsigned long long alive_b = __ballot(alive);
            unsigned long long kept = 0;
            for (int j = 0; j < 64; ++j) {
                const unsigned long long mj = __shfl(mask, j);
                if (((alive_b >> j) & 1ull) && !(mj & kept)) kept |= 1ull << j;
            }
            if ((kept >> lane) & 1ull) {
                const int r = nk + __popcll(kept & ((1ull << lane) - 1ull));
                kbox[r] = raw;
                kidx[r] = idx;
            }
            if (lane == 0) s_nk = nk + __popcll(kept);
        }
        __syncthreads();  // the appended boxes are visible to the workgroup's other waves
        nk = s_nk;
    }
    if (tid == 0) counts[seg] = nk;
}

// seg_kept = the exclusive sum of the counts; keep = the kept indices of segment 0, 1, ... back to back
__global__ __launch_bounds__(PACK_THREADS) void k_nms_pack(const int32_t* __restrict__ counts,
                                                          const int64_t* __restrict__ seg_start, int64_t n, int n_seg,
                                                          const int64_t* __restrict__ kidx_all, int64_t* keep,
                                                          int64_t* seg_kept) {
    __shared__ long long red[PACK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x;
    long long s = 0;
    for (int j = tid; j < seg; j += PACK_THREADS) s += counts[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const int64_t prefix = red[0] + red[1] + red[2] + red[3];
    const int cnt = counts[seg];
    if (tid == 0) {
        seg_kept[seg] = prefix;
        if (seg == n_seg - 1) seg_kept[n_seg] = prefix + cnt;
    }
    const int64_t s0 = clamp64(seg_start[seg], 0, n);
    for (int j = tid; j < cnt; j += PACK_THREADS)
        if (prefix + j < n) keep[prefix + j] = kidx_all[s0 + j];
}

constexpr int64_t NMS_MAX_N = int64_t(1) << 30, NMS_MAX_SEG = 1 << 24;

inline size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

}  // namespace
}  // namespace fr

using namespace fr;

extern "C" {

size_t fr_nms_workspace(int64_t n, int64_t n_seg) {
    if (n < 0 || n > NMS_MAX_N || n_seg < 0 || n_seg > NMS_MAX_SEG) {
        set_error("fr_nms_workspace: n must be 0..2^30 and n_seg 0..2^24");
        return 0;
    }
    return align16((size_t)n * sizeof(float4)) + align16((size_t)n * sizeof(int64_t)) +
           align16((size_t)n_seg * sizeof(int32_t)) + 16;
}

int fr_nms(const float* boxes, int64_t n, const int64_t* order, const int64_t* seg_start, int64_t n_seg, float thresh,
           int min_mode, int64_t* keep, int64_t* seg_kept, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0 || n > NMS_MAX_N) { set_error("fr_nms: n must be 0..2^30"); return FR_ERR_ARG; }
    if (n_seg < 0 || n_seg > NMS_MAX_SEG) { set_error("fr_nms: n_seg must be 0..2^24"); return FR_ERR_ARG; }
    if (!std::isfinite(thresh) || thresh < 0.f) {
        set_error("fr_nms: thresh must be finite and not negative");
        return FR_ERR_ARG;
    }
    if (min_mode != 0 && min_mode != 1) { set_error("fr_nms: min_mode must be 0 or 1"); return FR_ERR_ARG; }
    if (!seg_start || !seg_kept || ((uintptr_t)seg_start & 7) || ((uintptr_t)seg_kept & 7)) {
        set_error("fr_nms: null or misaligned seg_start or seg_kept");
        return FR_ERR_ARG;
    }
    if (n > 0 && (!boxes || !order || !keep || !ws || ((uintptr_t)boxes & 15) || ((uintptr_t)order & 7) ||
                  ((uintptr_t)keep & 7) || ((uintptr_t)ws & 15))) {
        set_error("fr_nms: null or misaligned boxes, order, keep or workspace");
        return FR_ERR_ARG;
    }
    if (n > 0 && ws_bytes < fr_nms_workspace(n, n_seg)) {
        set_error("fr_nms: workspace smaller than fr_nms_workspace");
        return FR_ERR_ARG;
    }
    if (n_seg == 0) return FR_OK;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {  // every segment is empty: no launch
        FR_HIP_CHECK(hipMemsetAsync(seg_kept, 0, (size_t)(n_seg + 1) * sizeof(int64_t), s));
        return FR_OK;
    }
    char* w = (char*)ws;
    float4* kbox = (float4*)w;
    w += align16((size_t)n * sizeof(float4));
    int64_t* kidx = (int64_t*)w;
    w += align16((size_t)n * sizeof(int64_t));
    int32_t* counts = (int32_t*)w;
    if (min_mode)
        hipLaunchKernelGGL(k_nms_segments<true>, dim3((unsigned)n_seg), dim3(NMS_THREADS), 0, s, (const float4*)boxes, n,
                           order, seg_start, thresh, kbox, kidx, counts);
    else
        hipLaunchKernelGGL(k_nms_segments<false>, dim3((unsigned)n_seg), dim3(NMS_THREADS), 0, s, (const float4*)boxes, n,
                           order, seg_start, thresh, kbox, kidx, counts);
    FR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_nms_pack, dim3((unsigned)n_seg), dim3(PACK_THREADS), 0, s, counts, seg_start, n, (int)n_seg, kidx,
                       keep, seg_kept);
    FR_HIP_CHECK(hipGetLastError());
    return FR_OK;
}

}  // extern "C"
