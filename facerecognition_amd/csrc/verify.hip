// All-pairs 1:1 verification over one set of labelled embeddings (the reference's compute_verification_accuracy,
// evaluated on every pair instead of 10 000 sampled ones; DESIGN.md §4 "Verification").
//
// Replaces: models/arcface/train_arcface.py:114-210 and models/facenet/train_facenet.py:64-160 (a Python loop with one
// np.dot per sampled pair, unseeded).
//
// Scores are exact f32: score_tile.h's v_mfma_f32_16x16x4f32 tile loop (64 rows x 64 rows, D staged through LDS in
// 64-float chunks, k = 16 t16 + 4 (lane >> 4) + c), then s = (g r_i) r_j with r = 1 / (sqrt(sum e^2) + 1e-8) (r = 1
// without normalisation).  No N x N matrix is stored.
//   prep_kernel     r[i] (score_tile.h's row_sqsum, IEEE square root and division); zeroes counts and totals
//   sweep_kernel    workgroup (row tile, column chunk): 64 rows x the chunk's VCHUNK columns, tiles in ascending j.
//                   Per-row state (sums, best / worst mate, best impostor) in registers, a lane owns the columns
//                   = its lane & 15 (mod 16) of its 4 rows; at the chunk's end a 16-lane tree, then one partial per
//                   (row, chunk).  i < j pairs only: a u32 histogram pair in LDS, per-thread packed threshold counters
//                   in LDS, the totals in registers; all flushed with 64-bit integer adds.
//   combine_kernel  one thread per row: the chunk partials in ascending chunk order -> row_score, row_idx, row_sum
// The chunk width is a constant, so every float sum's order is fixed by (N, D): the band of rows one launch covers
// (what the workspace holds) changes no bit.  Without row outputs the tiles below the diagonal are skipped.
#include "score_tile.h"
#include "frhip.h"
#include <float.h>
#include <limits.h>

#include <algorithm>

namespace fr {
using namespace tile;
namespace {

constexpr int VCHUNK = 1024;  // columns per partial: 16 tiles
constexpr int PART_B = 32;    // bytes of partials per (row, chunk): 2 sums, 3 scores, 3 indices

int pad64(int n) { return (n + 63) / 64 * 64; }
int n_chunks(int N) { return (N + VCHUNK - 1) / VCHUNK; }

// r[i] = 1 / (sqrt(sum_k e_ik^2) + 1e-8), the square sum by score_tile.h's row_sqsum; 1 when !normalize.
__global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ X, int R, int D, int normalize,
                                                   float* __restrict__ rinv, unsigned long long* __restrict__ counts,
                                                   int T, unsigned long long* __restrict__ totals) {
    if (blockIdx.x == 0) {
        if (threadIdx.x < 2 * T) counts[threadIdx.x] = 0;
        if (threadIdx.x < 2) totals[threadIdx.x] = 0;
    }
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    if (!normalize) {
        if (lane == 0) rinv[r] = 1.f;
        return;
    }
    const float ss = row_sqsum(X + (size_t)r * D, D);
    if (lane == 0) rinv[r] = __fdiv_rn(1.f, __fadd_rn(__fsqrt_rn(ss), 1e-8f));
}

struct VerifyArgs {
    const float* E;
    int N, D;
    const int32_t* labels;
    const float* rinv;
    int T;
    unsigned long long* counts;  // [T][2]
    unsigned long long* totals;  // [2]
    unsigned long long* hist;    // [2][nbins] or null
    int nbins;
    float lo, inv_w;
    int rows;  // 1: the partials are wanted (row_score / row_idx / row_sum); 0: only i < j tiles are swept
    int b0, b1, R;  // the band of rows of this launch, R = b1 - b0 rounded up to whole tiles
    float* part;    // [NC][R] x {sum_g, sum_i, best_g, worst_g, best_i} f32 then {3 indices} i32
    float thr[FR_VERIFY_MAX_THRESHOLDS];
};

// (score, index) of the larger score, ties to the lower index; -1 (no candidate yet) loses every tie
__device__ __forceinline__ void take_max(float& d, int& j, float od, int oj) {
    if (od > d || (od == d && (unsigned)oj < (unsigned)j)) {
        d = od;
        j = oj;
    }
}

__device__ __forceinline__ void take_min(float& d, int& j, float od, int oj) {
    if (od < d || (od == d && (unsigned)oj < (unsigned)j)) {
        d = od;
        j = oj;
    }
}

__global__ __launch_bounds__(256) void sweep_kernel(const VerifyArgs a) {
    __shared__ __attribute__((aligned(16))) float sXY[2 * MT * LD];
    extern __shared__ __attribute__((aligned(16))) char dyn[];  // [T][256] packed counters, [2][nbins] histograms
    uint32_t* cnt = (uint32_t*)dyn;
    uint32_t* hist2 = cnt + a.T * 256;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N;
    const int x0 = a.b0 + blockIdx.x * MT;
    const int c0 = blockIdx.y * VCHUNK, c1 = min(N, c0 + VCHUNK);
    // without row outputs only the tiles that hold a pair i < j are needed
    const int t_begin = a.rows ? c0 : max(c0, x0);
    if (t_begin >= c1) return;

    for (int b = tid; b < a.T * 256 + 2 * a.nbins; b += 256) cnt[b] = 0;  // visible after the first tile's barriers

    // this lane's 4 rows
    int ri[4], li[4];
    float rr[4];
    bool iv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ri[r] = x0 + 16 * wave + 4 * (lane >> 4) + r;
        iv[r] = ri[r] < a.b1;
        const int ic = min(ri[r], N - 1);
        li[r] = a.labels[ic];
        rr[r] = a.rinv[ic];
    }
    float sum_g[4], sum_i[4], bg[4], wg[4], bi[4];
    int bgj[4], wgj[4], bij[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sum_g[r] = sum_i[r] = 0.f;
        bg[r] = bi[r] = -INFINITY;
        wg[r] = INFINITY;
        bgj[r] = wgj[r] = bij[r] = -1;
    }
    uint32_t tot_g = 0, tot_i = 0;

    for (int t0 = t_begin; t0 < c1; t0 += MT) {
        f32x4_t acc[4];
        score_tile_prefetch(a.E, N, x0, a.E, N, t0, a.D, sXY, sXY + MT * LD, acc);
        int cj[4], lj[4];
        float rj[4];
        bool jv[4];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            cj[j4] = t0 + 16 * j4 + (lane & 15);
            jv[j4] = cj[j4] < c1;
            const int jc = min(cj[j4], N - 1);
            lj[j4] = a.labels[jc];
            rj[j4] = a.rinv[jc];
        }
        const bool upper = t0 + MT - 1 > x0;  // the tile holds pairs i < j
        float sv[16];
        uint32_t inc[16];  // 1: a genuine pair i < j, 1 << 16: an impostor pair i < j, 0: not counted
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4) {
                const float s = __fmul_rn(__fmul_rn(acc[j4][r], rr[r]), rj[j4]);
                const int j = cj[j4];
                const bool v = iv[r] && jv[j4];
                const bool gen = li[r] == lj[j4];
                if (a.rows && v && j != ri[r]) {
                    // a lane's columns ascend, so a strict comparison keeps the lowest j of equal scores
                    if (gen) {
                        sum_g[r] += s;
                        if (s > bg[r]) { bg[r] = s; bgj[r] = j; }
                        if (s < wg[r]) { wg[r] = s; wgj[r] = j; }
                    } else {
                        sum_i[r] += s;
                        if (s > bi[r]) { bi[r] = s; bij[r] = j; }
                    }
                }
                const bool pair = v && ri[r] < j;
                sv[4 * r + j4] = s;
                inc[4 * r + j4] = pair ? (gen ? 1u : 0x10000u) : 0u;
                if (pair) {
                    if (gen) ++tot_g; else ++tot_i;
                    if (a.hist) {
                        int bin = (int)floorf(__fmul_rn(__fsub_rn(s, a.lo), a.inv_w));
                        bin = min(max(bin, 0), a.nbins - 1);
                        atomicAdd(hist2 + (gen ? 0 : a.nbins) + bin, 1u);
                    }
                }
            }
        }
        if (upper) {
            // strict s > t; a chunk adds at most 16 tiles x 16 = 256 to either half of a thread's packed counter
            for (int t = 0; t < a.T; ++t) {
                const float th = a.thr[t];
                uint32_t c = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) c += sv[e] > th ? inc[e] : 0u;
                cnt[t * 256 + tid] += c;
            }
        }
    }

    // per-row partials of the chunk: the 16 lanes of a row in a fixed tree
    if (a.rows) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o <= 8; o <<= 1) {
                sum_g[r] += __shfl_xor(sum_g[r], o);
                sum_i[r] += __shfl_xor(sum_i[r], o);
                take_max(bg[r], bgj[r], __shfl_xor(bg[r], o), __shfl_xor(bgj[r], o));
                take_min(wg[r], wgj[r], __shfl_xor(wg[r], o), __shfl_xor(wgj[r], o));
                take_max(bi[r], bij[r], __shfl_xor(bi[r], o), __shfl_xor(bij[r], o));
            }
            if ((lane & 15) == 0 && iv[r]) {
                float* p = a.part + ((size_t)blockIdx.y * a.R + (ri[r] - a.b0)) * (PART_B / 4);
                *(float4*)p = make_float4(sum_g[r], sum_i[r], bg[r], wg[r]);
                *(float4*)(p + 4) = make_float4(bi[r], __int_as_float(bgj[r]), __int_as_float(wgj[r]),
                                                __int_as_float(bij[r]));
            }
        }
    }

    // totals: one 64-bit add per wave and class
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        tot_g += __shfl_xor(tot_g, o);
        tot_i += __shfl_xor(tot_i, o);
    }
    if (lane == 0) {
        if (tot_g) atomicAdd(a.totals, (unsigned long long)tot_g);
        if (tot_i) atomicAdd(a.totals + 1, (unsigned long long)tot_i);
    }
    __syncthreads();  // every thread's counters and histogram adds are in LDS
    for (int t = wave; t < a.T; t += 4) {
        uint32_t g = 0, i = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = cnt[t * 256 + 64 * k + lane];
            g += c & 0xffffu;
            i += c >> 16;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            g += __shfl_xor(g, o);
            i += __shfl_xor(i, o);
        }
        if (lane == 0) {
            if (g) atomicAdd(a.counts + 2 * t, (unsigned long long)g);
            if (i) atomicAdd(a.counts + 2 * t + 1, (unsigned long long)i);
        }
    }
    if (a.hist) {
        for (int b = tid; b < 2 * a.nbins; b += 256) {
            const uint32_t v = hist2[b];
            if (v) atomicAdd(a.hist + b, (unsigned long long)v);
        }
    }
}

// Row b0 + i: its chunk partials in ascending chunk order.
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ part, int b0, int b1, int nc,
                                                      float* __restrict__ row_score, int32_t* __restrict__ row_idx,
                                                      float* __restrict__ row_sum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (b0 + i >= b1) return;
    const size_t R = (size_t)((b1 - b0 + 63) / 64 * 64);
    float sg = 0.f, si = 0.f, bg = -INFINITY, wg = INFINITY, bi = -INFINITY;
    int bgj = -1, wgj = -1, bij = -1;
    for (int c = 0; c < nc; ++c) {
        const float* p = part + ((size_t)c * R + i) * (PART_B / 4);
        const float4 u = *(const float4*)p, w = *(const float4*)(p + 4);
        sg = c ? sg + u.x : u.x;
        si = c ? si + u.y : u.y;
        take_max(bg, bgj, u.z, __float_as_int(w.y));
        take_min(wg, wgj, u.w, __float_as_int(w.z));
        take_max(bi, bij, w.x, __float_as_int(w.w));
    }
    const size_t row = (size_t)(b0 + i);
    if (row_score) {
        row_score[3 * row] = bg; row_score[3 * row + 1] = wg; row_score[3 * row + 2] = bi;
        row_idx[3 * row] = bgj; row_idx[3 * row + 1] = wgj; row_idx[3 * row + 2] = bij;
    }
    if (row_sum) {
        row_sum[2 * row] = sg;
        row_sum[2 * row + 1] = si;
    }
}

}  // namespace

// The norms and one 64-row band of chunk partials.
size_t verify_min_workspace(int N) { return (size_t)pad64(N) * sizeof(float) + (size_t)MT * n_chunks(N) * PART_B; }

// Every row's partials where they are at most 256 MiB, else as many 64-row bands as fit in that.
size_t verify_workspace(int N) {
    const size_t band = (size_t)MT * n_chunks(N) * PART_B;
    const size_t all = (size_t)pad64(N) / MT;
    const size_t fit = std::max<size_t>(1, ((size_t)256 << 20) / band);
    return (size_t)pad64(N) * sizeof(float) + std::min(all, fit) * band;
}

hipError_t launch_verify_pairs(const float* E, int N, int D, const int32_t* labels, int normalize, const float* thresholds,
                               int T, uint64_t* counts, uint64_t* totals, uint64_t* hist, int nbins, float lo, float inv_w,
                               float* row_score, int32_t* row_idx, float* row_sum, void* ws, size_t ws_bytes,
                               hipStream_t s) {
    VerifyArgs a;
    a.E = E; a.N = N; a.D = D; a.labels = labels;
    a.rinv = (float*)ws;
    a.T = T;
    a.counts = (unsigned long long*)counts;
    a.totals = (unsigned long long*)totals;
    a.hist = (unsigned long long*)hist;
    a.nbins = hist ? nbins : 0;
    a.lo = lo; a.inv_w = inv_w;
    a.rows = row_score || row_sum;
    a.part = (float*)ws + pad64(N);
    for (int t = 0; t < FR_VERIFY_MAX_THRESHOLDS; ++t) a.thr[t] = t < T ? thresholds[t] : 0.f;
    const int nc = n_chunks(N);
    const size_t band = (size_t)MT * nc * PART_B;
    const size_t bands_fit = (ws_bytes - (size_t)pad64(N) * sizeof(float)) / band;  // >= 1: checked by the caller
    const int R = a.rows ? (int)std::min<size_t>(bands_fit * MT, (size_t)pad64(N)) : pad64(N);
    const int max_lds = (FR_VERIFY_MAX_THRESHOLDS * 256 + 2 * 2048) * (int)sizeof(uint32_t);
    if (hipError_t e = lds_opt_in((const void*)sweep_kernel, max_lds); e != hipSuccess) return e;
    const size_t lds = ((size_t)T * 256 + 2 * (size_t)a.nbins) * sizeof(uint32_t);
    hipLaunchKernelGGL(prep_kernel, dim3((N + 3) / 4), dim3(256), 0, s, E, N, D, normalize, (float*)ws,
                       (unsigned long long*)counts, T, (unsigned long long*)totals);
    for (int b0 = 0; b0 < N; b0 += R) {
        a.b0 = b0;
        a.b1 = std::min(N, b0 + R);
        a.R = pad64(a.b1 - b0);
        hipLaunchKernelGGL(sweep_kernel, dim3((a.b1 - b0 + MT - 1) / MT, nc), dim3(256), lds, s, a);
        if (a.rows)
            hipLaunchKernelGGL(combine_kernel, dim3((a.b1 - b0 + 255) / 256), dim3(256), 0, s, a.part, b0, a.b1, nc,
                               row_score, row_idx, row_sum);
    }
    return hipGetLastError();
}

}  // namespace fr
