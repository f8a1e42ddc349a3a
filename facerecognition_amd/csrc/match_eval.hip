// Labelled gallery evaluation: for probes P[B,D] with a known true gallery row each, the score of the
// true row, its 0-based rank in fr_match_topk's total order (score desc, index asc), and a histogram of
// every other (impostor) score -- without materialising the B x N score matrix.
//
// Replaces: notebook evaluate_arcface_kaggle.ipynb cells 15-19 (a [20387, 9343] f32 similarity matrix on the
// host, 760 MB, read for argmax / argsort[:, -5:] / sims[i, true_idx] / max(axis=1)) and the per-image
// loop of inference/evaluate.py:275-349.
//
// Scores are the exact f32 match path's, bit for bit: every output is the same v_mfma_f32_16x16x4f32
// sequence as in match.hip (k = 16 t16 + 4 (lane >> 4) + c, c = 0..3 per t16; the tile loops are
// score_tile.h's).  Two launches:
//   eval_true_kernel   one wave per 16 probes: a 16x16 tile whose B operand is the 16 probes' own true rows;
//                      the diagonal is true_score.  Also resets true_rank (0, or -1 for a true row outside
//                      the shard).
//   eval_p512_kernel   (D = 512) / eval_partial_kernel (other D): the p512_* ring pieces / score_tile_staged, as
//                      match_p512_kernel / match_partial_kernel -- 64 probes per block x one gallery
//                      split, 64-row tiles, the score tile in LDS -- with the top-k insert replaced by a
//                      compare-and-count against (true_score, true_idx) and an LDS histogram.  Counts are
//                      summed over splits with one integer add per (probe, split); the histogram (one u32
//                      copy per wave, so the 4 waves never contend for a bin) is flushed once per block with
//                      64-bit global adds.
#include "score_tile.h"
#include <float.h>
#include <limits.h>

#include <algorithm>

namespace fr {
using namespace tile;
namespace {

// True-row pre-pass.  Lane l holds probe (l & 15)'s and true row (l & 15)'s k-slice 4 (l >> 4) .. + 3 of every
// 16-float step, exactly the A / B fragments of the match kernels; D is walked in 64-float chunks with zeros
// past D as their staging does.  acc[r] = score(probe 4 (l >> 4) + r, true row of probe l & 15).
__global__ __launch_bounds__(64) void eval_true_kernel(const float* __restrict__ P, int B, const float* __restrict__ G,
                                                       int64_t N, int D, int64_t index_base,
                                                       const int32_t* __restrict__ true_idx,
                                                       float* __restrict__ true_score, int32_t* __restrict__ true_rank) {
    const int lane = threadIdx.x;
    const int p = blockIdx.x * 16 + (lane & 15);
    const int pc = min(p, B - 1);
    const int64_t tl = (int64_t)true_idx[pc] - index_base;
    const bool valid = tl >= 0 && tl < N;
    const float* pa = P + (size_t)pc * D;
    const float* gb = G + (size_t)(valid ? tl : 0) * D;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D; d0 += KC) {
#pragma unroll
        for (int t16 = 0; t16 < KC / 16; ++t16) {
            const int kof = d0 + 16 * t16 + 4 * (lane >> 4);
            float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f), b4 = a4;
            if (kof < D) {  // D % 4 == 0
                a4 = *(const float4*)(pa + kof);
                b4 = *(const float4*)(gb + kof);
            }
            mfma_k4(acc, a4, b4);
        }
    }
    const int r = (lane & 15) - 4 * (lane >> 4);  // the diagonal element of this lane, if it holds one
    if (r >= 0 && r < 4 && p < B) {
        const float v = r == 0 ? acc[0] : (r == 1 ? acc[1] : (r == 2 ? acc[2] : acc[3]));
        true_score[p] = valid ? v : -INFINITY;
        true_rank[p] = valid ? 0 : -1;
    }
}

struct EvalArgs {
    const float* P;
    int B;
    const float* G;
    int64_t N;
    int D;
    int64_t index_base;
    int64_t rows_per_split;
    const int32_t* true_idx;
    const float* true_score;
    int32_t* true_rank;
    unsigned long long* hist;  // null: no histogram
    int nbins;
    float lo, inv_w;
};

// This thread's probe (4 threads per probe, 16 tile columns each): what the epilogue compares against.
struct EvalProbe {
    float ts;   // true score (-inf: true row outside the shard)
    int tloc;   // true row, local to the shard (-1: outside)
    bool live;  // probe < B
    int cnt;    // rows better than the true row so far
};

__device__ __forceinline__ EvalProbe eval_probe_load(const EvalArgs& a, int p) {
    EvalProbe e;
    const int pc = min(p, a.B - 1);
    const int64_t tl = (int64_t)a.true_idx[pc] - a.index_base;
    e.tloc = (tl >= 0 && tl < a.N) ? (int)tl : -1;
    e.ts = a.true_score[pc];
    e.live = p < a.B;
    e.cnt = 0;
    return e;
}

// One 64 x 64 score tile (sS, row stride MG + 1) -> the count and this wave's histogram copy.  j0 = the
// tile's first row (local), lim = its valid rows.  The true row is skipped by index.
__device__ __forceinline__ void eval_tile(const float* sS, int my_p, int my_sub, int j0, int lim, EvalProbe& e,
                                          uint32_t* whist, int nbins, float lo, float inv_w) {
    const float* row = sS + my_p * (MG + 1) + my_sub * 16;
    const int jb = j0 + my_sub * 16;
    const int l = lim - my_sub * 16;
    float sv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) sv[i] = row[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const bool imp = (i < l) & (jb + i != e.tloc);
        e.cnt += (imp & better(sv[i], jb + i, e.ts, e.tloc)) ? 1 : 0;
        if (whist && imp && e.live) {
            int bin = (int)floorf(__fmul_rn(__fsub_rn(sv[i], lo), inv_w));
            bin = min(max(bin, 0), nbins - 1);
            atomicAdd(whist + bin, 1u);
        }
    }
}

// The block's results: the 4 sub-counts of each probe summed, one integer add per (probe, split); the 4
// wave histograms summed, one 64-bit add per non-empty bin.
__device__ __forceinline__ void eval_finish(const EvalArgs& a, const uint32_t* hist4, int p, int my_sub, EvalProbe& e) {
    int c = e.cnt;
    c += __shfl_xor(c, 1);
    c += __shfl_xor(c, 2);
    if (my_sub == 0 && e.live && e.tloc >= 0 && c) atomicAdd(a.true_rank + p, c);
    if (a.hist) {
        for (int b = threadIdx.x; b < a.nbins; b += 256) {
            const uint32_t v = hist4[b] + hist4[a.nbins + b] + hist4[2 * a.nbins + b] + hist4[3 * a.nbins + b];
            if (v) atomicAdd(a.hist + b, (unsigned long long)v);
        }
    }
}

// score_tile_staged (any D % 4 == 0) with the evaluation epilogue.
__global__ __launch_bounds__(256) void eval_partial_kernel(const EvalArgs a) {
    __shared__ __attribute__((aligned(16))) float sPG[2 * MP * LD];
    __shared__ float sS[MP * (MG + 1)];
    extern __shared__ __attribute__((aligned(16))) char dyn[];  // [4][nbins] u32 wave histograms
    float* sP = sPG;
    float* sG = sPG + MP * LD;
    uint32_t* hist4 = (uint32_t*)dyn;

    const int tid = threadIdx.x, wave = tid >> 6;
    const int p0 = blockIdx.x * MP;
    const int64_t g_begin = (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t g_end = std::min<int64_t>(g_begin + a.rows_per_split, a.N);

    const int my_p = tid >> 2, my_sub = tid & 3;
    EvalProbe e = eval_probe_load(a, p0 + my_p);
    if (a.hist)
        for (int b = tid; b < 4 * a.nbins; b += 256) hist4[b] = 0;  // visible after the first tile's barriers
    uint32_t* whist = a.hist ? hist4 + wave * a.nbins : nullptr;

    for (int64_t t0 = g_begin; t0 < g_end; t0 += MG) {
        f32x4_t acc[4];
        score_tile_staged(a.P, a.B, p0, a.G, g_end, t0, a.D, sP, sG, acc);
        store_score_tile(sS, acc);
        __syncthreads();
        eval_tile(sS, my_p, my_sub, (int)t0, (int)std::min<int64_t>(MG, g_end - t0), e, whist, a.nbins, a.lo, a.inv_w);
        __syncthreads();
    }
    eval_finish(a, hist4, p0 + my_p, my_sub, e);
}

// D = 512: the register-probe, LDS-DMA ring of score_tile.h (the p512_* pieces) with the evaluation epilogue.
// LDS: [4 chunks 64 KB][score tile 16.6 KB][4 wave histograms <= 32 KB].
__global__ __launch_bounds__(256, 1) void eval_p512_kernel(const EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [NBUF chunks][sS][4][nbins]
    float* sS = (float*)(smem + NBUF * CHUNK_B);
    uint32_t* hist4 = (uint32_t*)(smem + P512_LDS);

    const int tid = threadIdx.x, wave = tid >> 6;
    const int p0 = blockIdx.x * MP;
    const int64_t g_begin = (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t g_end = std::min<int64_t>(g_begin + a.rows_per_split, a.N);
    const int rows = (int)(g_end - g_begin);  // <= 64 tiles of 64 rows (the launcher's bound)
    const int ntiles = (rows + MG - 1) / MG;

    const int my_p = tid >> 2, my_sub = tid & 3;
    EvalProbe e = eval_probe_load(a, p0 + my_p);
    if (a.hist)
        for (int b = tid; b < 4 * a.nbins; b += 256) hist4[b] = 0;  // visible after the first chunk's barrier
    uint32_t* whist = a.hist ? hist4 + wave * a.nbins : nullptr;

    float4 pa[D512 / 16];
    p512_probes_load(a.P, a.B, p0, pa);
    asm volatile("" : "+v"(e.ts), "+v"(e.tloc));  // the probe's own loads are waited for there too
    p512_probes_mask(a.B, p0, pa);
    const P512Ring ring = p512_ring_start(a.G + (size_t)g_begin * D512, rows, smem);

    for (int tl = 0; tl < ntiles; ++tl) {
        f32x4_t acc[4];
        p512_tile(ring, pa, smem, tl, acc);
        // scores -> LDS (its previous readers are 8 barriers back), then the count and the histogram
        store_score_tile(sS, acc);
        lds_barrier();
        eval_tile(sS, my_p, my_sub, (int)(g_begin + (int64_t)tl * MG), min(MG, rows - tl * MG), e, whist, a.nbins, a.lo,
                  a.inv_w);
    }
    p512_ring_drain();
    // all histogram adds are done
    __syncthreads();
    eval_finish(a, hist4, p0 + my_p, my_sub, e);
}

}  // namespace

// The main pass's split: match_split_plan's for the exact top-5 (the p512 plan at D = 512).
void match_eval_plan(int B, int64_t N, int D, int* n_split, int64_t* rows_per_split) {
    match_split_plan(B, N, D, 5, n_split, rows_per_split);
}

// true_score / true_rank [B]; hist [nbins] u64 or null (added to).  N < 2^31.
hipError_t launch_match_eval(const float* P, int B, const float* G, int64_t N, int D, int64_t index_base,
                             const int32_t* true_idx, float* true_score, int32_t* true_rank,
                             unsigned long long* hist, int nbins, float lo, float inv_w, hipStream_t s) {
    if (B <= 0 || N <= 0 || N > 0x7fffffff || D <= 0 || D % 4 != 0 || (hist && (nbins < 1 || nbins > 2048)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(eval_true_kernel, dim3((B + 15) / 16), dim3(64), 0, s, P, B, G, N, D, index_base, true_idx,
                       true_score, true_rank);
    EvalArgs a;
    a.P = P; a.B = B; a.G = G; a.N = N; a.D = D; a.index_base = index_base;
    a.true_idx = true_idx; a.true_score = true_score; a.true_rank = true_rank;
    a.hist = hist; a.nbins = hist ? nbins : 0; a.lo = lo; a.inv_w = inv_w;
    int n_split;
    match_eval_plan(B, N, D, &n_split, &a.rows_per_split);
    const dim3 grid((B + MP - 1) / MP, n_split);
    const size_t hist_b = (size_t)4 * a.nbins * sizeof(uint32_t);
    if (D == D512 && a.rows_per_split <= P512_MAX_TILES * MG) {  // (32-bit DMA offsets: at most 64 tiles per split)
        const int max_lds = P512_LDS + 4 * 2048 * (int)sizeof(uint32_t);
        if (hipError_t e = lds_opt_in((const void*)eval_p512_kernel, max_lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(eval_p512_kernel, grid, dim3(256), P512_LDS + hist_b, s, a);
    } else {
        const int max_lds = 4 * 2048 * (int)sizeof(uint32_t);  // static 51.4 KB + up to 32 KB of histograms
        if (hipError_t e = lds_opt_in((const void*)eval_partial_kernel, max_lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(eval_partial_kernel, grid, dim3(256), hist_b, s, a);
    }
    return hipGetLastError();
}

}  // namespace fr
