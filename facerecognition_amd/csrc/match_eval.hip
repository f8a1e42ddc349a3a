// Labelled gallery evaluation: for probes P[B,D] with a known true gallery row each, the score of the
// true row, its 0-based rank in fr_match_topk's total order (score desc, index asc), and a histogram of
// every other (impostor) score -- without materialising the B x N score matrix.
//
// Replaces: notebook evaluate_arcface_kaggle.ipynb cells 15-19 (a [20387, 9343] f32 similarity matrix on the
// host, 760 MB, read for argmax / argsort[:, -5:] / sims[i, true_idx] / max(axis=1)) and the per-image
// loop of inference/evaluate.py:275-349.
//
// Scores are the exact f32 match path's, bit for bit: every output is the same v_mfma_f32_16x16x4f32
// sequence as in match.hip (k = 16 t16 + 4 (lane >> 4) + c, c = 0..3 per t16; the fragment code is restated
// here).  Two launches:
//   eval_true_kernel   one wave per 16 probes: a 16x16 tile whose B operand is the 16 probes' own true rows;
//                      the diagonal is true_score.  Also resets true_rank (0, or -1 for a true row outside
//                      the shard).
//   eval_p512_kernel   (D = 512) / eval_partial_kernel (other D): match_p512_kernel's / match_partial_kernel's
//                      main loop -- 64 probes per block x one gallery split, 64-row tiles, the score tile in
//                      LDS -- with the top-k insert replaced by a compare-and-count against (true_score,
//                      true_idx) and an LDS histogram.  Counts are summed over splits with one integer add
//                      per (probe, split); the histogram (one u32 copy per wave, so the 4 waves never
//                      contend for a bin) is flushed once per block with 64-bit global adds.
#include "kernels.h"
#include <float.h>
#include <limits.h>

#include <algorithm>

namespace fr {
namespace {

constexpr int MP = 64;  // probes per block
constexpr int MG = 64;  // gallery rows per tile
constexpr int KC = 64;  // D chunk (floats)
constexpr int LD = KC + 4;

// match.hip's comparator: score descending, index ascending
__device__ __forceinline__ bool better(float s1, int i1, float s2, int i2) {
    return s1 > s2 || (s1 == s2 && i1 < i2);
}

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
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc, 0, 0, 0);
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

// match_partial_kernel's main loop (any D % 4 == 0) with the evaluation epilogue.
__global__ __launch_bounds__(256) void eval_partial_kernel(const EvalArgs a) {
    __shared__ __attribute__((aligned(16))) float sPG[2 * MP * LD];
    __shared__ float sS[MP * (MG + 1)];
    extern __shared__ __attribute__((aligned(16))) char dyn[];  // [4][nbins] u32 wave histograms
    float* sP = sPG;
    float* sG = sPG + MP * LD;
    uint32_t* hist4 = (uint32_t*)dyn;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * MP;
    const int64_t g_begin = (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t g_end = std::min<int64_t>(g_begin + a.rows_per_split, a.N);
    const float* __restrict__ P = a.P;
    const float* __restrict__ G = a.G;
    const int B = a.B, D = a.D;

    const int my_p = tid >> 2, my_sub = tid & 3;
    EvalProbe e = eval_probe_load(a, p0 + my_p);
    if (a.hist)
        for (int b = tid; b < 4 * a.nbins; b += 256) hist4[b] = 0;  // visible after the first tile's barriers
    uint32_t* whist = a.hist ? hist4 + wave * a.nbins : nullptr;

    for (int64_t t0 = g_begin; t0 < g_end; t0 += MG) {
        f32x4_t acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        for (int d0 = 0; d0 < D; d0 += KC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = tid + 256 * i;
                const int row = q >> 4, c4 = (q & 15) * 4;
                float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), gv = pv;
                if (p0 + row < B && d0 + c4 < D) pv = *(const float4*)(P + (size_t)(p0 + row) * D + d0 + c4);
                if (t0 + row < g_end && d0 + c4 < D) gv = *(const float4*)(G + (size_t)(t0 + row) * D + d0 + c4);
                *(float4*)(sP + row * LD + c4) = pv;
                *(float4*)(sG + row * LD + c4) = gv;
            }
            __syncthreads();
#pragma unroll
            for (int t16 = 0; t16 < KC / 16; ++t16) {
                const int kof = 16 * t16 + 4 * (lane >> 4);
                const float4 a4 = *(const float4*)(sP + (16 * wave + (lane & 15)) * LD + kof);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 b4 = *(const float4*)(sG + (16 * j + (lane & 15)) * LD + kof);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc[j], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // acc[j][r] = score(probe 16 wave + 4 (lane >> 4) + r, gallery row t0 + 16 j + (lane & 15))
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sS[(16 * wave + 4 * (lane >> 4) + r) * (MG + 1) + 16 * j + (lane & 15)] = acc[j][r];
        __syncthreads();
        eval_tile(sS, my_p, my_sub, (int)t0, (int)std::min<int64_t>(MG, g_end - t0), e, whist, a.nbins, a.lo, a.inv_w);
        __syncthreads();
    }
    eval_finish(a, hist4, p0 + my_p, my_sub, e);
}

// D = 512: match_p512_kernel's main loop -- the wave's 16 probes' A fragments in registers for the whole
// split, gallery rows LDS-DMA'd in 64-row x 64-float chunks (16-B slots XOR-swizzled with the row) three
// chunks ahead into a 4-buffer ring, counted vmcnt waits, one LDS-only barrier per chunk -- with the
// evaluation epilogue.  LDS: [4 chunks 64 KB][score tile 16.6 KB][4 wave histograms <= 32 KB].
constexpr int D512 = 512;
constexpr int NBUF = 4;
constexpr int CHUNK_B = MG * KC * 4;  // 16384
constexpr int P512_LDS = NBUF * CHUNK_B + MP * (MG + 1) * 4;
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// 16-B LDS-DMA (lane l lands at lds_addr + 16 l); the compiler does not see the LDS write, the kernel's own
// counted waits cover it
typedef int v4i32 __attribute__((ext_vector_type(4)));
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma16_asm(const v4i32& rsrc, uint32_t lds_addr, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
                 :
                 : "v"(voff), "s"(rsrc), "s"(__builtin_amdgcn_readfirstlane(lds_addr))
                 : "memory", "m0");
}
#pragma clang diagnostic pop

__global__ __launch_bounds__(256, 1) void eval_p512_kernel(const EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [NBUF chunks][sS][4][nbins]
    float* sS = (float*)(smem + NBUF * CHUNK_B);
    uint32_t* hist4 = (uint32_t*)(smem + P512_LDS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * MP;
    const int64_t g_begin = (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t g_end = std::min<int64_t>(g_begin + a.rows_per_split, a.N);
    const int rows = (int)(g_end - g_begin);  // <= 64 tiles of 64 rows (the launcher's bound)
    const int ntiles = (rows + MG - 1) / MG;
    const int B = a.B;

    const int my_p = tid >> 2, my_sub = tid & 3;
    EvalProbe e = eval_probe_load(a, p0 + my_p);
    if (a.hist)
        for (int b = tid; b < 4 * a.nbins; b += 256) hist4[b] = 0;  // visible after the first chunk's barrier
    uint32_t* whist = a.hist ? hist4 + wave * a.nbins : nullptr;

    // the wave's A fragments: pa[t] = P[p0 + 16 wave + (lane & 15)][16 t + 4 (lane >> 4) .. + 3]
    float4 pa[D512 / 16];
    {
        const int p = p0 + 16 * wave + (lane & 15);
        const float* src = a.P + (size_t)min(p, B - 1) * D512 + 4 * (lane >> 4);
#pragma unroll
        for (int t = 0; t < D512 / 16; ++t) pa[t] = *(const float4*)(src + 16 * t);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the DMA wait counts below see only DMAs
        asm volatile("" : "+v"(e.ts), "+v"(e.tloc));      // (the probe's own loads are waited for here too)
        const float z = p < B ? 1.f : 0.f;  // rows past the batch: zero probes (no branch around the loads)
#pragma unroll
        for (int t = 0; t < D512 / 16; ++t) pa[t] = make_float4(pa[t].x * z, pa[t].y * z, pa[t].z * z, pa[t].w * z);
    }

    // the split's rows as a buffer resource: rows past the split read 0 (out of range)
    const uint64_t gp = (uint64_t)(a.G + (size_t)g_begin * D512);
    const v4i32 gr = {(int)(uint32_t)gp, (int)((gp >> 32) & 0xffff), rows * D512 * 4, 0x00020000};
    const uint32_t smem_base = (uint32_t)(uintptr_t)smem;
    // chunk c = (tile c / 8, floats 64 (c % 8) ..) into ring buffer c % NBUF: wave w issues pieces w + 4u,
    // piece q = rows 4q .. 4q + 3, lane -> row 4q + (lane >> 4), slot lane & 15 = column group
    // (lane & 15) ^ (row & 15).  Chunks past the split are issued anyway (all out of range) so that every
    // wait count is the same.
    auto issue_chunk = [&](int c) {
        const int t = c >> 3, d0 = (c & 7) * KC;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = wave + 4 * u, row = 4 * q + (lane >> 4), g = (lane & 15) ^ (row & 15);
            const uint32_t off = (uint32_t)((t * MG + row) * (D512 * 4) + (d0 + 4 * g) * 4);
            dma16_asm(gr, smem_base + (c % NBUF) * CHUNK_B + q * 1024, off);
        }
    };
#pragma unroll
    for (int c = 0; c < NBUF - 1; ++c) issue_chunk(c);

    for (int tl = 0; tl < ntiles; ++tl) {
        f32x4_t acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < D512 / KC; ++ch) {
            // chunk 8 tl + ch landed: only the two chunks issued after it (8 DMAs) may be in flight
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            lds_barrier();
            issue_chunk(8 * tl + ch + NBUF - 1);  // into the buffer read last chunk
            const char* buf = smem + (ch % NBUF) * CHUNK_B;
            // all 16 B fragments of the chunk first, one LDS wait, then the MFMAs with the 4 accumulators
            // interleaved; per accumulator the order is x y z w per t16
            float4 b4[KC / 16][4];
#pragma unroll
            for (int t16 = 0; t16 < KC / 16; ++t16) {
                const int slot = (4 * t16 + (lane >> 4)) ^ (lane & 15);
#pragma unroll
                for (int j = 0; j < 4; ++j) b4[t16][j] = *(const float4*)(buf + (16 * j + (lane & 15)) * 256 + slot * 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t16 = 0; t16 < KC / 16; ++t16) {
                const float4 a4 = pa[(KC / 16) * ch + t16];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4[t16][j].x, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4[t16][j].y, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4[t16][j].z, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4[t16][j].w, acc[j], 0, 0, 0);
            }
        }
        // scores -> LDS (its previous readers are 8 barriers back), then the count and the histogram
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sS[(16 * wave + 4 * (lane >> 4) + r) * (MG + 1) + 16 * j + (lane & 15)] = acc[j][r];
        lds_barrier();
        eval_tile(sS, my_p, my_sub, (int)(g_begin + (int64_t)tl * MG), min(MG, rows - tl * MG), e, whist, a.nbins, a.lo,
                  a.inv_w);
    }

    // the trailing (out-of-range) DMAs land before the block ends; all histogram adds are done
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
    if (D == D512 && a.rows_per_split <= 64 * MG) {  // (32-bit DMA offsets: at most 64 tiles per split)
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
