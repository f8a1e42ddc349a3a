// Threshold (range) search: for probes P[B,D], every gallery row whose score is >= thresh, as a CSR list
// (lims [B + 1] int64, scores / idx [lims[B]]) with each probe's hits in ascending gallery index -- without
// materialising the B x N score matrix, and with an optional per-probe lower index bound (`after`) that
// turns the same kernel into the self-join "all pairs i < j with score >= t".
//
// Replaces: the reference's decision rule as a query (known iff not best_score < threshold,
// inference/recognition_engine.py:286,323) over every identity instead of the best five; faiss
// IndexFlatIP.range_search, which keeps score > radius (strict) where this keeps score >= thresh (the
// reference's rule); and the N x N host matrix a duplicate-prototype scan of DatabaseBuilder's gallery needs.
//
// Scores are the exact f32 match path's, bit for bit: every output is the same v_mfma_f32_16x16x4f32
// sequence as in match.hip / match_eval.hip (k = 16 t16 + 4 (lane >> 4) + c, c = 0..3 per t16; the tile
// loops are score_tile.h's).  Two passes over one split plan (match_split_plan's for the exact top-5) and a
// scan between them:
//   range_*_kernel<false>  count: 64 probes per block x one gallery split; one int32 per (probe, split)
//                          into the workspace ws [n_split][B], a plain store (no atomics, no order-dependent
//                          adds);
//   range_offsets_kernel,  ws in place to each (probe, split)'s start offset inside the probe's segment, and
//   range_scan_kernel      lims = exclusive prefix over probes of the per-probe totals (int64);
//   range_*_kernel<true>   fill: the tiles recomputed; a kept pair's position is lims[b] + ws[split][b] +
//                          hits in earlier tiles of the split + hits of the probe's lower column-group
//                          threads (quad shuffles) + hits in the thread's earlier columns.  Positions
//                          >= capacity are not written.
// A pair (probe b, local row j) is kept when score >= thresh, j is a valid row of the split, b < B and,
// with `after`, index_base + j > after[b].  The last three matter: probe rows past B are zero probes and
// rows past the split read as zeros, so both score 0.0, which passes any thresh <= 0.
//
// The D = 512 loop's counted waits and the fill pass's stores (the loop is score_tile.h's p512_tile; this
// paragraph is about what only this file adds to it).  The loop waits `s_waitcnt vmcnt(8)` for the
// chunk it is about to read: three chunks of 4 LDS-DMAs are in flight, so "at most 8 outstanding" means the
// oldest chunk has landed.  On gfx950 global stores count on the same counter.  The count is of outstanding
// operations, and a wave's loads retire in issue order among themselves; the fill pass's stores are issued
// after the DMAs of the chunks then in flight.  With s stores outstanding next to the 12 DMAs, vmcnt(8)
// leaves at most 8 operations outstanding in total, hence at most 8 DMAs, hence (in-order loads) only the
// youngest two chunks: the needed chunk has landed whatever the stores do.  Extra stores can only make the
// wait stricter (it may also wait for part of the next chunk), never looser, so the wait counts stay as they
// are; the cost is a possible stall after a tile with hits, which the timing in DESIGN.md bounds.  The fill
// pass issues no global load inside the loop (offsets and `after` are read before the first DMA wait).
#include "score_tile.h"
#include <limits.h>

#include <algorithm>

namespace fr {
using namespace tile;
namespace {

struct RangeArgs {
    const float* P;
    int B;
    const float* G;
    int64_t N;
    int D;
    int64_t index_base;
    int64_t rows_per_split;
    int n_split;
    float thresh;
    const int32_t* after;  // [B] global indices, or null
    int32_t* ws;           // [n_split][B]: counts (count pass), start offsets (fill pass)
    const int64_t* lims;   // fill pass
    float* scores;
    int32_t* idx;
    int64_t capacity;
};

// This thread's probe (4 threads per probe, 16 tile columns each).
struct RangeProbe {
    bool live;    // probe < B
    int after;    // keep local rows j > after (-1: all)
    int cnt;      // count pass: hits so far
    int64_t pos;  // fill pass: where the probe's next hit of this split goes
};

template <bool FILL>
__device__ __forceinline__ RangeProbe range_probe_load(const RangeArgs& a, int p) {
    RangeProbe e;
    const int pc = min(p, a.B - 1);
    e.live = p < a.B;
    e.after = -1;
    if (a.after) {
        const int64_t al = (int64_t)a.after[pc] - a.index_base;
        e.after = (int)std::min<int64_t>(std::max<int64_t>(al, -1), INT_MAX);
    }
    e.cnt = 0;
    e.pos = 0;
    if (FILL) e.pos = a.lims[pc] + a.ws[(size_t)blockIdx.y * a.B + pc];
    return e;
}

// One 64 x 64 score tile (sS, row stride MG + 1).  j0 = the tile's first row (local to the shard), lim = its
// valid rows.  The fill pass re-reads a kept score from LDS by its column (no dynamic register index).
template <bool FILL>
__device__ __forceinline__ void range_tile(const RangeArgs& a, const float* sS, int my_p, int my_sub, int j0, int lim,
                                           RangeProbe& e) {
    const float* row = sS + my_p * (MG + 1) + my_sub * 16;
    const int jb = j0 + my_sub * 16;
    const int l = lim - my_sub * 16;
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const bool keep = (i < l) & (row[i] >= a.thresh) & (jb + i > e.after);
        m |= keep ? (1u << i) : 0u;
    }
    if (!e.live) m = 0;
    const int c = __popc(m);
    if (!FILL) {
        e.cnt += c;
        return;
    }
    // hits of the quad's lower column groups, and of the whole quad
    const int c1 = __shfl_xor(c, 1);
    const int pair = c + c1;
    const int other = __shfl_xor(pair, 2);
    int64_t pos = e.pos + ((my_sub & 1) ? c1 : 0) + ((my_sub & 2) ? other : 0);
    e.pos += pair + other;
    while (m) {
        const int i = __ffs(m) - 1;
        m &= m - 1;
        if (pos < a.capacity) {
            a.scores[pos] = row[i];
            a.idx[pos] = (int32_t)(a.index_base + jb + i);
        }
        ++pos;
    }
}

// Count pass: the 4 sub-counts of each probe summed, one plain store per (probe, split).
__device__ __forceinline__ void range_finish_count(const RangeArgs& a, int p, int my_sub, const RangeProbe& e) {
    int c = e.cnt;
    c += __shfl_xor(c, 1);
    c += __shfl_xor(c, 2);
    if (my_sub == 0 && e.live) a.ws[(size_t)blockIdx.y * a.B + p] = c;
}

// score_tile_staged (any D % 4 == 0) with the range epilogue.
template <bool FILL>
__global__ __launch_bounds__(256) void range_partial_kernel(const RangeArgs a) {
    __shared__ __attribute__((aligned(16))) float sPG[2 * MP * LD];
    __shared__ float sS[MP * (MG + 1)];
    float* sP = sPG;
    float* sG = sPG + MP * LD;

    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * MP;
    const int64_t g_begin = (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t g_end = std::min<int64_t>(g_begin + a.rows_per_split, a.N);

    const int my_p = tid >> 2, my_sub = tid & 3;
    RangeProbe e = range_probe_load<FILL>(a, p0 + my_p);

    for (int64_t t0 = g_begin; t0 < g_end; t0 += MG) {
        f32x4_t acc[4];
        score_tile_staged(a.P, a.B, p0, a.G, g_end, t0, a.D, sP, sG, acc);
        store_score_tile(sS, acc);
        __syncthreads();
        range_tile<FILL>(a, sS, my_p, my_sub, (int)t0, (int)std::min<int64_t>(MG, g_end - t0), e);
        __syncthreads();
    }
    if (!FILL) range_finish_count(a, p0 + my_p, my_sub, e);
}

// D = 512: the register-probe, LDS-DMA ring of score_tile.h (the p512_* pieces) with the range epilogue; the fill
// pass's stores and the ring's counted waits: the file header.  LDS: [4 chunks 64 KB][score tile 16.6 KB].
template <bool FILL>
__global__ __launch_bounds__(256, 1) void range_p512_kernel(const RangeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [NBUF chunks][sS]
    float* sS = (float*)(smem + NBUF * CHUNK_B);

    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * MP;
    const int64_t g_begin = (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t g_end = std::min<int64_t>(g_begin + a.rows_per_split, a.N);
    const int rows = (int)(g_end - g_begin);  // <= 64 tiles of 64 rows (the launcher's bound)
    const int ntiles = (rows + MG - 1) / MG;

    const int my_p = tid >> 2, my_sub = tid & 3;
    RangeProbe e = range_probe_load<FILL>(a, p0 + my_p);

    float4 pa[D512 / 16];
    p512_probes_load(a.P, a.B, p0, pa);
    asm volatile("" : "+v"(e.after), "+v"(e.pos));  // the probe's own loads are waited for there too
    p512_probes_mask(a.B, p0, pa);
    const P512Ring ring = p512_ring_start(a.G + (size_t)g_begin * D512, rows, smem);

    for (int tl = 0; tl < ntiles; ++tl) {
        f32x4_t acc[4];
        p512_tile(ring, pa, smem, tl, acc);
        // scores -> LDS (its previous readers are 8 barriers back), then the range epilogue
        store_score_tile(sS, acc);
        lds_barrier();
        range_tile<FILL>(a, sS, my_p, my_sub, (int)(g_begin + (int64_t)tl * MG), min(MG, rows - tl * MG), e);
    }
    p512_ring_drain();
    if (!FILL) range_finish_count(a, p0 + my_p, my_sub, e);
}

// The scan, in two launches.  range_offsets_kernel, one thread per probe: ws [n_split][B] counts -> each split's
// start offset inside its probe's segment, in place, and the probe's total into lims[b + 1].  range_scan_kernel,
// one block: lims[0] = 0 and lims[1 .. B] to their inclusive prefix, thread t owning the elements
// [t per, (t + 1) per).  Integer adds only, so the result does not depend on any order.
__global__ __launch_bounds__(256) void range_offsets_kernel(int32_t* __restrict__ ws, int B, int n_split,
                                                            int64_t* __restrict__ lims) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int32_t off = 0;  // <= N < 2^31
    for (int s = 0; s < n_split; ++s) {
        const int32_t c = ws[(size_t)s * B + b];
        ws[(size_t)s * B + b] = off;
        off += c;
    }
    lims[b + 1] = off;
}

constexpr int SCAN_T = 1024;
__global__ __launch_bounds__(SCAN_T) void range_scan_kernel(int B, int64_t* __restrict__ lims) {
    __shared__ int64_t part[SCAN_T];
    const int tid = threadIdx.x;
    const int per = (B + SCAN_T - 1) / SCAN_T;
    const int b0 = min(B, tid * per), b1 = min(B, b0 + per);
    int64_t sum = 0;
    for (int b = b0; b < b1; ++b) sum += lims[b + 1];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {  // inclusive Hillis-Steele scan of the threads' sums
        const int64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;
    for (int b = b0; b < b1; ++b) {
        run += lims[b + 1];
        lims[b + 1] = run;
    }
    if (tid == 0) lims[0] = 0;
}

template <bool FILL>
hipError_t launch_range_pass(const RangeArgs& a, hipStream_t s) {
    const dim3 grid((a.B + MP - 1) / MP, a.n_split);
    if (a.D == D512 && a.rows_per_split <= P512_MAX_TILES * MG) {  // (32-bit DMA offsets: at most 64 tiles per split)
        if (hipError_t e = lds_opt_in((const void*)range_p512_kernel<FILL>, P512_LDS); e != hipSuccess) return e;
        hipLaunchKernelGGL(range_p512_kernel<FILL>, grid, dim3(256), P512_LDS, s, a);
    } else {
        hipLaunchKernelGGL(range_partial_kernel<FILL>, grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

bool range_args_ok(int B, int64_t N, int D) { return B > 0 && N > 0 && N <= 0x7fffffff && D > 0 && D % 4 == 0; }

}  // namespace

// The passes' split: match_split_plan's for the exact top-5 (the p512 plan at D = 512), as match_eval's.
void match_range_plan(int B, int64_t N, int D, int* n_split, int64_t* rows_per_split) {
    match_split_plan(B, N, D, 5, n_split, rows_per_split);
}

size_t match_range_workspace(int B, int64_t N, int D) {
    if (!range_args_ok(B, N, D)) return 0;
    int n_split;
    int64_t rps;
    match_range_plan(B, N, D, &n_split, &rps);
    return (size_t)B * n_split * sizeof(int32_t);
}

hipError_t launch_match_range_count(const float* P, int B, const float* G, int64_t N, int D, int64_t index_base,
                                    float thresh, const int32_t* after, int32_t* ws, int64_t* lims, hipStream_t s) {
    if (!range_args_ok(B, N, D)) return hipErrorInvalidValue;
    RangeArgs a = {};
    a.P = P; a.B = B; a.G = G; a.N = N; a.D = D; a.index_base = index_base;
    a.thresh = thresh; a.after = after; a.ws = ws;
    match_range_plan(B, N, D, &a.n_split, &a.rows_per_split);
    if (hipError_t e = launch_range_pass<false>(a, s); e != hipSuccess) return e;
    hipLaunchKernelGGL(range_offsets_kernel, dim3((B + 255) / 256), dim3(256), 0, s, ws, B, a.n_split, lims);
    hipLaunchKernelGGL(range_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, B, lims);
    return hipGetLastError();
}

hipError_t launch_match_range_fill(const float* P, int B, const float* G, int64_t N, int D, int64_t index_base,
                                   float thresh, const int32_t* after, const int32_t* ws, const int64_t* lims,
                                   float* scores, int32_t* idx, int64_t capacity, hipStream_t s) {
    if (!range_args_ok(B, N, D) || capacity < 0) return hipErrorInvalidValue;
    RangeArgs a = {};
    a.P = P; a.B = B; a.G = G; a.N = N; a.D = D; a.index_base = index_base;
    a.thresh = thresh; a.after = after; a.ws = const_cast<int32_t*>(ws); a.lims = lims;
    a.scores = scores; a.idx = idx; a.capacity = capacity;
    match_range_plan(B, N, D, &a.n_split, &a.rows_per_split);
    return launch_range_pass<true>(a, s);
}

}  // namespace fr
