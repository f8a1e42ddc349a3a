// Exact f32 score tiles: the one place the v_mfma_f32_16x16x4_f32 tile loops are written.
//
// Every exact score in the library -- match, evaluation, range search, verification, triplet mining, the ArcFace
// loss -- is the same fmaf chain per output, whichever kernel computed it: a 64 x 64 tile of X rows . Y rows, four
// waves of 16 X rows each, the inner dimension walked in 64-float chunks and, per chunk, in four 16-float steps
// t16 in which lane l multiplies elements k = 16 t16 + 4 (l >> 4) + c, c = 0..3 in that order (mfma_k4).
//     acc[j][r] = score(X row 16 wave + 4 (lane >> 4) + r, Y row 16 j + (lane & 15))
// Three loops produce that sequence; they differ only in how the operands reach the MFMAs:
//   score_tile_staged    any D % 4 == 0; both operands through LDS, loaded and stored chunk by chunk
//                        (match_partial_kernel, match_scores_kernel, eval_partial_kernel, range_partial_kernel)
//   score_tile_prefetch  any D % 4 == 0; as above with the next chunk's global loads issued under the current
//                        chunk's MFMAs (arcmargin.hip, triplet.hip, verify.hip)
//   p512_tile            D = 512; the X fragments in registers for a whole gallery split, the Y rows LDS-DMA'd
//                        through a 4-chunk ring, with the p512_* pieces around it (eval_p512_kernel,
//                        range_p512_kernel; match_p512_kernel keeps a copy of this loop, for its speed on
//                        short splits: match.hip)
// A new consumer of exact scores includes this header; it does not copy a loop.  Device code only, no host state.
#pragma once
#include "kernels.h"
#include "lds_dma.h"

namespace fr {
namespace tile {  // consumers say `using namespace tile;` inside namespace fr

constexpr int MT = 64;       // rows per tile, both sides
constexpr int MP = MT;       // (the match kernels' names: probes per block,
constexpr int MG = MT;       //  gallery rows per tile)
constexpr int KC = 64;       // inner-dimension chunk (floats)
constexpr int LD = KC + 4;   // row stride of a staged operand tile in LDS
constexpr int SLD = MT + 1;  // row stride of a score tile in LDS

// One 16-float step of one accumulator: x y z w.
__device__ __forceinline__ void mfma_k4(f32x4_t& acc, const float4& a4, const float4& b4) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc, 0, 0, 0);
}

// Accumulators -> the 64 x 64 score tile sS (row stride SLD).
__device__ __forceinline__ void store_score_tile(float* sS, const f32x4_t (&acc)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) sS[(16 * wave + 4 * (lane >> 4) + r) * SLD + 16 * j + (lane & 15)] = acc[j][r];
}

// sum_k x[k]^2 of one row by one wave, in a fixed order: lane l adds x y z w of the float4s at 4 l, 4 l + 256, ...,
// then a butterfly from 32 down to 1.  Every lane gets the sum.
__device__ __forceinline__ float row_sqsum(const float* __restrict__ x, int D) {
    const int lane = threadIdx.x & 63;
    float ss = 0.f;
    for (int d = 4 * lane; d < D; d += 256) {
        const float4 v = *(const float4*)(x + d);
        ss += v.x * v.x;
        ss += v.y * v.y;
        ss += v.z * v.z;
        ss += v.w * v.w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o);
    return ss;
}

// One staged 64-float chunk (sX, sY: [64][LD]) into the accumulators.
__device__ __forceinline__ void chunk_mfma(const float* sX, const float* sY, f32x4_t (&acc)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t16 = 0; t16 < KC / 16; ++t16) {
        const int kof = 16 * t16 + 4 * (lane >> 4);
        const float4 a4 = *(const float4*)(sX + (16 * wave + (lane & 15)) * LD + kof);
#pragma unroll
        for (int j = 0; j < 4; ++j) mfma_k4(acc[j], a4, *(const float4*)(sY + (16 * j + (lane & 15)) * LD + kof));
    }
}

// acc = X[x0 ..][:] . Y[t0 ..][:]^T; rows past rx / ry and columns past D read as zero.  Per chunk: load, store to
// sX / sY, barrier, MFMAs, barrier (so sX / sY are free again on return).  IX / IY: the row-number type of either
// side (int or int64_t), so that a kernel whose rows fit an int keeps 32-bit compares and address arithmetic.
template <class IX, class IY>
__device__ __forceinline__ void score_tile_staged(const float* __restrict__ X, IX rx, IX x0, const float* __restrict__ Y,
                                                  IY ry, IY t0, int D, float* sX, float* sY, f32x4_t (&acc)[4]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D; d0 += KC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int row = q >> 4, c4 = (q & 15) * 4;
            float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), yv = xv;
            if (x0 + row < rx && d0 + c4 < D) xv = *(const float4*)(X + (size_t)(x0 + row) * D + d0 + c4);
            if (t0 + row < ry && d0 + c4 < D) yv = *(const float4*)(Y + (size_t)(t0 + row) * D + d0 + c4);
            *(float4*)(sX + row * LD + c4) = xv;
            *(float4*)(sY + row * LD + c4) = yv;
        }
        __syncthreads();
        chunk_mfma(sX, sY, acc);
        __syncthreads();
    }
}

// score_tile_staged with chunk d0 + KC loaded into registers while chunk d0's MFMAs run: the same values through
// the same MFMAs, so the same bits.  Kept apart because the two are timed differently.
template <class IX, class IY>
__device__ __forceinline__ void score_tile_prefetch(const float* __restrict__ X, IX rx, IX x0, const float* __restrict__ Y,
                                                    IY ry, IY t0, int D, float* sX, float* sY, f32x4_t (&acc)[4]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float4 xv[4], yv[4];
    auto load = [&](int d0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int row = q >> 4, c4 = (q & 15) * 4;
            xv[i] = yv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (x0 + row < rx && d0 + c4 < D) xv[i] = *(const float4*)(X + (size_t)(x0 + row) * D + d0 + c4);
            if (t0 + row < ry && d0 + c4 < D) yv[i] = *(const float4*)(Y + (size_t)(t0 + row) * D + d0 + c4);
        }
    };
    load(0);
    for (int d0 = 0; d0 < D; d0 += KC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int row = q >> 4, c4 = (q & 15) * 4;
            *(float4*)(sX + row * LD + c4) = xv[i];
            *(float4*)(sY + row * LD + c4) = yv[i];
        }
        __syncthreads();
        if (d0 + KC < D) load(d0 + KC);
        chunk_mfma(sX, sY, acc);
        __syncthreads();
    }
}

// ---- D = 512: the register-probe, LDS-DMA ring sweep ------------------------------------------------------------
// Each wave keeps its 16 probes' A fragments in registers for the whole split (32 float4 per lane, loaded once), so
// only gallery rows move through LDS: 64-row x 64-float chunks (256-B rows, 16-B slots XOR-swizzled with the row:
// conflict-free fragment reads) LDS-DMA'd three chunks ahead into a 4-buffer ring, counted vmcnt waits and one
// LDS-only barrier per chunk.  (Staging both operands per chunk through registers behind full barriers, even with a
// register prefetch one chunk ahead, left each block one 16-KB load in flight: 74 us at 256 x 10k, latency bound.)
constexpr int D512 = 512;
constexpr int NBUF = 4;                              // chunk ring depth (3 chunks in flight)
constexpr int CHUNK_B = MG * KC * 4;                 // 16384
constexpr int P512_LDS = NBUF * CHUNK_B + MP * SLD * 4;  // [NBUF chunks][score tile]
constexpr int P512_MAX_TILES = 64;                   // per split: the DMA offsets are 32-bit

// The ring moves by dma16_asm (lds_dma.h): p512_tile's own counted waits cover it.
//
// A kernel's sweep of one gallery split is put together from the pieces below, in this order (eval_p512_kernel is
// the plainest example):
//     float4 pa[D512 / 16];
//     p512_probes_load(P, B, p0, pa);   // probe fragments into registers, then s_waitcnt vmcnt(0)
//     asm volatile("" : "+v"(x));       // pin what the kernel itself loaded from global memory before (below)
//     p512_probes_mask(B, p0, pa);      // zero the probes past B
//     const P512Ring ring = p512_ring_start(Gs, rows, smem);   // buffer resource of the split, ring primed
//     for (int tl = 0; tl < (rows + 63) / 64; ++tl) {
//         f32x4_t acc[4];
//         p512_tile(ring, pa, smem, tl, acc);                  // the chunk loop of tile tl
//         store_score_tile(sS, acc);    // sS = smem + NBUF CHUNK_B; its previous readers are 8 barriers back
//         lds_barrier();
//         ... the kernel's per-tile epilogue on sS; it needs no barrier of its own ...
//     }
//     p512_ring_drain();                // vmcnt(0): the trailing (out-of-range) DMAs have landed
// Between p512_probes_load's vmcnt(0) and p512_ring_drain the counted waits must see nothing but the ring's DMAs.
// Per-thread state that the kernel loaded from global memory earlier and that its epilogue uses is therefore pinned
// right after p512_probes_load (asm volatile("" : "+v"(x))): it is consumed at that wait, and the compiler places no
// wait of its own inside the counted region.  The epilogue may store to global memory (such stores only make
// vmcnt(8) stricter: match_range.hip's header) but must not load from it.

// pa[t] = P[p0 + 16 wave + (lane & 15)][16 t + 4 (lane >> 4) .. + 3], rows past the batch clamped to row B - 1; ends
// with the s_waitcnt vmcnt(0) that separates these loads from the DMA counts.
__device__ __forceinline__ void p512_probes_load(const float* __restrict__ P, int B, int p0, float4 (&pa)[D512 / 16]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = p0 + 16 * wave + (lane & 15);
    const float* src = P + (size_t)min(p, B - 1) * D512 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < D512 / 16; ++t) pa[t] = *(const float4*)(src + 16 * t);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the DMA wait counts see only DMAs
}

// rows past the batch: zero probes (no branch around the loads)
__device__ __forceinline__ void p512_probes_mask(int B, int p0, float4 (&pa)[D512 / 16]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float z = p0 + 16 * wave + (lane & 15) < B ? 1.f : 0.f;
#pragma unroll
    for (int t = 0; t < D512 / 16; ++t) pa[t] = make_float4(pa[t].x * z, pa[t].y * z, pa[t].z * z, pa[t].w * z);
}

// The split's rows as a buffer resource (rows past the split read 0: out of range) and the ring's LDS address.
struct P512Ring {
    v4i32 gr;
    uint32_t smem_base;
    // chunk c = (tile c / 8, floats 64 (c % 8) ..) into ring buffer c % NBUF: wave w issues pieces w + 4u,
    // piece q = rows 4q .. 4q + 3, lane -> row 4q + (lane >> 4), slot lane & 15 = column group
    // (lane & 15) ^ (row & 15).  Chunks past the split are issued anyway (all out of range) so that every
    // wait count is the same.
    __device__ __forceinline__ void issue_chunk(int c) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int t = c >> 3, d0 = (c & 7) * KC;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = wave + 4 * u, row = 4 * q + (lane >> 4), g = (lane & 15) ^ (row & 15);
            const uint32_t off = (uint32_t)((t * MG + row) * (D512 * 4) + (d0 + 4 * g) * 4);
            dma16_asm(gr, smem_base + (c % NBUF) * CHUNK_B + q * 1024, off);
        }
    }
};

// Gs: the split's first row; rows <= 64 P512_MAX_TILES; smem: the block's P512_LDS bytes of dynamic LDS.  Issues the
// first NBUF - 1 chunks.
__device__ __forceinline__ P512Ring p512_ring_start(const float* __restrict__ Gs, int rows, char* smem) {
    // buffer_rsrc_words' four words, written out: through the builder hipcc orders this scalar code differently
    const uint64_t gp = (uint64_t)Gs;
    const P512Ring ring = {{(int)(uint32_t)gp, (int)((gp >> 32) & 0xffff), rows * D512 * 4, RSRC_WORD3},
                           (uint32_t)(uintptr_t)smem};
#pragma unroll
    for (int c = 0; c < NBUF - 1; ++c) ring.issue_chunk(c);
    return ring;
}

// acc = the 64 x 64 scores of tile tl of the split: its 8 chunks out of the ring, chunk 8 tl + ch + 3 issued under
// chunk 8 tl + ch.
__device__ __forceinline__ void p512_tile(const P512Ring& ring, const float4 (&pa)[D512 / 16], const char* smem, int tl,
                                          f32x4_t (&acc)[4]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < D512 / KC; ++ch) {
        // chunk 8 tl + ch landed: at most 8 operations, so at most the two chunks issued after it (8 DMAs),
        // may be in flight
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        lds_barrier();
        ring.issue_chunk(8 * tl + ch + NBUF - 1);  // into the buffer read last chunk
        const char* buf = smem + (ch % NBUF) * CHUNK_B;
        // all 16 B fragments of the chunk first, one LDS wait (left alone the compiler waits before every
        // 4 MFMAs, and one wave per SIMD cannot hide that), then the MFMAs with the 4 accumulators
        // interleaved (a dependent f32 MFMA waits 40 cycles, the issue is 32): per accumulator the order
        // is unchanged, x y z w per t16
        float4 b4[KC / 16][4];
#pragma unroll
        for (int t16 = 0; t16 < KC / 16; ++t16) {
            const int slot = (4 * t16 + (lane >> 4)) ^ (lane & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) b4[t16][j] = *(const float4*)(buf + (16 * j + (lane & 15)) * 256 + slot * 16);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);  // nothing crosses the wait (MFMAs are not memory operations)
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
}

// the trailing (out-of-range) DMAs land: the ring's LDS may be reused after a barrier, the block may end
__device__ __forceinline__ void p512_ring_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

}  // namespace tile
}  // namespace fr
