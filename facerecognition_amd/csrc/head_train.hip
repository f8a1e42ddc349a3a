// The embedding head in training mode, forward and backward (DESIGN.md §4 "Head training"; formulas in
// include/frhip.h "Head training"): input BN -> dropout -> Linear -> output BN on caller-owned f32 buffers.
//
// Replaces: models/arcface/arcface_model.py:154-159, 191-196 (bn1 -> dropout -> fc -> bn2 and autograd's copies of
// every intermediate), IResNet100's bn2 -> flatten -> fc -> features, FaceNet's dropout -> last_linear -> last_bn.
//
// The Linear's input A = dropout(BN(X)) is never stored: head_a4 recomputes four elements of it from X, the saved
// statistics and one Philox4x32-10 block wherever a tile of it is staged into LDS (forward product, dW product).
// Products are exact f32 on v_mfma_f32_16x16x4f32, 64 x 64 tiles, the inner dimension staged through LDS in 64s.
//   bn_cols_kernel   S = 1 statistics of 16 columns x 16 row groups per block (two passes), the running update,
//                    and for the output BN also Y
//   bn_chan_kernel   S > 1 statistics, one block per channel
//   fwd_gemm_kernel  64 rows x 64 outputs x one K split -> partial [split][B][N]; optionally writes A
//   fwd_merge_kernel partials in split order + bias -> Z
//   bn2_bwd_kernel   dgamma2, dbeta2, dZ (workspace) and dbias per column
//   bwd_gemm_kernel  T = true: dW = dZ^T A (one owner per element); T = false: dA = dZ W, then dH = dA m / (1 - p) in
//                    the epilogue, stored only when dX is wanted, and the tile's column sums of dH and dH x^
//   bn1_bwd_kernel   column sums in (row tile, s) order -> dgamma1, dbeta1
//   dx_kernel        dH -> dX in place
// No float atomics; every sum runs in an order fixed by (B, K, S, N).
#include "kernels.h"

#include <algorithm>

namespace fr {
namespace {

constexpr int MT = 64;  // rows per tile, both sides
constexpr int KC = 64;  // inner chunk (floats)
constexpr int LD = KC + 4;
constexpr int SLD = MT + 1;

// Philox4x32-10 (Random123: multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85).
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// The four generator words of elements i .. i + 3 (i % 4 == 0) of the [B][K] mask.
__device__ __forceinline__ uint4 mask_words(const HeadArgs& a, uint64_t i) {
    const uint64_t blk = i >> 2;
    return philox4x32_10(make_uint4((uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)a.offset, (uint32_t)(a.offset >> 32)),
                         make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32)));
}

// A[b][k .. k + 3] (k % 4 == 0): the input BN's affine on x^, then the dropout mask.
__device__ __forceinline__ float4 head_a4(const HeadArgs& a, int64_t b, int k) {
    float4 v = *(const float4*)(a.X + (size_t)b * a.K + k);
    float* e = (float*)&v;
    if (a.gamma1) {
        int c = k / a.S, rem = k - c * a.S;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (rem == a.S) {
                rem = 0;
                ++c;
            }
            e[j] = fmaf(a.gamma1[c], xhat(e[j], a.mean1[c], a.rstd1[c]), a.beta1[c]);
            ++rem;
        }
    }
    if (a.dropout) {
        const uint4 r = mask_words(a, (uint64_t)b * a.K + k);
        v.x = r.x >= a.thresh ? __fmul_rn(v.x, a.keep_scale) : 0.f;
        v.y = r.y >= a.thresh ? __fmul_rn(v.y, a.keep_scale) : 0.f;
        v.z = r.z >= a.thresh ? __fmul_rn(v.z, a.keep_scale) : 0.f;
        v.w = r.w >= a.thresh ? __fmul_rn(v.w, a.keep_scale) : 0.f;
    }
    return v;
}

// The sum of one value per thread in a fixed tree; every thread gets it.  red: 256 floats.
__device__ __forceinline__ float block_sum256(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

struct BnOut {
    float *rm, *rv;       // running statistics (read; written with batch statistics)
    float *mean, *rstd;   // what the BN normalises with
    float eps, momentum;
    bool batch;
};

// mean and var of one channel -> running update, mean, rstd (one thread per channel calls this)
__device__ __forceinline__ void bn_finish(const BnOut& o, int c, float mean, float var, float n) {
    if (o.batch) {
        o.rm[c] = (1.f - o.momentum) * o.rm[c] + o.momentum * mean;
        o.rv[c] = (1.f - o.momentum) * o.rv[c] + o.momentum * (var * (n / (n - 1.f)));
    }
    o.mean[c] = mean;
    o.rstd[c] = __fdiv_rn(1.f, __fsqrt_rn(var + o.eps));
}

// BN over the rows of M [R][C] (S = 1): 16 columns per block, row r belongs to group r % 16.
template <bool WRITE_Y>
__global__ __launch_bounds__(256) void bn_cols_kernel(const float* __restrict__ M, int64_t R, int C, const BnOut o,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ Y) {
    __shared__ float red[16 * 17];
    const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool live = c < C;
    const int cc = live ? c : C - 1;
    float mean, var;
    if (o.batch) {
        const float n = (float)R;
        float s = 0.f;
        if (live)
            for (int64_t r = g; r < R; r += 16) s += M[(size_t)r * C + c];
        mean = __fdiv_rn(col_sum16(s, red), n);
        float q = 0.f;
        if (live)
            for (int64_t r = g; r < R; r += 16) {
                const float d = M[(size_t)r * C + c] - mean;
                q = fmaf(d, d, q);
            }
        var = __fdiv_rn(col_sum16(q, red), n);
    } else {
        mean = o.rm[cc];
        var = o.rv[cc];
    }
    if (live && g == 0) bn_finish(o, c, mean, var, (float)R);
    if (WRITE_Y && live) {
        const float rstd = __fdiv_rn(1.f, __fsqrt_rn(var + o.eps));
        const float ga = gamma[c], be = beta[c];
        for (int64_t r = g; r < R; r += 16) Y[(size_t)r * C + c] = fmaf(ga, xhat(M[(size_t)r * C + c], mean, rstd), be);
    }
}

// Input BN with S > 1 and batch statistics: one block per channel over its B S elements, element j = b S + s to
// thread j % 256.
__global__ __launch_bounds__(256) void bn_chan_kernel(const float* __restrict__ X, int64_t B, int K, int S, const BnOut o) {
    __shared__ float red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t n = B * S;
    const float nf = (float)n;
    const float* x = X + (size_t)c * S;
    const int sb = 256 / S, ss = 256 % S;
    float mean = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        int64_t b = tid / S;
        int s = tid % S;
        float acc = 0.f;
        for (int64_t j = tid; j < n; j += 256) {
            const float v = x[(size_t)b * K + s];
            if (pass == 0) {
                acc += v;
            } else {
                const float d = v - mean;
                acc = fmaf(d, d, acc);
            }
            b += sb;
            s += ss;
            if (s >= S) {
                s -= S;
                ++b;
            }
        }
        const float tot = __fdiv_rn(block_sum256(acc, red), nf);
        if (pass == 0) mean = tot;
        else if (tid == 0) bn_finish(o, c, mean, tot, nf);
    }
}

// part[z][b][n] = sum over K split z of A[b][k] W[n][k].  Block (x, y, z) = (64-row tile, 64-output tile, split);
// the blocks of output tile 0 also write their part of A.
__global__ __launch_bounds__(256) void fwd_gemm_kernel(const HeadArgs a, int k_per_split, float* __restrict__ part,
                                                       float* __restrict__ A_out) {
    __shared__ __attribute__((aligned(16))) float sX[MT * LD];
    __shared__ __attribute__((aligned(16))) float sY[MT * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * MT;
    const int n0 = blockIdx.y * MT;
    const int k_begin = blockIdx.z * k_per_split;
    const int k_end = std::min(a.K, k_begin + k_per_split);
    const bool write_a = A_out != nullptr && blockIdx.y == 0;
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // chunk d0 + KC is loaded into registers while chunk d0's MFMAs run
    float4 xv[4], yv[4];
    auto load = [&](int d0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int row = q >> 4, c4 = (q & 15) * 4;
            xv[i] = yv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b0 + row < a.B && d0 + c4 < a.K) {
                xv[i] = head_a4(a, b0 + row, d0 + c4);
                if (write_a) *(float4*)(A_out + (size_t)(b0 + row) * a.K + d0 + c4) = xv[i];
            }
            if (n0 + row < a.N && d0 + c4 < a.K) yv[i] = *(const float4*)(a.W + (size_t)(n0 + row) * a.K + d0 + c4);
        }
    };
    load(k_begin);
    for (int d0 = k_begin; d0 < k_end; d0 += KC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int row = q >> 4, c4 = (q & 15) * 4;
            *(float4*)(sX + row * LD + c4) = xv[i];
            *(float4*)(sY + row * LD + c4) = yv[i];
        }
        __syncthreads();
        if (d0 + KC < k_end) load(d0 + KC);
#pragma unroll
        for (int t16 = 0; t16 < KC / 16; ++t16) {
            const int kof = 16 * t16 + 4 * (lane >> 4);
            const float4 a4 = *(const float4*)(sX + (16 * wave + (lane & 15)) * LD + kof);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 b4 = *(const float4*)(sY + (16 * j + (lane & 15)) * LD + kof);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    float* o = part + (size_t)blockIdx.z * a.B * a.N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t b = b0 + 16 * wave + 4 * (lane >> 4) + r;
            if (b < a.B && n < a.N) o[(size_t)b * a.N + n] = acc[j][r];
        }
    }
}

__global__ __launch_bounds__(256) void fwd_merge_kernel(const float* __restrict__ part, int n_split, int64_t B, int N,
                                                        const float* __restrict__ bias, float* __restrict__ Z) {
    const int64_t total = B * N / 4;  // float4s, grid-stride
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        float4 s = *(const float4*)(part + 4 * (size_t)q);
        for (int k = 1; k < n_split; ++k) {
            const float4 v = *(const float4*)(part + (size_t)k * B * N + 4 * (size_t)q);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        if (bias) {
            const float4 v = *(const float4*)(bias + (int)((4 * q) % N));
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *(float4*)(Z + 4 * (size_t)q) = s;
    }
}

// Per column n of dY / Z [B][N] (bn_cols_kernel's geometry): dgamma2, dbeta2 (always into dg / db), then dZ and dbias.
__global__ __launch_bounds__(256) void bn2_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ Z, int64_t B,
                                                      int N, bool batch, const float* __restrict__ gamma2,
                                                      const float* __restrict__ mean2, const float* __restrict__ rstd2,
                                                      float* __restrict__ dg, float* __restrict__ db,
                                                      float* __restrict__ dZ, float* __restrict__ dbias) {
    __shared__ float red[16 * 17];
    const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int n = blockIdx.x * 16 + cl;
    const bool live = n < N;
    const int nc = live ? n : N - 1;
    const float mean = mean2[nc], rstd = rstd2[nc], gr = gamma2[nc] * rstd;
    float s0 = 0.f, s1 = 0.f;
    if (live)
        for (int64_t b = g; b < B; b += 16) {
            const float d = dY[(size_t)b * N + n];
            s0 += d;
            s1 = fmaf(d, xhat(Z[(size_t)b * N + n], mean, rstd), s1);
        }
    const float dbeta = col_sum16(s0, red);
    const float dgamma = col_sum16(s1, red);
    if (live && g == 0) {
        db[n] = dbeta;
        dg[n] = dgamma;
    }
    const float inv_n = __fdiv_rn(1.f, (float)B);
    const float mb = dbeta * inv_n, mg = dgamma * inv_n;
    float sz = 0.f;
    if (live)
        for (int64_t b = g; b < B; b += 16) {
            const float d = dY[(size_t)b * N + n];
            const float v = batch ? gr * ((d - mb) - xhat(Z[(size_t)b * N + n], mean, rstd) * mg) : d * gr;
            dZ[(size_t)b * N + n] = v;
            sz += v;
        }
    const float sb = col_sum16(sz, red);
    if (dbias && live && g == 0) dbias[n] = sb;
}

// out[r][c] = sum_i L(r, i) R(i, c), block (x, y) = (64-row tile, 64-column tile of K).
// T = true  (dW): r = output n, i = sample b; L = dZ[b][n], R = A[b][k]; out = dW [N][K].
// T = false (dA): r = sample b, i = output n; L = dZ[b][n], R = W[n][k]; dH = out m / (1 - p) -> dX (when non-null) and
//                 colpart[(2 x + w) K + k] = the tile's column sums of dH (w = 0) and dH x^ (w = 1) (when non-null).
template <bool T>
__global__ __launch_bounds__(256) void bwd_gemm_kernel(const HeadArgs a, const float* __restrict__ dZ, float* __restrict__ out,
                                                       float* __restrict__ colpart) {
    __shared__ float sL[MT * SLD];
    __shared__ __attribute__((aligned(16))) float sR[MT * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t rows = T ? a.N : a.B, inner = T ? a.B : a.N;
    const int64_t r0 = (int64_t)blockIdx.x * MT;
    const int c0 = blockIdx.y * MT;
    f32x4_t acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int64_t i0 = 0; i0 < inner; i0 += KC) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = tid + 256 * t;
            const int row = q >> 4, c4 = (q & 15) * 4;
            float4 l = make_float4(0.f, 0.f, 0.f, 0.f), r = l;
            if (T) {  // row = sample within the chunk, c4 = output within the tile
                if (i0 + row < a.B && r0 + c4 < a.N) l = *(const float4*)(dZ + (size_t)(i0 + row) * a.N + r0 + c4);
                sL[(c4 + 0) * SLD + row] = l.x;
                sL[(c4 + 1) * SLD + row] = l.y;
                sL[(c4 + 2) * SLD + row] = l.z;
                sL[(c4 + 3) * SLD + row] = l.w;
                if (i0 + row < a.B && c0 + c4 < a.K) r = head_a4(a, i0 + row, c0 + c4);
            } else {  // row = sample within the tile, c4 = output within the chunk
                if (r0 + row < a.B && i0 + c4 < a.N) l = *(const float4*)(dZ + (size_t)(r0 + row) * a.N + i0 + c4);
                sL[row * SLD + c4 + 0] = l.x;
                sL[row * SLD + c4 + 1] = l.y;
                sL[row * SLD + c4 + 2] = l.z;
                sL[row * SLD + c4 + 3] = l.w;
                if (i0 + row < a.N && c0 + c4 < a.K) r = *(const float4*)(a.W + (size_t)(i0 + row) * a.K + c0 + c4);
            }
            *(float4*)(sR + row * LD + c4) = r;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < KC / 4; ++t) {
            const int k = 4 * t + (lane >> 4);
            const float av = sL[(16 * wave + (lane & 15)) * SLD + k];
#pragma unroll
            for (int f = 0; f < 4; ++f)
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sR[k * LD + 16 * f + (lane & 15)], acc[f], 0, 0, 0);
        }
        __syncthreads();
    }
    // acc[f][r] = out[r0 + 16 wave + 4 (lane >> 4) + r][c0 + 16 f + (lane & 15)]
    if (T) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int c = c0 + 16 * f + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t ro = r0 + 16 * wave + 4 * (lane >> 4) + r;
                if (ro < rows && c < a.K) out[(size_t)ro * a.K + c] = acc[f][r];
            }
        }
        return;
    }
    float* sCol = sL;  // [2][4 waves][64 columns]: free after the loop's last barrier
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int c = c0 + 16 * f + (lane & 15);
        const bool cin = c < a.K;
        const int ch = cin && a.gamma1 ? c / a.S : 0;
        const float mean = a.gamma1 ? a.mean1[ch] : 0.f, rstd = a.gamma1 ? a.rstd1[ch] : 0.f;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t b = r0 + 16 * wave + 4 * (lane >> 4) + r;
            if (b < a.B && cin) {
                float v = acc[f][r];
                if (a.dropout) {
                    const uint64_t i = (uint64_t)b * a.K + c;
                    const uint4 w = mask_words(a, i & ~(uint64_t)3);
                    const uint32_t word = (i & 3) == 0 ? w.x : (i & 3) == 1 ? w.y : (i & 3) == 2 ? w.z : w.w;
                    v = word >= a.thresh ? __fmul_rn(v, a.keep_scale) : 0.f;
                }
                if (out) out[(size_t)b * a.K + c] = v;
                if (colpart) {
                    s0 += v;
                    s1 = fmaf(v, xhat(a.X[(size_t)b * a.K + c], mean, rstd), s1);
                }
            }
        }
        if (colpart) {  // the wave's 16 rows: lane groups 0..3 in order
            float t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                t0 += __shfl(s0, 16 * g + (lane & 15));
                t1 += __shfl(s1, 16 * g + (lane & 15));
            }
            if (lane < 16) {
                sCol[(0 * 4 + wave) * 64 + 16 * f + lane] = t0;
                sCol[(1 * 4 + wave) * 64 + 16 * f + lane] = t1;
            }
        }
    }
    if (colpart) {
        __syncthreads();
        if (tid < 128) {
            const int w = tid >> 6, col = tid & 63;
            const float* p = sCol + w * 4 * 64 + col;
            const float s = ((p[0] + p[64]) + p[128]) + p[192];
            if (c0 + col < a.K) colpart[((size_t)blockIdx.x * 2 + w) * a.K + c0 + col] = s;
        }
    }
}

// dbeta1[c] / dgamma1[c]: the column sums of channel c in (row tile, s) order.  One thread per channel.
__global__ __launch_bounds__(256) void bn1_bwd_kernel(const float* __restrict__ colpart, int tiles, int K, int S,
                                                      float* __restrict__ dg, float* __restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K / S) return;
    float s0 = 0.f, s1 = 0.f;
    for (int t = 0; t < tiles; ++t) {
        const float* p = colpart + (size_t)t * 2 * K + (size_t)c * S;
        for (int s = 0; s < S; ++s) {
            s0 += p[s];
            s1 += p[K + s];
        }
    }
    db[c] = s0;
    dg[c] = s1;
}

// dX (holding dH) -> dX, four elements per thread.
__global__ __launch_bounds__(256) void dx_kernel(const HeadArgs a, const float* __restrict__ dg, const float* __restrict__ db,
                                                 float* __restrict__ dX) {
    const float inv_n = __fdiv_rn(1.f, (float)((int64_t)a.B * a.S));
    const int64_t total = (int64_t)a.B * a.K / 4;  // float4s, grid-stride
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int k = (int)((4 * q) % a.K);
        float4 v = *(const float4*)(dX + 4 * (size_t)q);
        const float4 x = *(const float4*)(a.X + 4 * (size_t)q);
        float* e = (float*)&v;
        const float* xe = (const float*)&x;
        int c = k / a.S, rem = k - c * a.S;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (rem == a.S) {
                rem = 0;
                ++c;
            }
            const float gr = a.gamma1[c] * a.rstd1[c];
            e[j] = a.batch_stats ? gr * ((e[j] - db[c] * inv_n) - xhat(xe[j], a.mean1[c], a.rstd1[c]) * (dg[c] * inv_n))
                                 : e[j] * gr;
            ++rem;
        }
        *(float4*)(dX + 4 * (size_t)q) = v;
    }
}

// K splits of the forward product, whole 64-float chunks each, a function of (B, K, N) alone: about two workgroups
// per CU over the (row tile, output tile, split) grid and at most 64 splits.
void head_train_plan(int B, int K, int N, int* n_split, int* k_per_split) {
    const int64_t tiles = (int64_t)((B + MT - 1) / MT) * ((N + MT - 1) / MT);
    const int chunks = (K + KC - 1) / KC;
    const int want = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(chunks, 64), 512 / tiles));
    const int cps = (chunks + want - 1) / want;
    *k_per_split = cps * KC;
    *n_split = (chunks + cps - 1) / cps;
}

size_t row_tiles(int B) { return (size_t)(B + MT - 1) / MT; }

unsigned stride_grid(int64_t quads) { return (unsigned)std::min<int64_t>((quads + 255) / 256, 1 << 20); }

}  // namespace

// forward: [split][B][N]; backward: dZ [B][N], colpart [row tiles][2][K], dgamma1 / dbeta1 [<= K] each,
// dgamma2 / dbeta2 [N] each
size_t head_workspace(int B, int K, int N) {
    int ns, kps;
    head_train_plan(B, K, N, &ns, &kps);
    const size_t fwd = (size_t)ns * B * N;
    const size_t bwd = (size_t)B * N + 2 * row_tiles(B) * K + 2 * (size_t)K + 2 * (size_t)N;
    return std::max(fwd, bwd) * sizeof(float);
}

hipError_t launch_head_train_forward(HeadArgs a, const float* bias, float* rm1, float* rv1, const float* gamma2,
                                     const float* beta2, float* rm2, float* rv2, float eps, float momentum, float* Y,
                                     float* Z, float* mean1, float* rstd1, float* mean2, float* rstd2, float* A, void* ws,
                                     hipStream_t s) {
    if (a.gamma1) {
        const BnOut o{rm1, rv1, mean1, rstd1, eps, momentum, a.batch_stats};
        const int Cin = a.K / a.S;
        if (a.S == 1 || !a.batch_stats)  // running statistics: one thread per channel copies them, X is not read
            hipLaunchKernelGGL(bn_cols_kernel<false>, dim3((Cin + 15) / 16), dim3(256), 0, s, a.X, (int64_t)a.B, Cin, o,
                               nullptr, nullptr, nullptr);
        else
            hipLaunchKernelGGL(bn_chan_kernel, dim3(Cin), dim3(256), 0, s, a.X, (int64_t)a.B, a.K, a.S, o);
        a.mean1 = mean1;
        a.rstd1 = rstd1;
    }
    int ns, kps;
    head_train_plan(a.B, a.K, a.N, &ns, &kps);
    float* part = (float*)ws;
    hipLaunchKernelGGL(fwd_gemm_kernel, dim3((a.B + MT - 1) / MT, (a.N + MT - 1) / MT, ns), dim3(256), 0, s, a, kps, part, A);
    const int64_t quads = (int64_t)a.B * a.N / 4;
    hipLaunchKernelGGL(fwd_merge_kernel, dim3(stride_grid(quads)), dim3(256), 0, s, part, ns, (int64_t)a.B, a.N,
                       bias, Z);
    const BnOut o2{rm2, rv2, mean2, rstd2, eps, momentum, a.batch_stats};
    hipLaunchKernelGGL(bn_cols_kernel<true>, dim3((a.N + 15) / 16), dim3(256), 0, s, Z, (int64_t)a.B, a.N, o2, gamma2, beta2, Y);
    return hipGetLastError();
}

hipError_t launch_head_train_backward(HeadArgs a, const float* gamma2, const float* mean2, const float* rstd2,
                                      const float* Z, const float* dY, float* dX, float* dW, float* dbias, float* dgamma1,
                                      float* dbeta1, float* dgamma2, float* dbeta2, void* ws, hipStream_t s) {
    const size_t tiles = row_tiles(a.B);
    float* dZ = (float*)ws;
    float* colpart = dZ + (size_t)a.B * a.N;
    float* t_dg1 = colpart + 2 * tiles * a.K;
    float* t_db1 = t_dg1 + a.K;
    float* t_dg2 = t_db1 + a.K;
    float* t_db2 = t_dg2 + a.N;
    hipLaunchKernelGGL(bn2_bwd_kernel, dim3((a.N + 15) / 16), dim3(256), 0, s, dY, Z, (int64_t)a.B, a.N, a.batch_stats, gamma2,
                       mean2, rstd2, dgamma2 ? dgamma2 : t_dg2, dbeta2 ? dbeta2 : t_db2, dZ, dbias);
    if (dW)
        hipLaunchKernelGGL(bwd_gemm_kernel<true>, dim3((a.N + MT - 1) / MT, (a.K + MT - 1) / MT), dim3(256), 0, s, a, dZ, dW,
                           nullptr);
    const bool sums = a.gamma1 && (dgamma1 || dbeta1 || (dX && a.batch_stats));
    if (dX || sums) {
        hipLaunchKernelGGL(bwd_gemm_kernel<false>, dim3((unsigned)tiles, (a.K + MT - 1) / MT), dim3(256), 0, s, a, dZ, dX,
                           sums ? colpart : nullptr);
        float* dg = dgamma1 ? dgamma1 : t_dg1;
        float* db = dbeta1 ? dbeta1 : t_db1;
        if (sums)
            hipLaunchKernelGGL(bn1_bwd_kernel, dim3((a.K / a.S + 255) / 256), dim3(256), 0, s, colpart, (int)tiles, a.K, a.S, dg,
                               db);
        if (dX && a.gamma1) {
            const int64_t quads = (int64_t)a.B * a.K / 4;
            hipLaunchKernelGGL(dx_kernel, dim3(stride_grid(quads)), dim3(256), 0, s, a, dg, db, dX);
        }
    }
    return hipGetLastError();
}

}  // namespace fr
