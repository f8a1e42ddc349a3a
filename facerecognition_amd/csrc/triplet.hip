// Online triplet mining and the triplet margin loss (the reference's mine_semi_hard_triplets, mine_batch_hard_triplets,
// mine_triplets and TripletLoss), forward and backward (DESIGN.md §4 "Triplet mining and loss").
//
// Replaces: models/facenet/facenet_dataloader.py:169-284 and models/facenet/facenet_model.py:53-115 (torch.cdist plus a
// Python loop with a host synchronisation per (anchor, positive) pair) and train_facenet.py:41-54.
//
// Mining distances are the Gram form on exact f32 scores: score_tile.h's v_mfma_f32_16x16x4f32 tile loop (64 rows x 64
// rows, D staged through LDS in 64-float chunks, k = 16 t16 + 4 (lane >> 4) + c).
//   count_kernel    per anchor the number of triplets (labels only) -> lims[a + 1];  scan_kernel: the prefix sums
//   sqnorm_kernel   s[r] = sum_k e_rk^2 in a fixed order
//   dist_kernel     one band of anchors x all rows: d = sqrt(max(s_i + s_j - 2 g_ij, 0)) -> band [R][N] in the workspace
//   select_pairs    one workgroup per anchor, its waves take the anchor's positives in turn (slot lims[a] + k): a
//                   wave-wide (value, index) reduction over the anchor's distance row, ties to the lowest index
//   select_hard     one wave per anchor (batch-hard)
//   loss_terms      one wave per triplet: the difference-form distances and the hinge -> terms [T][4]
//   loss_stats      one workgroup: terms in a fixed order -> {loss, accuracy, pos_dist, neg_dist}
//   coef_kernel     one wave per triplet: (u / T) / delta_ap and (u / T) / delta_an, zero where inactive
//   gather_kernel   one workgroup per dE row (and 1024-float D chunk): scans the index arrays and adds the row's terms in
//                   ascending triplet order
// No float atomics; every sum runs in an order fixed by the shapes; a band's height changes no bit.
#include "score_tile.h"
#include "frhip.h"
#include <float.h>
#include <limits.h>

#include <algorithm>

namespace fr {
using namespace tile;
namespace {

constexpr float PAIR_EPS = 1e-6f;  // F.pairwise_distance's eps

__global__ __launch_bounds__(256) void count_kernel(const int32_t* __restrict__ labels, int N, int mode,
                                                    int64_t* __restrict__ lims) {
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= N) return;
    const int la = labels[a];
    int same = 0;
    for (int j = lane; j < N; j += 64) same += labels[j] == la;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) same += __shfl_xor(same, o);
    if (lane == 0) {
        const bool any = same > 1 && same < N;  // a positive and a negative exist
        lims[a + 1] = !any ? 0 : (mode == FR_TRIPLET_BATCH_HARD ? 1 : same - 1);
        if (a == 0) lims[0] = 0;
    }
}

// lims[1 .. N] in place: counts -> inclusive prefix sums.  One workgroup; a thread owns `per` consecutive entries.
__global__ __launch_bounds__(1024) void scan_kernel(int64_t* lims, int N) {
    __shared__ int64_t s[1024];
    const int tid = threadIdx.x;
    const int per = (N + 1023) / 1024;
    const int lo = std::min(N, tid * per), hi = std::min(N, lo + per);
    int64_t sum = 0;
    for (int i = lo; i < hi; ++i) sum += lims[1 + i];
    s[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    int64_t run = s[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        run += lims[1 + i];
        lims[1 + i] = run;
    }
}

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ X, int R, int D, float* __restrict__ sq) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float ss = row_sqsum(X + (size_t)r * D, D);
    if (lane == 0) sq[r] = ss;
}

// band[i - b0][j] = d_ij for anchors i in [b0, b1) and every row j; block (x, y) = (64-row tile of j, 64-anchor tile).
__global__ __launch_bounds__(256) void dist_kernel(const float* __restrict__ E, int N, int D, const float* __restrict__ sq,
                                                   int b0, int b1, float* __restrict__ band) {
    __shared__ __attribute__((aligned(16))) float sXY[2 * MT * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = b0 + blockIdx.y * MT, t0 = blockIdx.x * MT;
    f32x4_t acc[4];
    score_tile_prefetch<int64_t, int64_t>(E, b1, x0, E, N, t0, D, sXY, sXY + MT * LD, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = x0 + 16 * wave + 4 * (lane >> 4) + r;
        if (i >= b1) continue;
        const float si = sq[i];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            const int j = t0 + 16 * j4 + (lane & 15);
            if (j >= N) continue;
            const float d2 = fmaxf((si + sq[j]) - 2.f * acc[j4][r], 0.f);
            band[(size_t)(i - b0) * N + j] = __fsqrt_rn(d2);
        }
    }
}

// The smaller (d, j) pair, lexicographic, over the wave; every lane ends with the result.  d is never NaN.
__device__ __forceinline__ void wave_min_pair(float& d, int& j) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float od = __shfl_xor(d, o);
        const int oj = __shfl_xor(j, o);
        if (od < d || (od == d && oj < j)) {
            d = od;
            j = oj;
        }
    }
}

__device__ __forceinline__ void wave_max_pair(float& d, int& j) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float od = __shfl_xor(d, o);
        const int oj = __shfl_xor(j, o);
        if (od > d || (od == d && oj < j)) {
            d = od;
            j = oj;
        }
    }
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

struct MineOut {
    int32_t *a_idx, *p_idx, *n_idx;
    uint8_t* semi;
    int64_t capacity;
};

// FR_TRIPLET_SEMI_HARD / FR_TRIPLET_FIRST: workgroup = anchor b0 + blockIdx.x, positive k of the anchor goes to wave
// k % 4.  A lane walks its columns in ascending order, so a strict comparison keeps the lowest index of equal values;
// an index left at INT_MAX says that nothing compared (non-finite distances): the lowest negative stands in.
template <int MODE>
__global__ __launch_bounds__(256) void select_pairs_kernel(const float* __restrict__ band, int b0, int N,
                                                           const int32_t* __restrict__ labels,
                                                           const int64_t* __restrict__ lims, float margin, MineOut out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = b0 + blockIdx.x;
    const int64_t base = lims[a], cnt = lims[a + 1] - base;
    if (cnt <= 0) return;
    const int la = labels[a];
    const float* __restrict__ row = band + (size_t)blockIdx.x * N;
    int64_t k = 0;
    for (int j0 = 0; j0 < N && k < cnt; j0 += 64) {
        const int jp = j0 + lane;
        unsigned long long m = __ballot(jp < N && jp != a && labels[jp] == la);
        for (; m && k < cnt; m &= m - 1, ++k) {
            if ((int)(k & 3) != wave) continue;
            const int p = j0 + __ffsll((long long)m) - 1;
            const float d_ap = row[p];
            const float thr = d_ap + margin;
            float sd = INFINITY, fd = MODE == FR_TRIPLET_FIRST ? -INFINITY : INFINITY;
            int sj = INT_MAX, fj = INT_MAX, first_neg = INT_MAX;
            for (int j = lane; j < N; j += 64) {
                if (labels[j] == la) continue;
                const float d = row[j];
                first_neg = min(first_neg, j);
                const bool sh = d > d_ap && d < thr;
                if (MODE == FR_TRIPLET_FIRST) {
                    if (sh) sj = min(sj, j);
                    if (d > fd) { fd = d; fj = j; }
                } else {
                    if (sh && d < sd) { sd = d; sj = j; }
                    if (d < fd) { fd = d; fj = j; }
                }
            }
            if (MODE == FR_TRIPLET_FIRST) {
                sj = wave_min_int(sj);
                wave_max_pair(fd, fj);
            } else {
                wave_min_pair(sd, sj);
                wave_min_pair(fd, fj);
            }
            first_neg = wave_min_int(first_neg);
            const bool took = sj != INT_MAX;
            const int n = took ? sj : (fj != INT_MAX ? fj : first_neg);
            const int64_t slot = base + k;
            if (lane == 0 && slot < out.capacity) {
                out.a_idx[slot] = a;
                out.p_idx[slot] = p;
                out.n_idx[slot] = n;
                if (out.semi) out.semi[slot] = took;
            }
        }
    }
}

// FR_TRIPLET_BATCH_HARD: one wave per anchor, the farthest positive and the nearest negative.
__global__ __launch_bounds__(256) void select_hard_kernel(const float* __restrict__ band, int b0, int b1, int N,
                                                          const int32_t* __restrict__ labels,
                                                          const int64_t* __restrict__ lims, MineOut out) {
    const int lane = threadIdx.x & 63;
    const int a = b0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= b1) return;
    const int64_t slot = lims[a];
    if (lims[a + 1] - slot <= 0) return;
    const int la = labels[a];
    const float* __restrict__ row = band + (size_t)(a - b0) * N;
    float pd = -INFINITY, nd = INFINITY;
    int pj = INT_MAX, nj = INT_MAX, first_pos = INT_MAX, first_neg = INT_MAX;
    for (int j = lane; j < N; j += 64) {
        if (j == a) continue;
        const float d = row[j];
        if (labels[j] == la) {
            first_pos = min(first_pos, j);
            if (d > pd) { pd = d; pj = j; }
        } else {
            first_neg = min(first_neg, j);
            if (d < nd) { nd = d; nj = j; }
        }
    }
    wave_max_pair(pd, pj);
    wave_min_pair(nd, nj);
    first_pos = wave_min_int(first_pos);
    first_neg = wave_min_int(first_neg);
    if (lane == 0 && slot < out.capacity) {
        out.a_idx[slot] = a;
        out.p_idx[slot] = pj != INT_MAX ? pj : first_pos;
        out.n_idx[slot] = nj != INT_MAX ? nj : first_neg;
        if (out.semi) out.semi[slot] = 0;
    }
}

// The wave's triplet t: sum (a - p + eps)^2, sum (a - n + eps)^2, sum (a - p)^2, sum (a - n)^2 over D, every lane.
__device__ __forceinline__ void pair_sums(const float* __restrict__ E, int D, int ia, int ip, int in, float* sp, float* sn,
                                          float* qp, float* qn) {
    const int lane = threadIdx.x & 63;
    const float* ea = E + (size_t)ia * D;
    const float* ep = E + (size_t)ip * D;
    const float* en = E + (size_t)in * D;
    float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
    for (int d = 4 * lane; d < D; d += 256) {
        const float4 va = *(const float4*)(ea + d), vp = *(const float4*)(ep + d), vn = *(const float4*)(en + d);
        const float xa[4] = {va.x, va.y, va.z, va.w}, xp[4] = {vp.x, vp.y, vp.z, vp.w}, xn[4] = {vn.x, vn.y, vn.z, vn.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float dp = xa[c] - xp[c], dn = xa[c] - xn[c];
            const float ep1 = dp + PAIR_EPS, en1 = dn + PAIR_EPS;
            q0 += dp * dp;
            q1 += dn * dn;
            s0 += ep1 * ep1;
            s1 += en1 * en1;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        q0 += __shfl_xor(q0, o);
        q1 += __shfl_xor(q1, o);
    }
    *sp = s0; *sn = s1; *qp = q0; *qn = q1;
}

__global__ __launch_bounds__(256) void loss_terms_kernel(const float* __restrict__ E, int D, const int32_t* __restrict__ a,
                                                         const int32_t* __restrict__ p, const int32_t* __restrict__ n,
                                                         int64_t T, float margin, float4* __restrict__ terms) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += (int64_t)gridDim.x * 4) {
        float sp, sn, qp, qn;
        pair_sums(E, D, a[t], p[t], n[t], &sp, &sn, &qp, &qn);
        const float x = (margin + __fsqrt_rn(sp)) - __fsqrt_rn(sn);
        if (lane == 0) terms[t] = make_float4(fmaxf(x, 0.f), __fsqrt_rn(qp), __fsqrt_rn(qn), x);
    }
}

// stats = {mean hinge, share of ||a - p|| < ||a - n||, mean ||a - p||, mean ||a - n||}: thread i sums the triplets
// i, i + 1024, ... in order, then a halving tree over the 1024 threads.
__global__ __launch_bounds__(1024) void loss_stats_kernel(const float4* __restrict__ terms, int64_t T,
                                                          float* __restrict__ stats) {
    __shared__ float s[4][1024];
    const int tid = threadIdx.x;
    float h = 0.f, c = 0.f, dp = 0.f, dn = 0.f;
    for (int64_t t = tid; t < T; t += 1024) {
        const float4 v = terms[t];
        h += v.x;
        c += v.y < v.z ? 1.f : 0.f;
        dp += v.y;
        dn += v.z;
    }
    s[0][tid] = h; s[1][tid] = c; s[2][tid] = dp; s[3][tid] = dn;
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q][tid] += s[q][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float inv = 1.f / (float)T;
        *(float4*)stats = make_float4(s[0][0] * inv, s[1][0] * inv, s[2][0] * inv, s[3][0] * inv);
    }
}

// coef[t] = {(u / T) / delta_ap, (u / T) / delta_an}, zero for an inactive triplet and where delta is zero.
__global__ __launch_bounds__(256) void coef_kernel(const float* __restrict__ E, int D, const int32_t* __restrict__ a,
                                                   const int32_t* __restrict__ p, const int32_t* __restrict__ n,
                                                   int64_t T, float margin, float u, float2* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const float ut = u / (float)T;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += (int64_t)gridDim.x * 4) {
        float sp, sn, qp, qn;
        pair_sums(E, D, a[t], p[t], n[t], &sp, &sn, &qp, &qn);
        const float dap = __fsqrt_rn(sp), dan = __fsqrt_rn(sn);
        const bool active = (margin + dap) - dan >= 0.f;
        if (lane == 0)
            coef[t] = make_float2(active && dap > 0.f ? __fdiv_rn(ut, dap) : 0.f,
                                  active && dan > 0.f ? __fdiv_rn(ut, dan) : 0.f);
    }
}

// acc += c ((x - y) + eps) on four floats
__device__ __forceinline__ void add_diff(float4& acc, float c, const float* __restrict__ x, const float* __restrict__ y) {
    const float4 vx = *(const float4*)x, vy = *(const float4*)y;
    acc.x += c * ((vx.x - vy.x) + PAIR_EPS);
    acc.y += c * ((vx.y - vy.y) + PAIR_EPS);
    acc.z += c * ((vx.z - vy.z) + PAIR_EPS);
    acc.w += c * ((vx.w - vy.w) + PAIR_EPS);
}

// dE[r][4 tid + 1024 blockIdx.y ..]: workgroup (r, D chunk) scans a, p, n in chunks of 256 triplets and adds the terms of
// the triplets that name r, in ascending triplet order and, within a triplet, as anchor, positive, negative.
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ E, int D, const int32_t* __restrict__ a,
                                                     const int32_t* __restrict__ p, const int32_t* __restrict__ n,
                                                     int64_t T, const float2* __restrict__ coef, float* __restrict__ dE) {
    __shared__ unsigned long long sm[4];
    __shared__ int sf[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const int d = blockIdx.y * 1024 + 4 * tid;
    const bool has = d < D;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t base = 0; base < T; base += 256) {
        const int64_t t = base + tid;
        int f = 0;
        if (t < T) f = (a[t] == r ? 1 : 0) | (p[t] == r ? 2 : 0) | (n[t] == r ? 4 : 0);
        if (!__syncthreads_or(f)) continue;
        const unsigned long long m = __ballot(f != 0);
        if (lane == 0) sm[wave] = m;
        sf[tid] = f;
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            for (unsigned long long mm = sm[w]; mm; mm &= mm - 1) {
                const int i = 64 * w + __ffsll((long long)mm) - 1;
                const int fi = sf[i];
                const int64_t tt = base + i;
                const float2 c = coef[tt];
                if (!has) continue;
                const float* ea = E + (size_t)a[tt] * D + d;
                if (fi & 1) {
                    if (c.x != 0.f) add_diff(acc, c.x, ea, E + (size_t)p[tt] * D + d);
                    if (c.y != 0.f) add_diff(acc, -c.y, ea, E + (size_t)n[tt] * D + d);
                }
                if ((fi & 2) && c.x != 0.f) add_diff(acc, -c.x, ea, E + (size_t)p[tt] * D + d);
                if ((fi & 4) && c.y != 0.f) add_diff(acc, c.y, ea, E + (size_t)n[tt] * D + d);
            }
        }
        __syncthreads();
    }
    if (has) *(float4*)(dE + (size_t)r * D + d) = acc;
}

int sq_floats(int N) { return (N + 63) / 64 * 64; }

}  // namespace

size_t triplet_min_workspace(int N) { return ((size_t)MT * N + sq_floats(N)) * sizeof(float); }

// The whole distance matrix where it is at most 256 MiB, else as many 64-anchor bands as fit in that.
size_t triplet_workspace(int N) {
    const size_t all = (size_t)(N + MT - 1) / MT;
    const size_t fit = std::max<size_t>(1, ((size_t)256 << 20) / ((size_t)MT * N * sizeof(float)));
    return (std::min(all, fit) * MT * N + sq_floats(N)) * sizeof(float);
}

hipError_t launch_triplet_count(const int32_t* labels, int N, int mode, int64_t* lims, hipStream_t s) {
    hipLaunchKernelGGL(count_kernel, dim3((N + 3) / 4), dim3(256), 0, s, labels, N, mode, lims);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, lims, N);
    return hipGetLastError();
}

hipError_t launch_triplet_mine(const float* E, int N, int D, const int32_t* labels, int mode, float margin,
                               const int64_t* lims, int32_t* a_idx, int32_t* p_idx, int32_t* n_idx, int64_t capacity,
                               uint8_t* semi, void* ws, size_t ws_bytes, hipStream_t s) {
    float* sq = (float*)ws;
    float* band = sq + sq_floats(N);
    const size_t rows_fit = (ws_bytes / sizeof(float) - sq_floats(N)) / N / MT * MT;  // >= 64: checked by the caller
    const int R = (int)std::min<size_t>(rows_fit, (size_t)(N + MT - 1) / MT * MT);
    const MineOut out = {a_idx, p_idx, n_idx, semi, capacity};
    hipLaunchKernelGGL(sqnorm_kernel, dim3((N + 3) / 4), dim3(256), 0, s, E, N, D, sq);
    for (int b0 = 0; b0 < N; b0 += R) {
        const int b1 = std::min(N, b0 + R);
        hipLaunchKernelGGL(dist_kernel, dim3((N + MT - 1) / MT, (b1 - b0 + MT - 1) / MT), dim3(256), 0, s, E, N, D, sq, b0,
                           b1, band);
        if (mode == FR_TRIPLET_BATCH_HARD)
            hipLaunchKernelGGL(select_hard_kernel, dim3((b1 - b0 + 3) / 4), dim3(256), 0, s, band, b0, b1, N, labels, lims,
                               out);
        else if (mode == FR_TRIPLET_FIRST)
            hipLaunchKernelGGL(select_pairs_kernel<FR_TRIPLET_FIRST>, dim3(b1 - b0), dim3(256), 0, s, band, b0, N, labels,
                               lims, margin, out);
        else
            hipLaunchKernelGGL(select_pairs_kernel<FR_TRIPLET_SEMI_HARD>, dim3(b1 - b0), dim3(256), 0, s, band, b0, N,
                               labels, lims, margin, out);
    }
    return hipGetLastError();
}

static int triplet_wave_blocks(int64_t T) { return (int)std::min<int64_t>((T + 3) / 4, 1 << 20); }

hipError_t launch_triplet_loss_forward(const float* E, int D, const int32_t* a, const int32_t* p, const int32_t* n,
                                       int64_t T, float margin, float* terms, float* stats, hipStream_t s) {
    hipLaunchKernelGGL(loss_terms_kernel, dim3(triplet_wave_blocks(T)), dim3(256), 0, s, E, D, a, p, n, T, margin,
                       (float4*)terms);
    hipLaunchKernelGGL(loss_stats_kernel, dim3(1), dim3(1024), 0, s, (const float4*)terms, T, stats);
    return hipGetLastError();
}

hipError_t launch_triplet_loss_backward(const float* E, int N, int D, const int32_t* a, const int32_t* p,
                                        const int32_t* n, int64_t T, float margin, float u, float* dE, void* ws,
                                        hipStream_t s) {
    hipLaunchKernelGGL(coef_kernel, dim3(triplet_wave_blocks(T)), dim3(256), 0, s, E, D, a, p, n, T, margin, u, (float2*)ws);
    hipLaunchKernelGGL(gather_kernel, dim3(N, (D + 1023) / 1024), dim3(256), 0, s, E, D, a, p, n, T, (const float2*)ws, dE);
    return hipGetLastError();
}

}  // namespace fr
