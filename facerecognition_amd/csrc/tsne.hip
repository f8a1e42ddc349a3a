// t-SNE on the device (DESIGN.md §4 "t-SNE"): sklearn.manifold.TSNE's default algorithm with the repulsive term summed
// exactly over all pairs (Barnes-Hut with angle 0), two components.
//
// Replaces: inference/extract_embeddings.py visualize_tsne's sklearn call (a host Barnes-Hut run on at most 2000 rows).
//
// Once per fit:
//   tsne_sqdist_kernel   one wave per row: sum_d (x_i - x_j)^2 of its k neighbours by direct subtraction;
//   tsne_search_kernel   one wave per row: sklearn's bisection for the bandwidth beta_i (float64, the row's smallest
//                        distance subtracted first), then p_j|i from the float32-rounded beta;
//   symmetrisation       P_cond (k unsorted columns per row) is transposed twice: the first transpose gives each row's
//                        reverse neighbours in ascending order, the second gives its own neighbours in ascending order;
//                        a two-pointer merge per row then writes (p_j|i + p_i|j) / (2 N) as CSR.  A transpose is
//                        count / prefix / fill in the manner of match_range.hip: the source rows are cut into splits,
//                        one wave walks a split's rows in ascending order and keeps one counter per (split, target
//                        row), a plain load / add / store (a row's targets are distinct, so no two lanes share a
//                        counter; a barrier orders one row after the other).  An entry's place is
//                        start[target] + earlier splits' counts + its counter, so ascending source order falls out with
//                        no atomics and no sort.
// Per iteration (three launches, no host synchronisation):
//   tsne_rep_kernel      the hot one: i points in registers (4 per thread), the split's j points as wave-uniform
//                        global loads, per pair dx, dy, w = 1 / (1 + dx^2 + dy^2), z += w, f += w^2 (dx, dy).  The
//                        self pair's force needs no branch (dx = dy = 0); its w = 1 is masked out of z by index, in
//                        the few tiles that hold the block's own points only (summing it and taking Z = sum - N
//                        costs Z its low bits once the layout has spread: 44 x the gradient bound at N = 2,
//                        |Y| = 30).  A tail tile is cut by its length, not by a sentinel.  j is split over
//                        blockIdx.y; partials {fx, fy, z} per (split, i);
//   tsne_attr_kernel     one wave per row of P: sum_j P_ij w_ij (y_i - y_j), the row's KL terms (float64, on request),
//                        the sum over splits of the row's repulsion partials; per-block float64 sums of z and KL;
//   tsne_update_kernel   Z from the per-block sums (every block adds them in the same order), the gradient, sklearn's
//                        gains / momentum step, per-block float64 sum of g^2.
// tsne_stats_kernel closes a call: {KL, Z, |grad|} from the per-block sums.  All sums run in a fixed order (strided
// per-thread sums, xor-butterfly wave sums, fixed LDS trees), so a run is bitwise repeatable.
#include "kernels.h"
#include <limits.h>

#include <algorithm>

namespace fr {
namespace {

constexpr int REP_T = 128;         // threads of a repulsion block
constexpr int REP_IPT = 4;         // i points per thread
constexpr int REP_IB = REP_T * REP_IPT;
constexpr int REP_JT = 256;        // j points per tile (the unit of the self-pair masking)
constexpr int REP_MAX_SPLIT = 64;  // <= 64: tsne_attr_kernel sums a row's partials with one lane per split
constexpr int ATTR_ROWS = 64;      // rows of P per tsne_attr_kernel block (4 waves x 16)
constexpr int UPD_T = 256;
constexpr int SCAN_T = 1024;

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

// Sum of a [n] (double) by one block of T threads, the same value in every thread and in every block: thread t adds
// a[t], a[t + T], ... and the T sums are added pairwise through LDS.
template <int T>
__device__ __forceinline__ double block_sum_strided(const double* __restrict__ a, int n, double* sh) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += T) v += a[i];
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = T / 2; o; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---- squared distances ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_sqdist_kernel(const float* __restrict__ X, int N, int D,
                                                          const int32_t* __restrict__ idx, int k,
                                                          float* __restrict__ d2) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const float* xi = X + (size_t)i * D;
    for (int j = 0; j < k; ++j) {
        const int c = clampi(idx[(size_t)i * k + j], N);
        const float* xj = X + (size_t)c * D;
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float t = xi[d] - xj[d];
            acc = fmaf(t, t, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) d2[(size_t)i * k + j] = acc;
    }
}

// ---- bandwidth search -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_search_kernel(const float* __restrict__ d2, int N, int k, double target,
                                                          float* __restrict__ beta_out, float* __restrict__ pc) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const float* d = d2 + (size_t)i * k;
    float m = INFINITY;
    for (int j = lane; j < k; j += 64) m = fminf(m, d[j]);
    const double dmin = (double)wave_min(m);
    double beta = 1.0, lo = -INFINITY, hi = INFINITY;
    for (int step = 0; step < 100; ++step) {
        double sp = 0.0, sdp = 0.0;
        for (int j = lane; j < k; j += 64) {
            const double dd = (double)d[j] - dmin;
            const double p = exp(-dd * beta);
            sp += p;
            sdp += dd * p;
        }
        sp = wave_sum(sp);
        sdp = wave_sum(sdp);
        if (sp == 0.0) sp = 1e-8;
        const double diff = log(sp) + beta * (sdp / sp) - target;  // the same value in every lane
        if (fabs(diff) <= 1e-5) break;
        if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) * 0.5;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5 : (beta + lo) * 0.5;
        }
    }
    const float bf = (float)beta;
    const double b = (double)bf;
    double sp = 0.0;
    for (int j = lane; j < k; j += 64) sp += exp(-((double)d[j] - dmin) * b);
    sp = wave_sum(sp);
    if (sp == 0.0) sp = 1e-8;
    for (int j = lane; j < k; j += 64) pc[(size_t)i * k + j] = (float)(exp(-((double)d[j] - dmin) * b) / sp);
    if (lane == 0) beta_out[i] = bf;
}

// ---- transpose: count / offsets / fill ----------------------------------------------------------------------------
// Source row j holds entries [inptr[j], inptr[j + 1]) (inptr null: [j k, (j + 1) k)) of icol / ival; an entry with
// column t becomes column j of target row t.  One wave (= one block) per split of rows_per_split source rows.
template <bool FILL>
__global__ __launch_bounds__(64) void tsne_transpose_kernel(const int32_t* __restrict__ inptr,
                                                            const int32_t* __restrict__ icol,
                                                            const float* __restrict__ ival, int N, int k,
                                                            int rows_per_split, int32_t* cnt,
                                                            const int32_t* __restrict__ outptr,
                                                            int32_t* __restrict__ ocol, float* __restrict__ oval,
                                                            int64_t capacity) {
    const int lane = threadIdx.x;
    int32_t* c = cnt + (size_t)blockIdx.x * N;
    const int j0 = blockIdx.x * rows_per_split, j1 = min(j0 + rows_per_split, N);
    for (int j = j0; j < j1; ++j) {
        const int64_t e0 = inptr ? inptr[j] : (int64_t)j * k, e1 = inptr ? inptr[j + 1] : (int64_t)(j + 1) * k;
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int t = clampi(icol[e], N);
            const int slot = c[t];
            c[t] = slot + 1;
            if (FILL) {
                const int64_t pos = (outptr ? (int64_t)outptr[t] : (int64_t)t * k) + slot;
                if (pos >= 0 && pos < capacity) {
                    ocol[pos] = j;
                    oval[pos] = ival[e];
                }
            }
        }
        __syncthreads();  // the next row may name the same targets
    }
}

// cnt [n_split][N] in place to each (split, target)'s start inside the target's row; tot [N] = the row lengths.
__global__ __launch_bounds__(256) void tsne_offsets_kernel(int32_t* __restrict__ cnt, int N, int n_split,
                                                           int32_t* __restrict__ tot) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    int run = 0;
    for (int s = 0; s < n_split; ++s) {
        const int v = cnt[(size_t)s * N + t];
        cnt[(size_t)s * N + t] = run;
        run += v;
    }
    if (tot) tot[t] = run;
}

// a [0, n) in place to its exclusive prefix sum, a[n] = the total.  One block.
__global__ __launch_bounds__(SCAN_T) void tsne_scan_kernel(int32_t* __restrict__ a, int n) {
    __shared__ int32_t part[SCAN_T];
    const int chunk = (n + SCAN_T - 1) / SCAN_T;
    const int b = min((int64_t)threadIdx.x * chunk, (int64_t)n), e = min((int64_t)b + chunk, (int64_t)n);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += a[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < SCAN_T; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        a[n] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = b; i < e; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
}

// Row i of P: the union of its own neighbours (fcol / fval [i k, (i + 1) k), ascending) and its reverse neighbours
// (rcol / rval [rptr[i], rptr[i + 1]), ascending).  FILL false: indptr[i] = the union's size; true: col / val.
template <bool FILL>
__global__ __launch_bounds__(256) void tsne_merge_kernel(const int32_t* __restrict__ fcol,
                                                         const float* __restrict__ fval,
                                                         const int32_t* __restrict__ rptr,
                                                         const int32_t* __restrict__ rcol,
                                                         const float* __restrict__ rval, int N, int k,
                                                         int32_t* __restrict__ indptr, int32_t* __restrict__ col,
                                                         float* __restrict__ val, int64_t capacity) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int64_t a = (int64_t)i * k, b = rptr[i];
    const int64_t a1 = a + k, b1 = rptr[i + 1];
    const float den = 2.f * (float)N;
    int64_t o = FILL ? indptr[i] : 0;
    const int64_t o0 = o;
    while (a < a1 || b < b1) {
        const int ca = a < a1 ? fcol[a] : INT_MAX, cb = b < b1 ? rcol[b] : INT_MAX;
        const int c = min(ca, cb);
        float p = 0.f;
        if (ca == c) p += fval[a++];
        if (cb == c) p += rval[b++];
        if (FILL && o >= 0 && o < capacity) {
            col[o] = c;
            val[o] = p / den;
        }
        ++o;
    }
    if (!FILL) indptr[i] = (int32_t)(o - o0);
}

// One tile of j against the thread's i points.  The self pair adds no force (dx = dy = 0) but would add w = 1 to z,
// and a z of 1 + (a small sum) loses that sum's low bits; DIAG masks it by index (two coincident points are a pair).
template <bool DIAG>
__device__ __forceinline__ void rep_tile(const float2* __restrict__ yj, int n, int jt, int ib, const f2* xi,
                                         const f2* yi, f2* fx, f2* fy, f2* z) {
#pragma unroll 4
    for (int t = 0; t < n; ++t) {
        const float2 q = yj[t];
#pragma unroll
        for (int m = 0; m < REP_IPT / 2; ++m) {
            const f2 dx = xi[m] - q.x, dy = yi[m] - q.y;
            const f2 d = dx * dx + (dy * dy + 1.f);
            f2 w = f2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
            const f2 w2 = w * w;
            if (DIAG) {
                if (jt + t == ib + (2 * m) * REP_T) w.x = 0.f;
                if (jt + t == ib + (2 * m + 1) * REP_T) w.y = 0.f;
            }
            z[m] += w;
            fx[m] += w2 * dx;
            fy[m] += w2 * dy;
        }
    }
}

// ---- repulsion ------------------------------------------------------------------------------------------------------
// part [n_split][N] = {sum_j w^2 dx, sum_j w^2 dy, sum_{j != i} w, 0} over j in [s jr, min((s + 1) jr, N)).
// The j points are read straight from global memory at a wave-uniform address (staging the tile in LDS and reading it
// back as broadcast reads measured 3-5 % slower at N = 46715 and was dropped); REP_JT only bounds the tiles that mask
// the self pair.
__global__ __launch_bounds__(REP_T) void tsne_rep_kernel(const float2* __restrict__ Y, int N, int jr,
                                                         float4* __restrict__ part) {
    const int ib = blockIdx.x * REP_IB + threadIdx.x;
    f2 xi[REP_IPT / 2], yi[REP_IPT / 2], fx[REP_IPT / 2], fy[REP_IPT / 2], z[REP_IPT / 2];
#pragma unroll
    for (int m = 0; m < REP_IPT / 2; ++m) {
        const float2 p0 = Y[min(ib + (2 * m) * REP_T, N - 1)], p1 = Y[min(ib + (2 * m + 1) * REP_T, N - 1)];
        xi[m] = f2{p0.x, p1.x};
        yi[m] = f2{p0.y, p1.y};
        fx[m] = fy[m] = z[m] = f2{0.f, 0.f};
    }
    const int j0 = blockIdx.y * jr, j1 = min(j0 + jr, N);
    for (int jt = j0; jt < j1; jt += REP_JT) {
        const int n = min(REP_JT, j1 - jt);
        const float2* src = Y + jt;
        // a tile that holds one of the block's own i points masks the self pair out of z (uniform per block and tile)
        if (jt < (int)(blockIdx.x + 1) * REP_IB && jt + n > (int)blockIdx.x * REP_IB)
            rep_tile<true>(src, n, jt, ib, xi, yi, fx, fy, z);
        else
            rep_tile<false>(src, n, jt, ib, xi, yi, fx, fy, z);
    }
    float4* out = part + (size_t)blockIdx.y * N;
#pragma unroll
    for (int m = 0; m < REP_IPT / 2; ++m) {
        const int i0 = ib + (2 * m) * REP_T, i1 = ib + (2 * m + 1) * REP_T;
        if (i0 < N) out[i0] = make_float4(fx[m].x, fy[m].x, z[m].x, 0.f);
        if (i1 < N) out[i1] = make_float4(fx[m].y, fy[m].y, z[m].y, 0.f);
    }
}

// ---- attraction, KL, per-row sums of the repulsion partials -------------------------------------------------------
// ar [N] = {attr x, attr y, rep x, rep y}; zblk / klblk [gridDim.x] = the block's rows' sum of z / of KL terms.
__global__ __launch_bounds__(256) void tsne_attr_kernel(const int32_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ col,
                                                        const float* __restrict__ val, int N,
                                                        const float2* __restrict__ Y,
                                                        const float4* __restrict__ part, int n_split, int want_kl,
                                                        float4* __restrict__ ar, double* __restrict__ zblk,
                                                        double* __restrict__ klblk) {
    __shared__ double sh[8];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double zacc = 0.0, klacc = 0.0;
    for (int q = 0; q < ATTR_ROWS / 4; ++q) {
        const int i = blockIdx.x * ATTR_ROWS + wv * (ATTR_ROWS / 4) + q;
        if (i >= N) break;
        const float2 yi = Y[i];
        float ax = 0.f, ay = 0.f;
        double kl = 0.0;
        const int e1 = indptr[i + 1];
        for (int e = indptr[i] + lane; e < e1; e += 64) {
            const float p = val[e];
            const float2 yj = Y[clampi(col[e], N)];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const float d = fmaf(dx, dx, fmaf(dy, dy, 1.f));
            const float pw = p * __builtin_amdgcn_rcpf(d);
            ax = fmaf(pw, dx, ax);
            ay = fmaf(pw, dy, ay);
            if (want_kl && p > 0.f) kl += (double)p * log((double)p * (double)d);
        }
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < n_split) r = part[(size_t)lane * N + i];
        ax = wave_sum(ax);
        ay = wave_sum(ay);
        const float rx = wave_sum(r.x), ry = wave_sum(r.y);
        zacc += wave_sum((double)r.z);
        if (want_kl) klacc += wave_sum(kl);
        if (lane == 0) ar[i] = make_float4(ax, ay, rx, ry);
    }
    if (lane == 0) sh[wv] = zacc, sh[4 + wv] = klacc;
    __syncthreads();
    if (threadIdx.x == 0) {
        zblk[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        klblk[blockIdx.x] = (sh[4] + sh[5]) + (sh[6] + sh[7]);
    }
}

// ---- gradient and optimiser step ------------------------------------------------------------------------------------
__global__ __launch_bounds__(UPD_T) void tsne_update_kernel(const float4* __restrict__ ar,
                                                            const double* __restrict__ zblk, int n_zblk, int N,
                                                            float exaggeration, int step, float momentum, float lr,
                                                            float2* __restrict__ Y, float2* __restrict__ update,
                                                            float2* __restrict__ gains, float2* __restrict__ grad,
                                                            double* __restrict__ gsq) {
    __shared__ double sh[UPD_T];
    const double Z = fmax(block_sum_strided<UPD_T>(zblk, n_zblk, sh), 2.220446049250313e-16);
    const float inv_z = (float)(1.0 / Z);
    const int i = blockIdx.x * UPD_T + threadIdx.x;
    double g2 = 0.0;
    if (i < N) {
        const float4 a = ar[i];
        const float gx = 4.f * (exaggeration * a.x - a.z * inv_z), gy = 4.f * (exaggeration * a.y - a.w * inv_z);
        grad[i] = make_float2(gx, gy);
        g2 = (double)gx * gx + (double)gy * gy;
        if (step) {
            float2 u = update[i], gn = gains[i], y = Y[i];
            const bool ix = (u.x < 0.f && gx > 0.f) || (u.x > 0.f && gx < 0.f);  // update * g < 0, no underflow
            const bool iy = (u.y < 0.f && gy > 0.f) || (u.y > 0.f && gy < 0.f);
            gn.x = fmaxf(ix ? gn.x + 0.2f : gn.x * 0.8f, 0.01f);
            gn.y = fmaxf(iy ? gn.y + 0.2f : gn.y * 0.8f, 0.01f);
            u.x = momentum * u.x - lr * (gn.x * gx);
            u.y = momentum * u.y - lr * (gn.y * gy);
            y.x += u.x;
            y.y += u.y;
            gains[i] = gn, update[i] = u, Y[i] = y;
        }
    }
    sh[threadIdx.x] = g2;
    __syncthreads();
#pragma unroll
    for (int o = UPD_T / 2; o; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) gsq[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(UPD_T) void tsne_stats_kernel(const double* __restrict__ zblk,
                                                           const double* __restrict__ klblk, int n_zblk,
                                                           const double* __restrict__ gsq, int n_gsq, int N,
                                                           double* __restrict__ stats) {
    __shared__ double sh[UPD_T];
    const double Z = fmax(block_sum_strided<UPD_T>(zblk, n_zblk, sh), 2.220446049250313e-16);
    const double kl = block_sum_strided<UPD_T>(klblk, n_zblk, sh);
    const double g2 = block_sum_strided<UPD_T>(gsq, n_gsq, sh);
    if (threadIdx.x == 0) stats[0] = kl + log(Z), stats[1] = Z, stats[2] = sqrt(g2);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int transpose_splits(int N) { return std::max(1, std::min(128, std::min(N / 256, (1 << 24) / N))); }

struct AffWs {
    size_t pc, cnt, rptr, rcol, rval, fcol, fval, total;
    int n_split;
    AffWs(int N, int k) {
        const size_t nk = (size_t)N * k;
        n_split = transpose_splits(N);
        size_t o = 0;
        pc = o, o += align256(nk * 4);
        cnt = o, o += align256((size_t)n_split * N * 4);
        rptr = o, o += align256(((size_t)N + 1) * 4);
        rcol = o, o += align256(nk * 4);
        rval = o, o += align256(nk * 4);
        fcol = o, o += align256(nk * 4);
        fval = o, o += align256(nk * 4);
        total = o;
    }
};

// The repulsion's split of j: at least 64 j per split, and about 8192 blocks of two waves where N allows (measured at
// N = 46715: 0.46 ms at 2048 blocks, 0.41 at 4096, 0.385 at 5888 = the 64-split cap; N = 2000 gets 4 x 32 blocks).
void rep_plan(int N, int* n_split, int* jr) {
    const int n_it = (N + REP_IB - 1) / REP_IB;
    int s = std::min({REP_MAX_SPLIT, (8192 + n_it - 1) / n_it, (N + 63) / 64});
    *jr = (N + s - 1) / s;
    *n_split = (N + *jr - 1) / *jr;
}

struct GradWs {
    size_t part, ar, zblk, klblk, gsq, total;
    int n_split, jr, n_ablk, n_ublk;
    explicit GradWs(int N) {
        rep_plan(N, &n_split, &jr);
        n_ablk = (N + ATTR_ROWS - 1) / ATTR_ROWS;
        n_ublk = (N + UPD_T - 1) / UPD_T;
        size_t o = 0;
        part = o, o += align256((size_t)n_split * N * 16);
        ar = o, o += align256((size_t)N * 16);
        zblk = o, o += align256((size_t)n_ablk * 8);
        klblk = o, o += align256((size_t)n_ablk * 8);
        gsq = o, o += align256((size_t)n_ublk * 8);
        total = o;
    }
};

}  // namespace

hipError_t launch_tsne_knn_sqdist(const float* X, int N, int D, const int32_t* idx, int k, float* d2, hipStream_t s) {
    hipLaunchKernelGGL(tsne_sqdist_kernel, dim3((N + 3) / 4), dim3(256), 0, s, X, N, D, idx, k, d2);
    return hipGetLastError();
}

size_t tsne_affinities_workspace(int N, int k) { return AffWs(N, k).total; }

hipError_t launch_tsne_affinities(const int32_t* idx, const float* d2, int N, int k, float perplexity, int32_t* indptr,
                                  int32_t* col, float* val, float* beta, void* ws, hipStream_t s) {
    const AffWs w(N, k);
    char* base = (char*)ws;
    float* pc = (float*)(base + w.pc);
    int32_t* cnt = (int32_t*)(base + w.cnt);
    int32_t* rptr = (int32_t*)(base + w.rptr);
    int32_t* rcol = (int32_t*)(base + w.rcol);
    float* rval = (float*)(base + w.rval);
    int32_t* fcol = (int32_t*)(base + w.fcol);
    float* fval = (float*)(base + w.fval);
    const int64_t nk = (int64_t)N * k;
    const int S = w.n_split, rps = (N + S - 1) / S;
    const size_t cnt_bytes = (size_t)S * N * 4;
    hipError_t e;
    hipLaunchKernelGGL(tsne_search_kernel, dim3((N + 3) / 4), dim3(256), 0, s, d2, N, k, std::log((double)perplexity),
                       beta, pc);
    // P_cond -> its transpose (each row's reverse neighbours, ascending)
    if ((e = hipMemsetAsync(cnt, 0, cnt_bytes, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(tsne_transpose_kernel<false>, dim3(S), dim3(64), 0, s, (const int32_t*)nullptr, idx,
                       (const float*)pc, N, k, rps, cnt, (const int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr,
                       nk);
    hipLaunchKernelGGL(tsne_offsets_kernel, dim3((N + 255) / 256), dim3(256), 0, s, cnt, N, S, rptr);
    hipLaunchKernelGGL(tsne_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, rptr, N);
    hipLaunchKernelGGL(tsne_transpose_kernel<true>, dim3(S), dim3(64), 0, s, (const int32_t*)nullptr, idx,
                       (const float*)pc, N, k, rps, cnt, (const int32_t*)rptr, rcol, rval, nk);
    // ... and back: each row's own neighbours, ascending
    if ((e = hipMemsetAsync(cnt, 0, cnt_bytes, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(tsne_transpose_kernel<false>, dim3(S), dim3(64), 0, s, (const int32_t*)rptr,
                       (const int32_t*)rcol, (const float*)rval, N, k, rps, cnt, (const int32_t*)nullptr,
                       (int32_t*)nullptr, (float*)nullptr, nk);
    hipLaunchKernelGGL(tsne_offsets_kernel, dim3((N + 255) / 256), dim3(256), 0, s, cnt, N, S, (int32_t*)nullptr);
    hipLaunchKernelGGL(tsne_transpose_kernel<true>, dim3(S), dim3(64), 0, s, (const int32_t*)rptr,
                       (const int32_t*)rcol, (const float*)rval, N, k, rps, cnt, (const int32_t*)nullptr, fcol, fval,
                       nk);
    // merge
    hipLaunchKernelGGL(tsne_merge_kernel<false>, dim3((N + 255) / 256), dim3(256), 0, s, (const int32_t*)fcol,
                       (const float*)fval, (const int32_t*)rptr, (const int32_t*)rcol, (const float*)rval, N, k, indptr,
                       col, val, 2 * nk);
    hipLaunchKernelGGL(tsne_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, indptr, N);
    hipLaunchKernelGGL(tsne_merge_kernel<true>, dim3((N + 255) / 256), dim3(256), 0, s, (const int32_t*)fcol,
                       (const float*)fval, (const int32_t*)rptr, (const int32_t*)rcol, (const float*)rval, N, k, indptr,
                       col, val, 2 * nk);
    return hipGetLastError();
}

size_t tsne_gradient_workspace(int N) { return GradWs(N).total; }

static void launch_rep(const float2* Y, int N, const GradWs& w, float4* part, hipStream_t s) {
    hipLaunchKernelGGL(tsne_rep_kernel, dim3((N + REP_IB - 1) / REP_IB, w.n_split), dim3(REP_T), 0, s, Y, N, w.jr, part);
}

hipError_t launch_tsne_repulsion(const float* Y, int N, void* ws, hipStream_t s) {
    const GradWs w(N);
    launch_rep((const float2*)Y, N, w, (float4*)((char*)ws + w.part), s);
    return hipGetLastError();
}

hipError_t launch_tsne_steps(const int32_t* indptr, const int32_t* col, const float* val, int N, float* Y,
                             float* update, float* gains, float exaggeration, float momentum, float learning_rate,
                             int n_steps, float* grad, double* stats, void* ws, hipStream_t s) {
    const GradWs w(N);
    char* base = (char*)ws;
    float4* part = (float4*)(base + w.part);
    float4* ar = (float4*)(base + w.ar);
    double* zblk = (double*)(base + w.zblk);
    double* klblk = (double*)(base + w.klblk);
    double* gsq = (double*)(base + w.gsq);
    const int n_eval = std::max(n_steps, 1);
    for (int it = 0; it < n_eval; ++it) {
        const int last = it == n_eval - 1;
        launch_rep((const float2*)Y, N, w, part, s);
        hipLaunchKernelGGL(tsne_attr_kernel, dim3(w.n_ablk), dim3(256), 0, s, indptr, col, val, N, (const float2*)Y,
                           (const float4*)part, w.n_split, last, ar, zblk, klblk);
        hipLaunchKernelGGL(tsne_update_kernel, dim3(w.n_ublk), dim3(UPD_T), 0, s, (const float4*)ar,
                           (const double*)zblk, w.n_ablk, N, exaggeration, n_steps > 0 ? 1 : 0, momentum, learning_rate,
                           (float2*)Y, (float2*)update, (float2*)gains, (float2*)grad, gsq);
    }
    hipLaunchKernelGGL(tsne_stats_kernel, dim3(1), dim3(UPD_T), 0, s, (const double*)zblk, (const double*)klblk,
                       w.n_ablk, (const double*)gsq, w.n_ublk, N, stats);
    return hipGetLastError();
}

}  // namespace fr
