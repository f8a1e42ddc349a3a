// LBPH on the device (OpenCV LBPHFaceRecognizer restated, DESIGN.md §4 LBPH): gray u8 images -> extended-LBP codes
// -> per-cell histograms kept as u16 counts (lbph_hist), and probes x gallery chi-square distances with a
// deterministic top-k (lbph_match + lbph_merge).  Built with -ffp-contract=off: the interpolation's float32
// products and left-to-right sums are part of the contract (a fused multiply-add changes codes).
#include <cfloat>

#include "common.h"
#include "kernels.h"

namespace fr {

// ------------------------------------------------------------------------------------------------ lbph_hist
// One workgroup per (image, grid row).  The grid row's band of image rows (cell height + 2 * radius) goes through
// LDS as bytes, LBPH_TILE_BYTES at a time; the row's grid_x cell histograms sit in LDS as u32 and take LDS atomics;
// they leave as u16 pairs (P <= 65535 bounds every count).
#define LBPH_TILE_BYTES 32768
#define LBPH_THREADS 256

__global__ __launch_bounds__(LBPH_THREADS) void lbph_hist_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                                 int radius, int neighbors, int grid_x, int grid_y,
                                                                 int cw, int ch, LbphTable tab,
                                                                 uint16_t* __restrict__ counts) {
    extern __shared__ __align__(16) uint8_t lbph_smem[];
    const int nb = 1 << neighbors;
    uint32_t* hist = (uint32_t*)lbph_smem;                         // [grid_x][nb]
    uint8_t* tile = lbph_smem + (size_t)grid_x * nb * sizeof(uint32_t);  // LBPH_TILE_BYTES
    const int tid = threadIdx.x;
    const int b = blockIdx.x / grid_y, gy = blockIdx.x % grid_y;
    const uint8_t* im = img + (size_t)b * H * W;
    const int ncols = grid_x * cw;  // code columns that fall in a cell (<= W - 2 * radius)
    for (int i = tid; i < grid_x * nb; i += LBPH_THREADS) hist[i] = 0;

    const int rows_max = (LBPH_TILE_BYTES - 4) / W;  // image rows per tile (>= 63)
    const int T = rows_max - 2 * radius;              // code rows per tile
    for (int c0 = 0; c0 < ch; c0 += T) {
        const int t = min(T, ch - c0);                // code rows of this tile
        const int row0 = gy * ch + c0;                // first image row: rows [row0, row0 + t + 2r) <= H
        const uint8_t* g0 = im + (size_t)row0 * W;
        const int nbytes = (t + 2 * radius) * W;
        const int shift = (int)((uintptr_t)g0 & 3);   // LDS copy keeps the global address's dword phase
        __syncthreads();                              // the previous tile's readers (and the zeroed hist) are done
        {
            const int head = min(nbytes, (4 - shift) & 3);
            const int body = (nbytes - head) >> 2;    // whole aligned dwords
            const int tail0 = head + body * 4;
            if (tid < head) tile[shift + tid] = g0[tid];
            const uint32_t* gd = (const uint32_t*)(g0 + head);
            uint32_t* ld = (uint32_t*)(tile + shift + head);
            for (int i = tid; i < body; i += LBPH_THREADS) ld[i] = gd[i];
            if (tid < nbytes - tail0) tile[shift + tail0 + tid] = g0[tail0 + tid];
        }
        __syncthreads();
        const uint8_t* tl = tile + shift;
        for (int p = tid; p < t * ncols; p += LBPH_THREADS) {
            const int lr = p / ncols, cj = p - lr * ncols;
            const uint8_t* ctr = tl + (lr + radius) * W + cj + radius;
            const float c = (float)ctr[0];
            unsigned code = 0;
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                if (n < neighbors) {
                    const int fx = tab.off[n][0], fy = tab.off[n][1], cx = tab.off[n][2], cy = tab.off[n][3];
                    const float a00 = (float)ctr[fy * W + fx], a01 = (float)ctr[fy * W + cx];
                    const float a10 = (float)ctr[cy * W + fx], a11 = (float)ctr[cy * W + cx];
                    float v = __fmul_rn(tab.w[n][0], a00);
                    v = __fadd_rn(v, __fmul_rn(tab.w[n][1], a01));
                    v = __fadd_rn(v, __fmul_rn(tab.w[n][2], a10));
                    v = __fadd_rn(v, __fmul_rn(tab.w[n][3], a11));
                    if (v > c || fabsf(__fsub_rn(v, c)) < FLT_EPSILON) code |= 1u << n;
                }
            }
            atomicAdd(&hist[(cj / cw) * nb + code], 1u);
        }
    }
    __syncthreads();
    // grid_x * nb is even and so is every row offset: u16 pairs leave as aligned dwords
    uint32_t* out = (uint32_t*)(counts + ((size_t)b * grid_y + gy) * grid_x * nb);
    for (int i = tid; i < grid_x * nb / 2; i += LBPH_THREADS) out[i] = hist[2 * i] | (hist[2 * i + 1] << 16);
}

hipError_t launch_lbph_hist(const uint8_t* img, int B, int H, int W, int radius, int neighbors, int grid_x, int grid_y,
                            const LbphTable& tab, uint16_t* counts, hipStream_t s) {
    const int cw = (W - 2 * radius) / grid_x, ch = (H - 2 * radius) / grid_y;
    const size_t lds = (size_t)grid_x * (1u << neighbors) * sizeof(uint32_t) + LBPH_TILE_BYTES;  // <= 48 KiB
    hipLaunchKernelGGL(lbph_hist_kernel, dim3((unsigned)B * grid_y), dim3(LBPH_THREADS), lds, s, img, H, W, radius,
                       neighbors, grid_x, grid_y, cw, ch, tab, counts);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------- lbph_match
// d(a, b) = 2 / P * sum_j delta_j^2 / s_j over bins with s_j > 0, delta = ka - kb, s = ka + kb on the u16 counts:
// the term in f32 (correctly rounded division), the sum in f64.  One wave owns a (probe, row) pair's whole sum:
// lane l adds the elements j with (j / 8) % 64 == l in ascending j, then the 64 partial sums fold by xor-butterfly.
// That order depends on D alone, so a pair's distance is bitwise the same for every B, tile and split.
//
// A wave computes a PT x LBPH_RT tile of pairs per pass (each 16-byte load feeds PT or LBPH_RT pairs), a workgroup's
// four waves take consecutive row groups of its row range, and every wave keeps a sorted top-k per probe in LDS
// (lane 0 inserts; rows arrive in ascending index, so an equal distance never displaces a lower index).
#define LBPH_RT 4
#define LBPH_WAVES 4
#define LBPH_KMAX 32

__device__ __forceinline__ void lbph_unpack(const uint4& v, float* f) {
    f[0] = (float)(v.x & 0xffffu); f[1] = (float)(v.x >> 16);
    f[2] = (float)(v.y & 0xffffu); f[3] = (float)(v.y >> 16);
    f[4] = (float)(v.z & 0xffffu); f[5] = (float)(v.z >> 16);
    f[6] = (float)(v.w & 0xffffu); f[7] = (float)(v.w >> 16);
#pragma unroll
    for (int e = 0; e < 8; ++e) asm("" : "+v"(f[e]));  // convert once per count, not once per pair (no integer re-fold)
}

// Correctly rounded n / d for 0 <= n <= 2^32, 1 <= d < 2^17, two quotients at a time: the compiler's own float32
// division expansion (reciprocal, two Newton steps, two residual corrections) without the range scaling and
// special-case fix-up that only operands near the exponent limits, zeros, infinities and NaN need; on float2 the
// products and fused multiply-adds are packed instructions (two lanes' worth per issue), which round as the scalar
// ones do.  tests/test_gpu_lbph.py compares the distances with a host restatement that uses IEEE division, bit
// for bit.
typedef float lbph_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ lbph_f2 lbph_div2(lbph_f2 n, lbph_f2 d) {
    const lbph_f2 one = {1.0f, 1.0f};
    lbph_f2 r = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    lbph_f2 e = __builtin_elementwise_fma(-d, r, one);
    r = __builtin_elementwise_fma(e, r, r);
    lbph_f2 q = n * r;
    e = __builtin_elementwise_fma(-d, q, n);
    q = __builtin_elementwise_fma(e, r, q);
    e = __builtin_elementwise_fma(-d, q, n);
    return __builtin_elementwise_fma(e, r, q);
}

template <bool VEC>
__device__ __forceinline__ void lbph_load8(const uint16_t* row, int j, int D, float* f) {
    if (VEC) {  // D % 8 == 0 and 16-byte aligned rows: j + 8 <= D whenever j < D
        uint4 v = make_uint4(0, 0, 0, 0);
        if (j < D) v = *(const uint4*)(row + j);
        lbph_unpack(v, f);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (j + e < D) ? (float)row[j + e] : 0.f;
    }
}

template <int PT, bool VEC>
__global__ __launch_bounds__(LBPH_WAVES * 64) void lbph_match_kernel(const uint16_t* __restrict__ Q, int B,
                                                                     const uint16_t* __restrict__ G, int N, int D,
                                                                     double scale, int k, int rows_per_split,
                                                                     double* __restrict__ wd, int32_t* __restrict__ wi) {
    __shared__ double s_d[LBPH_WAVES][PT][LBPH_KMAX];
    __shared__ int32_t s_i[LBPH_WAVES][PT][LBPH_KMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // probe tiles along x: the workgroups that run side by side read the same gallery rows (one L2 fill feeds them all)
    const int split = blockIdx.y, n_split = gridDim.y, p0 = blockIdx.x * PT;
    for (int i = lane; i < PT * LBPH_KMAX; i += 64) {
        (&s_d[wave][0][0])[i] = INFINITY;
        (&s_i[wave][0][0])[i] = -1;
    }
    const int r_begin = split * rows_per_split, r_end = min(N, r_begin + rows_per_split);
    const uint16_t* q[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) q[p] = Q + (size_t)min(p0 + p, B - 1) * D;

    for (int r0 = r_begin + wave * LBPH_RT; r0 < r_end; r0 += LBPH_WAVES * LBPH_RT) {
        const uint16_t* g[LBPH_RT];
#pragma unroll
        for (int r = 0; r < LBPH_RT; ++r) g[r] = G + (size_t)min(r0 + r, N - 1) * D;
        double acc[PT][LBPH_RT];
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int r = 0; r < LBPH_RT; ++r) acc[p][r] = 0.0;
        for (int j = lane * 8; j < D; j += 512) {
            float fq[PT][8], fg[LBPH_RT][8];
#pragma unroll
            for (int p = 0; p < PT; ++p) lbph_load8<VEC>(q[p], j, D, fq[p]);
#pragma unroll
            for (int r = 0; r < LBPH_RT; ++r) lbph_load8<VEC>(g[r], j, D, fg[r]);
#pragma unroll
            for (int p = 0; p < PT; ++p)
#pragma unroll
                for (int r = 0; r < LBPH_RT; ++r)
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        // exact: counts < 2^16.  An empty bin pair (s = 0, so delta = 0) divides 0 by 1: its term
                        // is +0.0, which leaves the sum's bits unchanged, as skipping it does.
                        const lbph_f2 a = {fq[p][e], fq[p][e + 1]}, b = {fg[r][e], fg[r][e + 1]};
                        const lbph_f2 dl = a - b, sm = a + b;
                        const lbph_f2 t = lbph_div2(dl * dl, lbph_f2{fmaxf(sm.x, 1.f), fmaxf(sm.y, 1.f)});
                        acc[p][r] += (double)t.x;
                        acc[p][r] += (double)t.y;
                    }
        }
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int r = 0; r < LBPH_RT; ++r) {
                double v = acc[p][r];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);  // a + b == b + a: every lane the same bits
                acc[p][r] = v * scale;
            }
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                if (p0 + p >= B) continue;
                double* ld = s_d[wave][p];
                int32_t* li = s_i[wave][p];
#pragma unroll
                for (int r = 0; r < LBPH_RT; ++r) {
                    const int row = r0 + r;
                    const double d = acc[p][r];
                    if (row >= r_end || !(d < ld[k - 1])) continue;  // equal to the worst kept: the lower index stays
                    int pos = k - 1;
                    while (pos > 0 && d < ld[pos - 1]) {
                        ld[pos] = ld[pos - 1];
                        li[pos] = li[pos - 1];
                        --pos;
                    }
                    ld[pos] = d;
                    li[pos] = row;
                }
            }
        }
    }
    // list (split, wave) of probe p: workspace [B][n_split * LBPH_WAVES][k]
    const int n_lists = n_split * LBPH_WAVES;
    for (int i = lane; i < PT * k; i += 64) {
        const int p = i / k, e = i - p * k;
        if (p0 + p >= B) continue;
        const size_t o = ((size_t)(p0 + p) * n_lists + split * LBPH_WAVES + wave) * k + e;
        wd[o] = s_d[wave][p][e];
        wi[o] = s_i[wave][p][e];
    }
}

// One workgroup per probe merges its n_lists sorted lists: k rounds, each selecting the smallest (distance, index)
// above the previous pick.  Every gallery row is in at most one list, so the keys are distinct but for the
// (+inf, -1) fillers, which order last and come out as the tail when k > N.
#define LBPH_MERGE_THREADS 256

__device__ __forceinline__ bool lbph_less(double d0, int i0, double d1, int i1) {  // index -1 (filler) orders last
    if (d0 != d1) return d0 < d1;
    return (unsigned)i0 < (unsigned)i1;
}

__global__ __launch_bounds__(LBPH_MERGE_THREADS) void lbph_merge_kernel(const double* __restrict__ wd,
                                                                        const int32_t* __restrict__ wi, int n_lists,
                                                                        int k, double* __restrict__ dist,
                                                                        int32_t* __restrict__ idx) {
    __shared__ double r_d[LBPH_MERGE_THREADS];
    __shared__ int32_t r_i[LBPH_MERGE_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const size_t base = (size_t)b * n_lists * k;
    const int total = n_lists * k;
    double last_d = -1.0;  // below every distance (all >= 0)
    int last_i = 0;
    for (int round = 0; round < k; ++round) {
        double best_d = INFINITY;
        int best_i = -1;
        for (int c = tid; c < total; c += LBPH_MERGE_THREADS) {
            const double d = wd[base + c];
            const int i = wi[base + c];
            if (i >= 0 && lbph_less(last_d, last_i, d, i) && lbph_less(d, i, best_d, best_i)) {
                best_d = d;
                best_i = i;
            }
        }
        r_d[tid] = best_d;
        r_i[tid] = best_i;
        __syncthreads();
        for (int s = LBPH_MERGE_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s && lbph_less(r_d[tid + s], r_i[tid + s], r_d[tid], r_i[tid])) {
                r_d[tid] = r_d[tid + s];
                r_i[tid] = r_i[tid + s];
            }
            __syncthreads();
        }
        last_d = r_d[0];
        last_i = r_i[0];
        __syncthreads();
        if (tid == 0) {
            dist[(size_t)b * k + round] = last_d;
            idx[(size_t)b * k + round] = last_i;
        }
        if (last_i < 0) {  // nothing left: the rest is the (+inf, -1) tail
            for (int e = round + 1 + tid; e < k; e += LBPH_MERGE_THREADS) {
                dist[(size_t)b * k + e] = INFINITY;
                idx[(size_t)b * k + e] = -1;
            }
            break;
        }
    }
}

void lbph_match_plan(int B, int64_t N, int* pt, int* n_split, int* rows_per_split) {
    const int PT = B == 1 ? 1 : 4;
    const int tiles = (B + PT - 1) / PT;
    const int group = LBPH_WAVES * LBPH_RT;  // rows one workgroup pass covers
    const int64_t groups = (N + group - 1) / group;
    int64_t want = (1024 + tiles - 1) / tiles;  // about four workgroups per CU over the whole grid
    if (want > groups) want = groups;
    if (want < 1) want = 1;
    const int64_t rps = (groups + want - 1) / want * group;
    *pt = PT;
    *rows_per_split = (int)rps;
    *n_split = (int)((N + rps - 1) / rps);
}

size_t lbph_match_workspace(int B, int64_t N, int k) {
    int pt, n_split, rps;
    lbph_match_plan(B, N, &pt, &n_split, &rps);
    return (size_t)B * n_split * LBPH_WAVES * k * (sizeof(double) + sizeof(int32_t));
}

hipError_t launch_lbph_match(const uint16_t* Q, int B, const uint16_t* G, int64_t N, int D, int cell_pixels, int k,
                             double* dist, int32_t* idx, void* ws, hipStream_t s) {
    int pt, n_split, rps;
    lbph_match_plan(B, N, &pt, &n_split, &rps);
    const int n_lists = n_split * LBPH_WAVES;
    double* wd = (double*)ws;
    int32_t* wi = (int32_t*)(wd + (size_t)B * n_lists * k);
    const bool vec = D % 8 == 0 && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)G & 15) == 0;
    const double scale = 2.0 / (double)cell_pixels;
    const dim3 grid((unsigned)((B + pt - 1) / pt), (unsigned)n_split), block(LBPH_WAVES * 64);
#define LBPH_LAUNCH(PT_, VEC_)                                                                                  \
    hipLaunchKernelGGL((lbph_match_kernel<PT_, VEC_>), grid, block, 0, s, Q, B, G, (int)N, D, scale, k, rps, wd, wi)
    if (pt == 1) {
        if (vec) LBPH_LAUNCH(1, true); else LBPH_LAUNCH(1, false);
    } else {
        if (vec) LBPH_LAUNCH(4, true); else LBPH_LAUNCH(4, false);
    }
#undef LBPH_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lbph_merge_kernel, dim3((unsigned)B), dim3(LBPH_MERGE_THREADS), 0, s, wd, wi, n_lists, k, dist,
                       idx);
    return hipGetLastError();
}

}  // namespace fr
