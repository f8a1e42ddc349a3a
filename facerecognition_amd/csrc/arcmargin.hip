// ArcFace additive-angular-margin softmax loss (the reference's ArcMarginProduct + CrossEntropyLoss with label
// smoothing and mixup), forward and backward, without a B x C matrix (DESIGN.md §4 "ArcFace margin loss").
//
// Replaces: models/arcface/arcface_model.py:23-62 (cosine, one-hot and output, three B x C tensors, plus
// autograd's copies) and the criterion of train_arcface.py:109-111.
//
// Scores are exact f32: score_tile.h's v_mfma_f32_16x16x4f32 tile loop (64 rows x 64 rows, D staged through LDS in
// 64-float chunks, k = 16 t16 + 4 (lane >> 4) + c), the raw dot scaled by inv_e[b] inv_w[j] in the epilogue.
//   norms_kernel    inv[r] = 1 / max(|x_r|, 1e-12), IEEE sqrt and division (rows of norm 1 give exactly 1)
//   fwd_kernel      64 probes x one class split: per 64-class tile the label transform and an online
//                   (max, sum exp, sum z, z at y, z at y') per probe; one partial per (probe, split); optionally z
//   fwd_merge       partials in split order -> lse, loss
//   bwd_kernel<T>   T = false (dE): 64 probes x one class split; T = true (dW): one 64-class tile x all probes.
//                   Per tile: the score tile again, g (from (lse, targets, u) or from dense dlogits) into LDS,
//                   then acc += g (64 x 64) . other-side tile (64 x D) with the same MFMA, the other side staged
//                   through LDS a second time.  dE: one [B, D] partial per split; dW: every row has one owner.
//   jacobian_kernel partials in split order, then the normalise Jacobian (d - (d . x^) x^) / max(|x|, 1e-12)
//   The next D chunk is loaded into registers while the current chunk's MFMAs run (score and product loops).
// No float atomics; every sum runs in an order fixed by (B, C, D).
#include "score_tile.h"
#include <float.h>

#include <algorithm>

namespace fr {
using namespace tile;
namespace {

constexpr int PREC = 8;  // floats per forward partial: {max, sum exp, sum z, z at y, z at y', -, -, -}

__global__ __launch_bounds__(256) void norms_kernel(const float* __restrict__ X, int64_t R, int D, float* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float ss = row_sqsum(X + (size_t)r * D, D);
    if (lane == 0) inv[r] = __fdiv_rn(1.f, fmaxf(__fsqrt_rn(ss), 1e-12f));
}

// The label logit and its derivative by the cosine (torch's rules for clamp, where and sqrt).
__device__ __forceinline__ float margin_z(const ArcArgs& a, float c, float* dz) {
    const float q = 1.f - c * c;
    const float sine = __fsqrt_rn(fmaxf(q, 1e-7f));
    const bool on = a.easy_margin ? (c > 0.f) : (c > a.th);
    *dz = on ? a.cos_m + (q >= 1e-7f ? a.sin_m * c / sine : 0.f) : 1.f;
    return on ? c * a.cos_m - sine * a.sin_m : (a.easy_margin ? c : c - a.mm);
}

__global__ __launch_bounds__(256) void fwd_kernel(const ArcArgs a, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sXY[2 * MT * LD];
    __shared__ float sS[MT * SLD];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * MT;
    const int64_t c_begin = (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t c_end = std::min<int64_t>(c_begin + a.rows_per_split, a.C);

    const int my_p = tid >> 2, my_sub = tid & 3;
    const int64_t b = p0 + my_p;
    const bool live = b < a.B;
    const int64_t bc = live ? b : a.B - 1;
    const float ie = a.inv_e[bc];
    const int y = a.label[bc];
    const int yb = a.label_b ? a.label_b[bc] : -1;
    float m = -INFINITY, se = 0.f, sz = 0.f, zy = 0.f, zyb = 0.f;

    for (int64_t t0 = c_begin; t0 < c_end; t0 += MT) {
        f32x4_t acc[4];
        score_tile_prefetch<int64_t, int64_t>(a.E, a.B, p0, a.W, c_end, t0, a.D, sXY, sXY + MT * LD, acc);
        store_score_tile(sS, acc);
        __syncthreads();
        const float* row = sS + my_p * SLD + my_sub * 16;
        const int64_t jb = t0 + my_sub * 16;
        const int l = (int)std::min<int64_t>(16, c_end - jb);  // valid columns of this thread (may be <= 0)
        float z[16];
        float tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            z[i] = -INFINITY;
            if (i < l) {
                const int64_t j = jb + i;
                float c = row[i] * ie * a.inv_w[j], dz;
                if (j == y) c = margin_z(a, c, &dz);
                z[i] = a.scale * c;
                if (j == y) zy = z[i];
                if (j == yb) zyb = z[i];
                sz += z[i];
                tm = fmaxf(tm, z[i]);
                if (a.logits && live) a.logits[(size_t)b * a.C + j] = z[i];
            }
        }
        if (l > 0) {
            if (tm > m) {
                se *= expf(m - tm);
                m = tm;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i < l) se += expf(z[i] - m);
        }
        __syncthreads();
    }
    // the probe's 4 sub-threads in order 0..3 (sub-thread 0 always saw a column)
    const int base = (tid & 63) & ~3;
    float M = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) M = fmaxf(M, __shfl(m, base + k));
    float SE = 0.f, SZ = 0.f, ZY = 0.f, ZYB = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float mk = __shfl(m, base + k), sk = __shfl(se, base + k);
        SE += mk == -INFINITY ? 0.f : sk * expf(mk - M);
        SZ += __shfl(sz, base + k);
        ZY += __shfl(zy, base + k);
        ZYB += __shfl(zyb, base + k);
    }
    if (my_sub == 0 && live) {
        float* o = part + ((size_t)b * a.n_split + blockIdx.y) * PREC;
        o[0] = M; o[1] = SE; o[2] = SZ; o[3] = ZY; o[4] = ZYB;
    }
}

// The weights of the two cross-entropy terms: a label outside [0, C) switches its term off.
__device__ __forceinline__ void term_weights(const ArcArgs& a, int y, int yb, float* la, float* lb) {
    *la = (y >= 0 && y < a.C) ? a.lam : 0.f;
    *lb = (a.label_b && yb >= 0 && yb < a.C) ? 1.f - a.lam : 0.f;
}

__global__ __launch_bounds__(256) void fwd_merge_kernel(const ArcArgs a, const float* __restrict__ part) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    const float* p = part + (size_t)b * a.n_split * PREC;
    float M = -INFINITY;
    for (int k = 0; k < a.n_split; ++k) M = fmaxf(M, p[k * PREC]);
    float se = 0.f, sz = 0.f, zy = 0.f, zyb = 0.f;
    for (int k = 0; k < a.n_split; ++k) {
        se += p[k * PREC + 1] * expf(p[k * PREC] - M);
        sz += p[k * PREC + 2];
        zy += p[k * PREC + 3];
        zyb += p[k * PREC + 4];
    }
    const float lse = M + logf(se);
    float la, lb;
    term_weights(a, a.label[b], a.label_b ? a.label_b[b] : -1, &la, &lb);
    const float eps = a.label_smoothing;
    const float smooth = eps * (lse - sz / (float)a.C);
    float loss = 0.f;
    if (la != 0.f) loss += la * ((1.f - eps) * (lse - zy) + smooth);
    if (lb != 0.f) loss += lb * ((1.f - eps) * (lse - zyb) + smooth);
    a.lse[b] = lse;
    a.loss[b] = loss;
}

// What g needs of one probe.
struct ProbeCtx {
    float ie, lse, u, la, lb;
    int y, yb;
};

__device__ __forceinline__ ProbeCtx probe_ctx(const ArcArgs& a, int64_t b) {
    ProbeCtx p;
    p.ie = a.inv_e[b];
    p.y = a.label[b];
    p.yb = a.label_b ? a.label_b[b] : -1;
    term_weights(a, p.y, p.yb, &p.la, &p.lb);
    p.lse = a.dlogits ? 0.f : a.lse[b];
    p.u = a.dlogits ? 0.f : a.u[b];
    return p;
}

// dL/dc at (b, j) from the raw dot product.
template <bool DENSE>
__device__ __forceinline__ float g_value(const ArcArgs& a, const ProbeCtx& p, int64_t b, int64_t j, float iw, float dot) {
    float c = dot * p.ie * iw, dz = 1.f;
    if (j == p.y) c = margin_z(a, c, &dz);
    float g;
    if (DENSE) {
        g = a.dlogits[(size_t)b * a.C + j];
    } else {
        const float eps = a.label_smoothing;
        const float sm = eps / (float)a.C;
        const float tgt = p.la * ((j == p.y ? 1.f - eps : 0.f) + sm) + p.lb * ((j == p.yb ? 1.f - eps : 0.f) + sm);
        g = p.u * ((p.la + p.lb) * expf(a.scale * c - p.lse) - tgt);
    }
    return g * a.scale * dz;
}

// TRANS = false: X = E, Y = W, block (x, y, z) = (64-probe tile, class split, D chunk), out = partial [split][B][D].
// TRANS = true:  X = W, Y = E, block (x, -, z) = (64-class tile, -, D chunk) over all probes, out = dW^ [C][D].
// acc[ch][f][r] = out[x0 + 16 wave + 4 (lane >> 4) + r][dz0 + 64 ch + 16 f + (lane & 15)].
template <bool TRANS, bool DENSE, int DCH>
__global__ __launch_bounds__(256) void bwd_kernel(const ArcArgs a, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float sXY[2 * MT * LD];
    __shared__ float sS[MT * SLD];
    float* sX = sXY;
    float* sY = sXY + MT * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ X = TRANS ? a.W : a.E;
    const float* __restrict__ Y = TRANS ? a.E : a.W;
    const int64_t rx = TRANS ? a.C : a.B;
    const int64_t x0 = (int64_t)blockIdx.x * MT;
    const int64_t y_begin = TRANS ? 0 : (int64_t)blockIdx.y * a.rows_per_split;
    const int64_t y_end = TRANS ? a.B : std::min<int64_t>(y_begin + a.rows_per_split, a.C);
    const int D = a.D, dz0 = blockIdx.z * DCH;

    const int my_r = tid >> 2, my_sub = tid & 3;
    const int64_t xr = x0 + my_r;
    const bool live = xr < rx;
    ProbeCtx pc;
    float iw = 0.f;
    if (TRANS) iw = a.inv_w[live ? xr : rx - 1];
    else pc = probe_ctx(a, live ? xr : rx - 1);

    f32x4_t acc[DCH / KC][4];
#pragma unroll
    for (int ch = 0; ch < DCH / KC; ++ch)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[ch][f] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    for (int64_t t0 = y_begin; t0 < y_end; t0 += MT) {
        f32x4_t sc[4];
        score_tile_prefetch<int64_t, int64_t>(X, rx, x0, Y, y_end, t0, D, sX, sY, sc);
        store_score_tile(sS, sc);
        __syncthreads();
        {   // the score tile -> g, scaled by the walked side's 1 / norm (its rows enter the product raw)
            float* row = sS + my_r * SLD + my_sub * 16;
            const int64_t cb = t0 + my_sub * 16;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t yc = cb + i;
                float g = 0.f;
                if (live && yc < y_end) {
                    if (TRANS) {
                        const ProbeCtx q = probe_ctx(a, yc);
                        g = g_value<DENSE>(a, q, yc, xr, iw, row[i]) * q.ie;
                    } else {
                        const float jw = a.inv_w[yc];
                        g = g_value<DENSE>(a, pc, xr, yc, jw, row[i]) * jw;
                    }
                }
                row[i] = g;
            }
        }
        __syncthreads();
        // acc += g . Y tile, k = the tile's 64 rows: step t has k = 4 t + (lane >> 4); the next chunk of the Y tile
        // is loaded into registers while this chunk's MFMAs run
        float4 yv[4];
        auto load_y = [&](int d0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = tid + 256 * i;
                const int r = q >> 4, c4 = (q & 15) * 4;
                yv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t0 + r < y_end && d0 + c4 < D) yv[i] = *(const float4*)(Y + (size_t)(t0 + r) * D + d0 + c4);
            }
        };
        load_y(dz0);
#pragma unroll
        for (int ch = 0; ch < DCH / KC; ++ch) {
            const int d0 = dz0 + ch * KC;
            if (d0 < D) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int q = tid + 256 * i;
                    *(float4*)(sY + (q >> 4) * LD + (q & 15) * 4) = yv[i];
                }
                __syncthreads();
                if (ch + 1 < DCH / KC && d0 + KC < D) load_y(d0 + KC);
#pragma unroll
                for (int t = 0; t < MT / 4; ++t) {
                    const int k = 4 * t + (lane >> 4);
                    const float av = sS[(16 * wave + (lane & 15)) * SLD + k];
#pragma unroll
                    for (int f = 0; f < 4; ++f)
                        acc[ch][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sY[k * LD + 16 * f + (lane & 15)], acc[ch][f], 0, 0, 0);
                }
                __syncthreads();
            }
        }
    }

    float* o = out + (TRANS ? (size_t)0 : (size_t)blockIdx.y * a.B * D);
#pragma unroll
    for (int ch = 0; ch < DCH / KC; ++ch)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int d = dz0 + ch * KC + 16 * f + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t xo = x0 + 16 * wave + 4 * (lane >> 4) + r;
                if (xo < rx && d < D) o[(size_t)xo * D + d] = acc[ch][f][r];
            }
        }
}

// out[r] = (d - (d . x^) x^) inv[r] with d = sum_k part[k][r] in split order and x^ = X[r] inv[r]; without the
// projection where the norm clamp was active (F.normalize's clamp_min passes no gradient there).  part may be out
// (n_split = 1): every element is read and written by the same thread, on either side of the barrier.
__global__ __launch_bounds__(256) void jacobian_kernel(const float* part, int n_split, int64_t R, int D,
                                                       const float* __restrict__ X, const float* __restrict__ inv,
                                                       float* out) {
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const float iv = inv[r];
    const float* x = X + (size_t)r * D;
    float dot = 0.f;
    for (int d = tid; d < D; d += 256) {
        float s = 0.f;
        for (int k = 0; k < n_split; ++k) s += part[((size_t)k * R + r) * D + d];
        dot += s * (x[d] * iv);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o);
    if ((tid & 63) == 0) red[tid >> 6] = dot;
    __syncthreads();
    dot = ((red[0] + red[1]) + red[2]) + red[3];
    if (iv >= 1e12f) dot = 0.f;
    for (int d = tid; d < D; d += 256) {
        float s = 0.f;
        for (int k = 0; k < n_split; ++k) s += part[((size_t)k * R + r) * D + d];
        out[(size_t)r * D + d] = (s - dot * (x[d] * iv)) * iv;
    }
}

template <bool TRANS, bool DENSE>
void launch_bwd(const ArcArgs& a, float* out, dim3 grid, hipStream_t s) {
    const int D = a.D;
    if (D <= 64) {
        hipLaunchKernelGGL((bwd_kernel<TRANS, DENSE, 64>), grid, dim3(256), 0, s, a, out);
    } else if (D <= 128) {
        hipLaunchKernelGGL((bwd_kernel<TRANS, DENSE, 128>), grid, dim3(256), 0, s, a, out);
    } else if (D <= 256) {
        hipLaunchKernelGGL((bwd_kernel<TRANS, DENSE, 256>), grid, dim3(256), 0, s, a, out);
    } else {
        grid.z = (D + 511) / 512;
        hipLaunchKernelGGL((bwd_kernel<TRANS, DENSE, 512>), grid, dim3(256), 0, s, a, out);
    }
}

}  // namespace

// Class splits, whole 64-class tiles each, a function of (B, C) alone.  Forward: about three workgroups per CU over
// the (probe tile, split) grid (its partials are 8 floats per probe and split).  Backward: about two per CU and at
// most 64 splits (the dE partials are n_split x B x D floats).
void arcmargin_plan(int B, int C, bool fwd, int* n_split, int64_t* rows_per_split) {
    const int pblocks = (B + MT - 1) / MT;
    const int tiles = (C + MT - 1) / MT;
    const int want = fwd ? std::max(1, std::min(256, 768 / pblocks)) : std::max(1, std::min(64, 512 / pblocks));
    const int tps = (tiles + want - 1) / want;
    *rows_per_split = (int64_t)tps * MT;
    *n_split = (tiles + tps - 1) / tps;
}

static size_t fwd_partial_floats(int B, int C) {
    int ns;
    int64_t rps;
    arcmargin_plan(B, C, true, &ns, &rps);
    return (size_t)B * ns * PREC;
}

size_t arcmargin_workspace(int B, int C, int D) {
    int ns;
    int64_t rps;
    arcmargin_plan(B, C, false, &ns, &rps);
    return (fwd_partial_floats(B, C) + (size_t)ns * B * D) * sizeof(float);
}

hipError_t launch_arcmargin_forward(ArcArgs a, void* ws, hipStream_t s) {
    arcmargin_plan(a.B, a.C, true, &a.n_split, &a.rows_per_split);
    float* part = (float*)ws;
    hipLaunchKernelGGL(norms_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a.E, (int64_t)a.B, a.D, a.inv_e_out);
    hipLaunchKernelGGL(norms_kernel, dim3((a.C + 3) / 4), dim3(256), 0, s, a.W, (int64_t)a.C, a.D, a.inv_w_out);
    a.inv_e = a.inv_e_out;
    a.inv_w = a.inv_w_out;
    hipLaunchKernelGGL(fwd_kernel, dim3((a.B + MT - 1) / MT, a.n_split), dim3(256), 0, s, a, part);
    hipLaunchKernelGGL(fwd_merge_kernel, dim3((a.B + 255) / 256), dim3(256), 0, s, a, part);
    return hipGetLastError();
}

hipError_t launch_arcmargin_backward(ArcArgs a, float* dE, float* dW, void* ws, hipStream_t s) {
    arcmargin_plan(a.B, a.C, false, &a.n_split, &a.rows_per_split);
    const bool dense = a.dlogits != nullptr;
    if (dE) {
        float* part = (float*)ws + fwd_partial_floats(a.B, a.C);
        const dim3 grid((a.B + MT - 1) / MT, a.n_split, 1);
        if (dense) launch_bwd<false, true>(a, part, grid, s);
        else launch_bwd<false, false>(a, part, grid, s);
        hipLaunchKernelGGL(jacobian_kernel, dim3(a.B), dim3(256), 0, s, part, a.n_split, (int64_t)a.B, a.D, a.E, a.inv_e, dE);
    }
    if (dW) {
        const dim3 grid((a.C + MT - 1) / MT, 1, 1);
        if (dense) launch_bwd<true, true>(a, dW, grid, s);
        else launch_bwd<true, false>(a, dW, grid, s);
        hipLaunchKernelGGL(jacobian_kernel, dim3(a.C), dim3(256), 0, s, dW, 1, (int64_t)a.C, a.D, a.W, a.inv_w, dW);
    }
    return hipGetLastError();
}

}  // namespace fr
