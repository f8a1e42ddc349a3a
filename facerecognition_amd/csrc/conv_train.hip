// Convolution and BatchNorm2d in training mode, forward and backward, for ResNet-50's layer4 (DESIGN.md §4 "Backbone
// training: layer4"; formulas in include/frhip.h "Backbone training"): physical NHWC activations, [Cout][Kh][Kw][Cin]
// weights, caller-owned f32 buffers.
//
// Replaces: torchvision's Bottleneck under autograd as models/arcface/arcface_model.py:223 (freeze_layers, ratio 0.8)
// leaves it trainable: F.conv2d, F.batch_norm, ReLU, the residual add and autograd's copies of every intermediate.
//
// A convolution's operand A = relu?(X scale + shift) is never stored: conv_a4 recomputes four elements of it from X
// and the folded BN of the layer before wherever a tile of it is staged into LDS (forward product, dW product), and
// returns +0 for a padded tap (the padding is zero in A-space).  Products are exact f32 on v_mfma_f32_16x16x4f32,
// 64 x 64 tiles, the inner dimension staged through LDS in 64s, as head_train.hip's two GEMMs.
//   conv_fwd_kernel    64 output pixels x 64 output channels x one K split, K = (r, s, c) -> Z or partial [split][M][N]
//   conv_merge_kernel  partials in split order -> Z
//   conv_bwd_kernel    T = true: dW = dZ^T A, reducing over the M output pixels (one owner per element);
//                      T = false: dA = gather(dZ) Wt', 64 input pixels x 64 input channels, reducing over (r, s, n)
//                      with the taps that meet no output pixel staged as zeros
//   bn2d_stats_kernel  mean, rstd, the running update and the folded scale / shift of 16 channels per block
//   bn_act_fwd_kernel  Y = relu?(Z scale + shift + Res?)
//   bn_act_bwd_kernel  dgamma, dbeta, dZ and dRes of 16 channels per block
// No float atomics; every sum runs in an order fixed by the shape.
#include "kernels.h"

#include <algorithm>

namespace fr {
namespace {

constexpr int MT = 64;  // rows per tile, both sides
constexpr int KC = 64;  // inner chunk (floats)
constexpr int LD = KC + 4;
constexpr int SLD = MT + 1;

// Output pixel m -> (b, oh, ow).
struct Pix {
    int b, y, x;
};
__device__ __forceinline__ Pix pix_of(int64_t m, int h, int w) {
    const int hw = h * w;
    Pix p;
    p.b = (int)(m / hw);
    const int rem = (int)(m - (int64_t)p.b * hw);
    p.y = rem / w;
    p.x = rem - p.y * w;
    return p;
}

// A[(b, oh, ow)][kk .. kk + 3] with kk = (r Kw + s) Cin + c (kk % 4 == 0): the transformed input under tap (r, s), or
// +0 where the tap falls into the padding.
__device__ __forceinline__ float4 conv_a4(const ConvTrainArgs& a, const Pix& p, int kk) {
    const int tap = kk / a.Cin, c = kk - tap * a.Cin;
    const int r = tap / a.k, s = tap - r * a.k;
    const int h = p.y * a.stride + r - a.pad, w = p.x * a.stride + s - a.pad;
    if ((unsigned)h >= (unsigned)a.H || (unsigned)w >= (unsigned)a.W) return make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = *(const float4*)(a.X + (((size_t)p.b * a.H + h) * a.W + w) * a.Cin + c);
    if (a.scale) {
        const float4 sc = *(const float4*)(a.scale + c), sh = *(const float4*)(a.shift + c);
        v.x = fmaf(v.x, sc.x, sh.x);
        v.y = fmaf(v.y, sc.y, sh.y);
        v.z = fmaf(v.z, sc.z, sh.z);
        v.w = fmaf(v.w, sc.w, sh.w);
        if (a.relu) {
            v.x = v.x > 0.f ? v.x : 0.f;
            v.y = v.y > 0.f ? v.y : 0.f;
            v.z = v.z > 0.f ? v.z : 0.f;
            v.w = v.w > 0.f ? v.w : 0.f;
        }
    }
    return v;
}

// out[z][m][n] = sum over K split z of A[m][kk] Wt[n][kk].  Block (x, y, z) = (64-pixel tile, 64-channel tile, split).
__global__ __launch_bounds__(256) void conv_fwd_kernel(const ConvTrainArgs a, int k_per_split, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float sX[MT * LD];
    __shared__ __attribute__((aligned(16))) float sY[MT * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t M = (int64_t)a.B * a.OH * a.OW;
    const int K = a.k * a.k * a.Cin, N = a.Cout;
    const int64_t m0 = (int64_t)blockIdx.x * MT;
    const int n0 = blockIdx.y * MT;
    const int k_begin = blockIdx.z * k_per_split;
    const int k_end = std::min(K, k_begin + k_per_split);
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    Pix px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (tid + 256 * i) >> 4;
        px[i] = pix_of(std::min(m0 + row, M - 1), a.OH, a.OW);
    }
    // chunk d0 + KC is loaded into registers while chunk d0's MFMAs run
    float4 xv[4], yv[4];
    auto load = [&](int d0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            const int row = q >> 4, c4 = (q & 15) * 4;
            xv[i] = yv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m0 + row < M && d0 + c4 < K) xv[i] = conv_a4(a, px[i], d0 + c4);
            if (n0 + row < N && d0 + c4 < K) yv[i] = *(const float4*)(a.Wt + (size_t)(n0 + row) * K + d0 + c4);
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
    float* o = out + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + 16 * wave + 4 * (lane >> 4) + r;
            if (m < M && n < N) o[(size_t)m * N + n] = acc[j][r];
        }
    }
}

__global__ __launch_bounds__(256) void conv_merge_kernel(const float* __restrict__ part, int n_split, int64_t total4,
                                                         float* __restrict__ Z) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total4; q += (int64_t)gridDim.x * 256) {
        float4 s = *(const float4*)(part + 4 * (size_t)q);
        for (int k = 1; k < n_split; ++k) {
            const float4 v = *(const float4*)(part + ((size_t)k * total4 + (size_t)q) * 4);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *(float4*)(Z + 4 * (size_t)q) = s;
    }
}

// out[r][c] = sum_i L(r, i) R(i, c), block (x, y) = (64-row tile, 64-column tile).
// T = true  (dW): r = output channel n, i = output pixel m, c = kk = (tap, c); L = dZ[m][n], R = A[m][kk];
//                 out = dW [Cout][K].
// T = false (dA): r = input pixel (b, h, w), i = (tap, n), c = input channel; L = dZ[b][oh][ow][n] with
//                 oh stride + r - pad = h (likewise w), or 0 where no such output pixel exists; R = Wt[n][tap][c];
//                 out = dA [B H W][Cin].
template <bool T>
__global__ __launch_bounds__(256) void conv_bwd_kernel(const ConvTrainArgs a, const float* __restrict__ dZ,
                                                       float* __restrict__ out) {
    __shared__ float sL[MT * SLD];
    __shared__ __attribute__((aligned(16))) float sR[MT * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t M = (int64_t)a.B * a.OH * a.OW;
    const int taps = a.k * a.k, K = taps * a.Cin, N = a.Cout;
    const int64_t rows = T ? (int64_t)N : (int64_t)a.B * a.H * a.W;
    const int64_t inner = T ? M : (int64_t)taps * N;
    const int cols = T ? K : a.Cin;
    const int64_t r0 = (int64_t)blockIdx.x * MT;
    const int c0 = blockIdx.y * MT;
    f32x4_t acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    Pix px[4];  // T = false: the tile's input pixels of this thread's four staging rows
    if (!T) {
#pragma unroll
        for (int t = 0; t < 4; ++t) px[t] = pix_of(std::min(r0 + ((tid + 256 * t) >> 4), rows - 1), a.H, a.W);
    }
    for (int64_t i0 = 0; i0 < inner; i0 += KC) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = tid + 256 * t;
            const int row = q >> 4, c4 = (q & 15) * 4;
            float4 l = make_float4(0.f, 0.f, 0.f, 0.f), r = l;
            if (T) {  // row = output pixel within the chunk, c4 = output channel within the tile
                if (i0 + row < M) {
                    if (r0 + c4 < N) l = *(const float4*)(dZ + (size_t)(i0 + row) * N + r0 + c4);
                    if (c0 + c4 < K) r = conv_a4(a, pix_of(i0 + row, a.OH, a.OW), c0 + c4);
                }
                sL[(c4 + 0) * SLD + row] = l.x;
                sL[(c4 + 1) * SLD + row] = l.y;
                sL[(c4 + 2) * SLD + row] = l.z;
                sL[(c4 + 3) * SLD + row] = l.w;
            } else {  // row = input pixel within the tile, c4 = (tap, n) within the chunk
                if (r0 + row < rows && i0 + c4 < inner) {
                    const int i = (int)(i0 + c4);
                    const int tap = i / N, n = i - tap * N;
                    const int kr = tap / a.k, ks = tap - kr * a.k;
                    const int hn = px[t].y + a.pad - kr, wn = px[t].x + a.pad - ks;
                    const int oh = hn / a.stride, ow = wn / a.stride;
                    if (hn >= 0 && wn >= 0 && oh * a.stride == hn && ow * a.stride == wn && oh < a.OH && ow < a.OW)
                        l = *(const float4*)(dZ + (((size_t)px[t].b * a.OH + oh) * a.OW + ow) * N + n);
                }
                sL[row * SLD + c4 + 0] = l.x;
                sL[row * SLD + c4 + 1] = l.y;
                sL[row * SLD + c4 + 2] = l.z;
                sL[row * SLD + c4 + 3] = l.w;
                if (i0 + row < inner && c0 + c4 < cols) {
                    const int i = (int)(i0 + row);
                    const int tap = i / N, n = i - tap * N;
                    r = *(const float4*)(a.Wt + ((size_t)n * taps + tap) * a.Cin + c0 + c4);
                }
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
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int c = c0 + 16 * f + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t ro = r0 + 16 * wave + 4 * (lane >> 4) + r;
            if (ro < rows && c < cols) out[(size_t)ro * cols + c] = acc[f][r];
        }
    }
}

// BN over the rows of Z [M][C]: 16 channels per block, row r belongs to group r % 16 (head_train.hip's bn_cols_kernel
// plus the folded affine).
__global__ __launch_bounds__(256) void bn2d_stats_kernel(const float* __restrict__ Z, int64_t M, int C,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ rm, float* __restrict__ rv, bool batch,
                                                         float eps, float momentum, float* __restrict__ mean_out,
                                                         float* __restrict__ rstd_out, float* __restrict__ scale_out,
                                                         float* __restrict__ shift_out) {
    __shared__ float red[16 * 17];
    const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool live = c < C;
    const int cc = live ? c : C - 1;
    float mean, var;
    if (batch) {
        const float n = (float)M;
        float s = 0.f;
        if (live)
            for (int64_t r = g; r < M; r += 16) s += Z[(size_t)r * C + c];
        mean = __fdiv_rn(col_sum16(s, red), n);
        float q = 0.f;
        if (live)
            for (int64_t r = g; r < M; r += 16) {
                const float d = Z[(size_t)r * C + c] - mean;
                q = fmaf(d, d, q);
            }
        var = __fdiv_rn(col_sum16(q, red), n);
    } else {
        mean = rm[cc];
        var = rv[cc];
    }
    if (live && g == 0) {
        if (batch) {
            const float n = (float)M;
            rm[c] = (1.f - momentum) * rm[c] + momentum * mean;
            rv[c] = (1.f - momentum) * rv[c] + momentum * (var * (n / (n - 1.f)));
        }
        const float rstd = __fdiv_rn(1.f, __fsqrt_rn(var + eps));
        const float sc = __fmul_rn(gamma[c], rstd);
        mean_out[c] = mean;
        rstd_out[c] = rstd;
        scale_out[c] = sc;
        shift_out[c] = __fsub_rn(beta[c], __fmul_rn(mean, sc));
    }
}

// y = Z scale + shift (+ Res): what the forward stores and the backward's ReLU mask tests.
__device__ __forceinline__ float bn_act_y(float z, float sc, float sh, const float* Res, size_t i) {
    const float y = fmaf(z, sc, sh);
    return Res ? __fadd_rn(y, Res[i]) : y;
}

__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const float* __restrict__ Z, int64_t total4, int C,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const float* __restrict__ Res, bool relu, float* __restrict__ Y) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total4; q += (int64_t)gridDim.x * 256) {
        const int c = (int)((4 * q) % C);
        const float4 z = *(const float4*)(Z + 4 * (size_t)q);
        const float4 sc = *(const float4*)(scale + c), sh = *(const float4*)(shift + c);
        float4 y;
        y.x = bn_act_y(z.x, sc.x, sh.x, Res, 4 * (size_t)q + 0);
        y.y = bn_act_y(z.y, sc.y, sh.y, Res, 4 * (size_t)q + 1);
        y.z = bn_act_y(z.z, sc.z, sh.z, Res, 4 * (size_t)q + 2);
        y.w = bn_act_y(z.w, sc.w, sh.w, Res, 4 * (size_t)q + 3);
        if (relu) {
            y.x = y.x > 0.f ? y.x : 0.f;
            y.y = y.y > 0.f ? y.y : 0.f;
            y.z = y.z > 0.f ? y.z : 0.f;
            y.w = y.w > 0.f ? y.w : 0.f;
        }
        *(float4*)(Y + 4 * (size_t)q) = y;
    }
}

// Per channel c of dY / Z [M][C] (bn2d_stats_kernel's geometry, head_train.hip's bn2_bwd_kernel plus the ReLU mask and
// the residual): dgamma, dbeta, then dZ and dRes.  dZ may be dY: every element is read, then written, by one thread.
__global__ __launch_bounds__(256) void bn_act_bwd_kernel(const float* dY, const float* __restrict__ Z, int64_t M, int C,
                                                         bool batch, bool relu, const float* __restrict__ gamma,
                                                         const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const float* __restrict__ Res, float* dZ, float* __restrict__ dRes,
                                                         float* __restrict__ dg, float* __restrict__ db) {
    __shared__ float red[16 * 17];
    const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool live = c < C;
    const int cc = live ? c : C - 1;
    const float mean = mean_in[cc], rstd = rstd_in[cc], sc = scale[cc], sh = shift[cc], gr = gamma[cc] * rstd;
    auto dh_at = [&](size_t i) {
        const float d = dY[i];
        return !relu || bn_act_y(Z[i], sc, sh, Res, i) > 0.f ? d : 0.f;
    };
    float s0 = 0.f, s1 = 0.f;
    if (live)
        for (int64_t r = g; r < M; r += 16) {
            const size_t i = (size_t)r * C + c;
            const float d = dh_at(i);
            s0 += d;
            s1 = fmaf(d, xhat(Z[i], mean, rstd), s1);
        }
    const float dbeta = col_sum16(s0, red);
    const float dgamma = col_sum16(s1, red);
    if (live && g == 0) {
        if (db) db[c] = dbeta;
        if (dg) dg[c] = dgamma;
    }
    if (!dZ && !dRes) return;
    const float inv_n = __fdiv_rn(1.f, (float)M);
    const float mb = dbeta * inv_n, mg = dgamma * inv_n;
    if (live)
        for (int64_t r = g; r < M; r += 16) {
            const size_t i = (size_t)r * C + c;
            const float d = dh_at(i);
            if (dRes) dRes[i] = d;
            if (dZ) dZ[i] = batch ? gr * ((d - mb) - xhat(Z[i], mean, rstd) * mg) : d * sc;
        }
}

unsigned stride_grid(int64_t quads) { return (unsigned)std::min<int64_t>((quads + 255) / 256, 1 << 20); }

}  // namespace

// K splits of the forward product, whole 64-float chunks each, a function of the shape alone: about two workgroups
// per CU over the (pixel tile, channel tile, split) grid and at most 64 splits (head_train_plan's rule).
void conv_train_plan(int64_t M, int K, int N, int* n_split, int* k_per_split) {
    const int64_t tiles = ((M + MT - 1) / MT) * ((N + MT - 1) / MT);
    const int chunks = (K + KC - 1) / KC;
    const int want = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(chunks, 64), 512 / tiles));
    const int cps = (chunks + want - 1) / want;
    *k_per_split = cps * KC;
    *n_split = (chunks + cps - 1) / cps;
}

// forward: partials [split][M][Cout] when the plan splits K, else nothing (16 bytes, so that 0 stays the error value)
size_t conv_train_workspace(const ConvTrainArgs& a) {
    int ns, kps;
    const int64_t M = (int64_t)a.B * a.OH * a.OW;
    conv_train_plan(M, a.k * a.k * a.Cin, a.Cout, &ns, &kps);
    return ns > 1 ? (size_t)ns * M * a.Cout * sizeof(float) : 16;
}

hipError_t launch_conv_train_forward(const ConvTrainArgs& a, float* Z, void* ws, hipStream_t s) {
    int ns, kps;
    const int64_t M = (int64_t)a.B * a.OH * a.OW;
    conv_train_plan(M, a.k * a.k * a.Cin, a.Cout, &ns, &kps);
    const dim3 grid((unsigned)((M + MT - 1) / MT), (a.Cout + MT - 1) / MT, ns);
    hipLaunchKernelGGL(conv_fwd_kernel, grid, dim3(256), 0, s, a, kps, ns > 1 ? (float*)ws : Z);
    if (ns > 1) {
        const int64_t quads = M * a.Cout / 4;
        hipLaunchKernelGGL(conv_merge_kernel, dim3(stride_grid(quads)), dim3(256), 0, s, (const float*)ws, ns, quads, Z);
    }
    return hipGetLastError();
}

hipError_t launch_conv_train_backward(const ConvTrainArgs& a, const float* dZ, float* dA, float* dW, hipStream_t s) {
    if (dW)
        hipLaunchKernelGGL(conv_bwd_kernel<true>, dim3((a.Cout + MT - 1) / MT, (a.k * a.k * a.Cin + MT - 1) / MT), dim3(256),
                           0, s, a, dZ, dW);
    if (dA) {
        const int64_t rows = (int64_t)a.B * a.H * a.W;
        hipLaunchKernelGGL(conv_bwd_kernel<false>, dim3((unsigned)((rows + MT - 1) / MT), (a.Cin + MT - 1) / MT), dim3(256),
                           0, s, a, dZ, dA);
    }
    return hipGetLastError();
}

hipError_t launch_bn2d_train_stats(const float* Z, int64_t M, int C, const float* gamma, const float* beta, float* rm,
                                   float* rv, bool batch, float eps, float momentum, float* mean, float* rstd, float* scale,
                                   float* shift, hipStream_t s) {
    hipLaunchKernelGGL(bn2d_stats_kernel, dim3((C + 15) / 16), dim3(256), 0, s, Z, M, C, gamma, beta, rm, rv, batch, eps,
                       momentum, mean, rstd, scale, shift);
    return hipGetLastError();
}

hipError_t launch_bn_act_forward(const float* Z, int64_t M, int C, const float* scale, const float* shift, const float* Res,
                                 bool relu, float* Y, hipStream_t s) {
    const int64_t quads = M * C / 4;
    hipLaunchKernelGGL(bn_act_fwd_kernel, dim3(stride_grid(quads)), dim3(256), 0, s, Z, quads, C, scale, shift, Res, relu, Y);
    return hipGetLastError();
}

hipError_t launch_bn_act_backward(const float* dY, const float* Z, int64_t M, int C, bool batch, bool relu,
                                  const float* gamma, const float* mean, const float* rstd, const float* scale,
                                  const float* shift, const float* Res, float* dZ, float* dRes, float* dgamma, float* dbeta,
                                  hipStream_t s) {
    hipLaunchKernelGGL(bn_act_bwd_kernel, dim3((C + 15) / 16), dim3(256), 0, s, dY, Z, M, C, batch, relu, gamma, mean, rstd,
                       scale, shift, Res, dZ, dRes, dgamma, dbeta);
    return hipGetLastError();
}

}  // namespace fr
