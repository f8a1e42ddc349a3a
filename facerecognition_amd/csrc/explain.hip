// Class-activation maps on the device (gfx950): the reference's Grad-CAM (inference/explainability.py:76-131,
// GradCAM.generate) and its FaceNet activation map (:482-501) without a backward pass.  In eval mode everything
// after the explained tensor is affine and already folded into the head matrix (weights.fold_state_dict head.w), so
// d score / d head-input = head.w^T . g with g = d score / d embedding in closed form:
//  * score_grad    g [B][N] from the raw embedding e and an optional target t:
//                  g = 2 e ((e ** 2).sum()), or t / (|e||t|) - (e.t) e / (|e|^3 |t|) (F.cosine_similarity, norms
//                  clamped at 1e-8)
//  * head_grad     V [B][Kpad] = G [B][N] . W [N][Kpad], one pass over the 16-bit weight image per tile of 8 images
//  * cam           one workgroup per image: channel weights (mean gradient over positions), the weighted channel sum
//                  per position, ReLU, torch's align_corners=False bilinear upsample, min / max normalisation
#include "kernels.h"

#include "../../include/frhip.h"

namespace fr {
namespace {

constexpr int HG_BT = 8;        // images per head_grad workgroup (the weight image is read once per tile)
constexpr int HG_WAVES = 8;     // waves of a workgroup: each sums its own eighth of the n rows
constexpr int HG_KB = 512;      // K columns per workgroup: 64 lanes x 8 consecutive columns (one 16-B load per row)
constexpr int HG_NMAX = 1024;   // G tile [HG_BT][N] in LDS

// One workgroup per image.
__global__ __launch_bounds__(256) void score_grad_kernel(const float* __restrict__ emb, const float* __restrict__ target,
                                                         int N, float* __restrict__ g) {
    __shared__ float red[4];
    const float* e = emb + (size_t)blockIdx.x * N;
    float* out = g + (size_t)blockIdx.x * N;
    if (!target) {
        for (int n = threadIdx.x; n < N; n += 256) out[n] = 2.0f * e[n];
        return;
    }
    const float* t = target + (size_t)blockIdx.x * N;
    float ee = 0.f, tt = 0.f, et = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float a = e[n], b = t[n];
        ee += a * a;
        tt += b * b;
        et += a * b;
    }
    ee = block_sum_256(ee, red);
    tt = block_sum_256(tt, red);
    et = block_sum_256(et, red);
    const float ne = fmaxf(sqrtf(ee), 1e-8f), nt = fmaxf(sqrtf(tt), 1e-8f);
    const float ca = 1.0f / (ne * nt), cb = et / (ne * ne * ne * nt);
    for (int n = threadIdx.x; n < N; n += 256) out[n] = t[n] * ca - e[n] * cb;
}

// Grid (ceil(K / 512), ceil(B / 8)), 512 threads.  A lane owns 8 consecutive K columns; wave u sums rows
// [u * ceil(N / 8), ...) in ascending order for the tile's 8 images (g from LDS, a broadcast read), then the 8 wave
// partials of a column are added in wave order: the order of the sum over n depends on N alone, not on B.
template <bool F16>
__global__ __launch_bounds__(HG_WAVES * 64) void head_grad_kernel(const float* __restrict__ g, int B, int N,
                                                                   const bf16_t* __restrict__ w, int K, int Kpad,
                                                                   float* __restrict__ v) {
    __shared__ float gs[HG_BT][HG_NMAX];
    __shared__ float red[HG_WAVES][HG_KB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.y * HG_BT;
    for (int i = tid; i < HG_BT * N; i += HG_WAVES * 64) {
        const int b = i / N, n = i - b * N;
        gs[b][n] = b0 + b < B ? g[(size_t)(b0 + b) * N + n] : 0.f;
    }
    __syncthreads();
    const int k0 = blockIdx.x * HG_KB + lane * 8;
    const bool own = k0 < K;  // K % 8 == 0: a lane's 8 columns are all inside or all outside
    const int chunk = (N + HG_WAVES - 1) / HG_WAVES;
    const int n0 = min(N, wave * chunk), n1 = min(N, n0 + chunk);
    float acc[HG_BT][8];
#pragma unroll
    for (int b = 0; b < HG_BT; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[b][j] = 0.f;
    if (own) {
        const bf16_t* wp = w + k0;
        int n = n0;
        for (; n + 4 <= n1; n += 4) {  // four rows' loads in flight
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = *(const uint4*)(wp + (size_t)(n + u) * Kpad);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float f[8];
                Num<F16>::unpack8(q[u], f);
#pragma unroll
                for (int b = 0; b < HG_BT; ++b) {
                    const float gv = gs[b][n + u];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[b][j] = fmaf(gv, f[j], acc[b][j]);
                }
            }
        }
        for (; n < n1; ++n) {
            float f[8];
            Num<F16>::unpack8(*(const uint4*)(wp + (size_t)n * Kpad), f);
#pragma unroll
            for (int b = 0; b < HG_BT; ++b) {
                const float gv = gs[b][n];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[b][j] = fmaf(gv, f[j], acc[b][j]);
            }
        }
    }
    const int kc = blockIdx.x * HG_KB + tid;  // the column this thread sums and stores (tid < 512)
#pragma unroll
    for (int b = 0; b < HG_BT; ++b) {
        if (b0 + b >= B) break;  // uniform over the workgroup
        *(float4*)&red[wave][lane * 8] = make_float4(acc[b][0], acc[b][1], acc[b][2], acc[b][3]);
        *(float4*)&red[wave][lane * 8 + 4] = make_float4(acc[b][4], acc[b][5], acc[b][6], acc[b][7]);
        __syncthreads();
        float s = red[0][tid];
#pragma unroll
        for (int u = 1; u < HG_WAVES; ++u) s += red[u][tid];
        if (kc < K) v[(size_t)(b0 + b) * Kpad + kc] = s;  // columns [K, Kpad) are never written
        __syncthreads();
    }
}

constexpr int CAM_CMAX = 4096;  // channel weights in LDS
constexpr int CAM_PMAX = 256;   // positions of the explained tensor

// torch's area_pixel_compute_source_index (align_corners = False, no scale factor given): src = max(0, (dst + 0.5) *
// in / out - 0.5), upper neighbour clamped to in - 1.  Evaluated as one rounded quotient of exact integers,
// ((2 dst + 1) in - out) / (2 out) (both below 2^24), so the weight is within half an ulp of the exact one (torch's
// f32 form rounds the scale, the product and the difference).
__device__ __forceinline__ void bilin_src(int dst, int in, int out, int* i0, int* i1, float* l1) {
    const float src = fmaxf((float)((2 * dst + 1) * in - out) / (float)(2 * out), 0.f);
    const int a = min((int)src, in - 1);
    *i0 = a;
    *i1 = a + (a < in - 1 ? 1 : 0);
    *l1 = src - (float)a;
}

// One workgroup (4 waves) per image.  LAYOUT 0: v [B][vs] holds the gradient of the pooled head input, every
// position's gradient is v / (h w); 1: v [B][vs] is the gradient of the flattened NHWC tensor; 2: no gradient,
// low[p] = sum_c |A[p][c]| (the FaceNet activation map), no ReLU, zeros for a constant map.
template <bool F16, int LAYOUT>
__global__ __launch_bounds__(256) void cam_kernel(const bf16_t* __restrict__ act, int h, int w, int C,
                                                  const float* __restrict__ v, int vs, int S, float* __restrict__ cam,
                                                  float* __restrict__ low) {
    __shared__ float wgt[LAYOUT == 2 ? 1 : CAM_CMAX];
    __shared__ float lo[CAM_PMAX];
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, P = h * w;
    const bf16_t* A = act + (size_t)b * P * C;
    if (LAYOUT != 2) {
        const float* vb = v + (size_t)b * vs;
        const float np = (float)P;
        for (int c = tid; c < C; c += 256) {
            float s;
            if (LAYOUT == 0) {
                s = vb[c] / np;  // the mean over positions of P equal values v / P
            } else {
                s = 0.f;
                for (int p = 0; p < P; ++p) s += vb[(size_t)p * C + c];
                s = s / np;
            }
            wgt[c] = s;
        }
        __syncthreads();
    }
    for (int p = wave; p < P; p += 4) {
        const bf16_t* ap = A + (size_t)p * C;
        float s = 0.f;
        for (int c = lane * 8; c < C; c += 512) {
            float f[8];
            Num<F16>::unpack8(*(const uint4*)(ap + c), f);
            if constexpr (LAYOUT == 2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) s += fabsf(f[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) s = fmaf(wgt[c + j], f[j], s);
            }
        }
        s = wave_sum(s);
        if (lane == 0) {
            if (low) low[(size_t)b * P + p] = s;  // the map before ReLU
            lo[p] = LAYOUT == 2 ? s : fmaxf(s, 0.f);
        }
    }
    __syncthreads();
    float* out = cam + (size_t)b * S * S;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < S * S; i += 256) {
        const int oy = i / S, ox = i - oy * S;
        int y0, y1, x0, x1;
        float ly, lx;
        bilin_src(oy, h, S, &y0, &y1, &ly);
        bilin_src(ox, w, S, &x0, &x1, &lx);
        // a + l (b - a): a constant map stays that constant exactly, so it is stored unnormalised (max == min)
        const float top = lo[y0 * w + x0] + lx * (lo[y0 * w + x1] - lo[y0 * w + x0]);
        const float bot = lo[y1 * w + x0] + lx * (lo[y1 * w + x1] - lo[y1 * w + x0]);
        const float c = top + ly * (bot - top);
        out[i] = c;  // read back by this thread below
        mn = fminf(mn, c);
        mx = fmaxf(mx, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if (lane == 0) { red[wave] = mn; red[4 + wave] = mx; }
    __syncthreads();
    mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    if (mx > mn) {
        const float d = mx - mn;
        for (int i = tid; i < S * S; i += 256) out[i] = (out[i] - mn) / d;
    } else if (LAYOUT == 2) {
        for (int i = tid; i < S * S; i += 256) out[i] = 0.f;
    }
}

}  // namespace

hipError_t launch_score_grad(const float* emb, const float* target, int B, int N, float* g, hipStream_t s) {
    score_grad_kernel<<<B, 256, 0, s>>>(emb, target, N, g);
    return hipGetLastError();
}

bool head_grad_supported(int B, int N, int K, int Kpad) {
    return B > 0 && N > 0 && N <= HG_NMAX && K > 0 && K % 8 == 0 && Kpad % 8 == 0 && Kpad >= K &&
           (B + HG_BT - 1) / HG_BT <= 65535;
}

hipError_t launch_head_grad(const float* g, int B, int N, const bf16_t* w, int K, int Kpad, int f16, float* v,
                            hipStream_t s) {
    if (!head_grad_supported(B, N, K, Kpad)) return hipErrorInvalidValue;
    const dim3 grid((K + HG_KB - 1) / HG_KB, (B + HG_BT - 1) / HG_BT);
    if (f16) head_grad_kernel<true><<<grid, HG_WAVES * 64, 0, s>>>(g, B, N, w, K, Kpad, v);
    else head_grad_kernel<false><<<grid, HG_WAVES * 64, 0, s>>>(g, B, N, w, K, Kpad, v);
    return hipGetLastError();
}

bool cam_supported(int B, int h, int w, int C, int S) {
    return B > 0 && h > 0 && w > 0 && h * w <= CAM_PMAX && C > 0 && C % 8 == 0 && C <= CAM_CMAX && S > 0 && S <= 4096;
}

hipError_t launch_cam(const bf16_t* act, int B, int h, int w, int C, int f16, const float* v, int v_stride, int layout,
                      int S, float* cam, float* low, hipStream_t s) {
    if (!cam_supported(B, h, w, C, S) || layout < 0 || layout > 2 || (layout != 2 && !v)) return hipErrorInvalidValue;
#define FR_CAM(F, L) cam_kernel<F, L><<<B, 256, 0, s>>>(act, h, w, C, v, v_stride, S, cam, low)
    if (f16) {
        if (layout == 0) FR_CAM(true, 0);
        else if (layout == 1) FR_CAM(true, 1);
        else FR_CAM(true, 2);
    } else {
        if (layout == 0) FR_CAM(false, 0);
        else if (layout == 1) FR_CAM(false, 1);
        else FR_CAM(false, 2);
    }
#undef FR_CAM
    return hipGetLastError();
}

}  // namespace fr
