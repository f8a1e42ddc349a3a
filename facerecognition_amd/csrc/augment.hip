// Training augmentations on the device (DESIGN.md §4 "Augmentation"; include/frhip.h "Augmentation"): an interpreter over
// a short per-image op list, one workgroup per image, the image resident in LDS.
//   LDS: two u8 image buffers of H W 3 bytes (ping-pong: geometric ops and the blur gather from one into the other,
//   colour ops run in place), then the resampler's per-image coefficient tables, 16 (W + H) bytes.  The input is read
//   from global memory once, the outputs are written once.  Opcode and arguments are the same for every thread of the
//   workgroup, so the dispatch is scalar; a barrier separates ops.
//   Definitions (Pillow's libImaging unless stated, restated in tests/augment_ref.py and checked against Pillow there):
//     FLIP_H                transpose(FLIP_LEFT_RIGHT)
//     AFFINE_NEAREST        Geometry.c affine_fixed: 16.16 fixed point, source (a2 + a1 y + a0 x) >> 16, fill 0
//     PERSPECTIVE_BILINEAR  perspective_transform + bilinear_filter32RGB in double, truncating store, fill 0
//     CROP_RESIZE           Resample.c: triangle filter, 22-bit coefficients, horizontal pass then vertical pass
//     BRIGHTNESS / CONTRAST / SATURATION   ImageEnhance: Blend.c against black / the rounded mean of L / L
//     HUE                   torchvision's PIL adjust_hue: Convert.c rgb2hsv, u8 wrap of H, hsv2rgb
//     GRAYSCALE             convert("L") in 3 channels
//     GAUSS_BLUR            torchvision's tensor blur: f32 taps w[dy] w[dx], reflect padding, f32 sum in row-major tap
//                           order from 0, rintf, clamp to a byte
//     ERASE                 RandomErasing(value=0) of the normalised f32 output
//   This file is built with -ffp-contract=off: every product is rounded, as on the host Pillow runs on.
//   No atomics, no randomness: the result is a pure function of (input, op list).
//   Bounds: the boxes of CROP_RESIZE and ERASE, k, the opcodes and finiteness are validated by augment_api.cpp; source
//   coordinates of the geometric ops are range-checked per pixel here, taps of the resampler are clamped to its input,
//   so no argument value makes the kernel touch anything outside its image.
#include "../../include/frhip.h"
#include "kernels.h"

namespace fr {
namespace {

constexpr int AUG_THREADS = 1024;

struct AugParams {
    const uint8_t* in;
    const int32_t* ops;   // [B][n_ops]
    const double* args;   // [B][n_ops][8]
    const float* norm;    // [256]
    float* out_f32;       // [B][3][H][W] or null
    uint8_t* out_u8;      // [B][H][W][3] or null
    int H, W, n_ops;
};

__device__ __forceinline__ int align16(int v) { return (v + 15) & ~15; }

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Blend.c: deg + alpha (src - deg) in float; truncation inside [0, 1], clipping outside
__device__ __forceinline__ uint8_t blend(int deg, int src, float f, bool inside) {
    const float t = (float)deg + f * (float)(src - deg);
    if (inside) return (uint8_t)(int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (uint8_t)(int)t);
}

// one axis of Pillow's precompute_coeffs + normalize_coeffs_8bpc for BILINEAR over [0, in_size], in_size <= out_size
// (support 1, at most 3 taps): e = {first source index, number of taps, k0, k1, k2}, packed in 4 ints
__device__ void resample_entry(int xx, int in_size, int out_size, int32_t* e) {
    const double scale = (double)in_size / out_size;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - 1.0 + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + 1.0 + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > 3) xmax = 3;  // cannot happen with support 1; keeps the table and the reads in bounds
    if (xmax < 0) xmax = 0;
    double k[3] = {0.0, 0.0, 0.0};
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double t = (x + xmin - center + 0.5) * 1.0;
        if (t < 0.0) t = -t;
        const double w = t < 1.0 ? 1.0 - t : 0.0;
        k[x] = w;
        ww += w;
    }
    for (int x = 0; x < 3; ++x) {
        double v = k[x];
        if (x < xmax && ww != 0.0) v /= ww;
        e[1 + x] = (int32_t)(0.5 + v * (double)(1 << PB));
    }
    e[0] = xmin | (xmax << 24);
}

// Convert.c rgb2hsv / hsv2rgb with the hue byte moved by shift (u8 wrap)
__device__ __forceinline__ void hue_pixel(uint8_t* px, int shift) {
    const int r = px[0], g = px[1], b = px[2];
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double x = (double)h / 6.0 + 1.0;  // in [0.5, 2): fmod(x, 1.0) is x or x - 1, exactly
        h = (float)(x >= 1.0 ? x - 1.0 : x);
        uh = (int)((double)h * 255.0);
        us = (int)((double)s * 255.0);
        uh = uh < 0 ? 0 : (uh > 255 ? 255 : uh);
        us = us < 0 ? 0 : (us > 255 ? 255 : us);
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        px[0] = px[1] = px[2] = (uint8_t)uv;
        return;
    }
    const float fh = (float)((double)uh * 6.0 / 255.0);
    const float fi = floorf(fh);
    const float f = fh - fi;
    const float fs = (float)((double)us / 255.0);
    const float vf = (float)uv;
    // C round() of a non-negative value: half away from zero
    const float xp = vf * (1.f - fs), xq = vf * (1.f - fs * f), xt = vf * (1.f - fs * (1.f - f));
    float fp = floorf(xp), fq = floorf(xq), ft = floorf(xt);
    if (xp - fp >= 0.5f) fp += 1.f;
    if (xq - fq >= 0.5f) fq += 1.f;
    if (xt - ft >= 0.5f) ft += 1.f;
    const int p = min(max((int)fp, 0), 255), q = min(max((int)fq, 0), 255), t = min(max((int)ft, 0), 255);
    int R, G, B;
    switch ((int)fi % 6) {
        case 0: R = uv; G = t; B = p; break;
        case 1: R = q; G = uv; B = p; break;
        case 2: R = p; G = uv; B = t; break;
        case 3: R = p; G = q; B = uv; break;
        case 4: R = t; G = p; B = uv; break;
        default: R = uv; G = p; B = q; break;
    }
    px[0] = (uint8_t)R;
    px[1] = (uint8_t)G;
    px[2] = (uint8_t)B;
}

__device__ __forceinline__ int reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);  // the API keeps k / 2 < n, so the clamp never acts
}

__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(AugParams p) {
    extern __shared__ __align__(16) uint8_t lds[];
    __shared__ float s_norm[256];
    __shared__ int s_red[AUG_THREADS / 64];
    const int tid = threadIdx.x;
    const int H = p.H, W = p.W, npx = H * W, nby = npx * 3;
    const size_t b = blockIdx.x;
    uint8_t* cur = lds;
    uint8_t* alt = lds + align16(nby);
    int32_t* tab = (int32_t*)(lds + 2 * align16(nby));  // [W + H][4]

    const uint8_t* g = p.in + b * (size_t)nby;
    if ((nby & 3) == 0 && (((uintptr_t)g) & 3) == 0) {
        for (int i = tid; i < nby / 4; i += AUG_THREADS) ((uint32_t*)cur)[i] = ((const uint32_t*)g)[i];
    } else {
        for (int i = tid; i < nby; i += AUG_THREADS) cur[i] = g[i];
    }
    if (tid < 256) s_norm[tid] = p.norm[tid];
    __syncthreads();

    int er_i = 0, er_j = 0, er_h = 0, er_w = 0;
    for (int k = 0; k < p.n_ops; ++k) {
        const int op = __builtin_amdgcn_readfirstlane(p.ops[b * p.n_ops + k]);
        const double* a = p.args + (b * p.n_ops + k) * FR_AUGMENT_ARGS;
        switch (op) {
            case FR_AUG_FLIP_H: {
                for (int i = tid; i < npx; i += AUG_THREADS) {
                    const int y = i / W, x = i - y * W;
                    const uint8_t* s = cur + i * 3;
                    uint8_t* d = alt + (y * W + (W - 1 - x)) * 3;
                    d[0] = s[0];
                    d[1] = s[1];
                    d[2] = s[2];
                }
                uint8_t* t = cur; cur = alt; alt = t;
                break;
            }
            case FR_AUG_AFFINE_NEAREST: {
                // FIX(v) = floor(v 65536 + 0.5); the API keeps every corner inside +-32768, so the int casts are exact
                const uint32_t a0 = (uint32_t)(int)floor(a[0] * 65536.0 + 0.5), a1 = (uint32_t)(int)floor(a[1] * 65536.0 + 0.5);
                const uint32_t a3 = (uint32_t)(int)floor(a[3] * 65536.0 + 0.5), a4 = (uint32_t)(int)floor(a[4] * 65536.0 + 0.5);
                const uint32_t a2 = (uint32_t)(int)floor((a[2] + a[0] * 0.5 + a[1] * 0.5) * 65536.0 + 0.5);
                const uint32_t a5 = (uint32_t)(int)floor((a[5] + a[3] * 0.5 + a[4] * 0.5) * 65536.0 + 0.5);
                for (int i = tid; i < npx; i += AUG_THREADS) {
                    const int y = i / W, x = i - y * W;
                    const int sx = (int)(a2 + a1 * (uint32_t)y + a0 * (uint32_t)x) >> 16;  // wraps like Pillow's int walk
                    const int sy = (int)(a5 + a4 * (uint32_t)y + a3 * (uint32_t)x) >> 16;
                    uint8_t* d = alt + i * 3;
                    if (sx >= 0 && sx < W && sy >= 0 && sy < H) {
                        const uint8_t* s = cur + (sy * W + sx) * 3;
                        d[0] = s[0];
                        d[1] = s[1];
                        d[2] = s[2];
                    } else {
                        d[0] = d[1] = d[2] = 0;
                    }
                }
                uint8_t* t = cur; cur = alt; alt = t;
                break;
            }
            case FR_AUG_PERSPECTIVE_BILINEAR: {
                const double c0 = a[0], c1 = a[1], c2 = a[2], c3 = a[3], c4 = a[4], c5 = a[5], c6 = a[6], c7 = a[7];
                for (int i = tid; i < npx; i += AUG_THREADS) {
                    const int y = i / W, x = i - y * W;
                    const double xi = x + 0.5, yi = y + 0.5;
                    const double den = c6 * xi + c7 * yi + 1;
                    double xin = (c0 * xi + c1 * yi + c2) / den;
                    double yin = (c3 * xi + c4 * yi + c5) / den;
                    uint8_t* d = alt + i * 3;
                    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {  // a NaN is outside
                        d[0] = d[1] = d[2] = 0;
                        continue;
                    }
                    xin -= 0.5;
                    yin -= 0.5;
                    const double fx = floor(xin), fy = floor(yin);
                    const double dx = xin - fx, dy = yin - fy;
                    const int ix = (int)fx, iy = (int)fy;  // in [-1, W) and [-1, H)
                    const int x0 = min(max(ix, 0), W - 1), x1 = min(max(ix + 1, 0), W - 1);
                    const int y0 = min(max(iy, 0), H - 1);
                    const bool has = iy + 1 >= 0 && iy + 1 < H;
                    const uint8_t* r0 = cur + y0 * W * 3;
                    const uint8_t* r1 = cur + (has ? iy + 1 : y0) * W * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double p0 = r0[x0 * 3 + c], q0 = r0[x1 * 3 + c];
                        const double v1 = p0 + (q0 - p0) * dx;
                        double v2 = v1;
                        if (has) {
                            const double p1 = r1[x0 * 3 + c], q1 = r1[x1 * 3 + c];
                            v2 = p1 + (q1 - p1) * dx;
                        }
                        d[c] = (uint8_t)(int)(v1 + (v2 - v1) * dy);
                    }
                }
                uint8_t* t = cur; cur = alt; alt = t;
                break;
            }
            case FR_AUG_CROP_RESIZE: {
                const int ci = (int)a[0], cj = (int)a[1], ch = (int)a[2], cw = (int)a[3];  // validated: inside the image
                const bool horiz = cw != W, vert = ch != H;
                if (!horiz && !vert) break;
                for (int t = tid; t < W + H; t += AUG_THREADS) {
                    if (t < W) resample_entry(t, cw, W, tab + 4 * t);
                    else resample_entry(t - W, ch, H, tab + 4 * t);
                }
                __syncthreads();
                const uint8_t* vsrc = cur + ci * W * 3;  // rows of the crop when there is no horizontal pass (cj = 0)
                if (horiz) {  // alt [ch][W] from cur rows ci .., columns cj ..
                    for (int i = tid; i < ch * W; i += AUG_THREADS) {
                        const int r = i / W, x = i - r * W;
                        const int32_t* e = tab + 4 * x;
                        const int xmin = e[0] & 0xffffff, xn = e[0] >> 24;
                        const uint8_t* s = cur + ((ci + r) * W + cj + xmin) * 3;
                        int s0 = 1 << (PB - 1), s1 = s0, s2 = s0;
                        for (int t = 0; t < xn; ++t) {
                            const int w = e[1 + t];
                            s0 += s[3 * t] * w;
                            s1 += s[3 * t + 1] * w;
                            s2 += s[3 * t + 2] * w;
                        }
                        uint8_t* d = alt + i * 3;
                        d[0] = clip8(s0);
                        d[1] = clip8(s1);
                        d[2] = clip8(s2);
                    }
                    __syncthreads();
                    uint8_t* t = cur; cur = alt; alt = t;
                    vsrc = cur;
                }
                if (vert) {
                    for (int i = tid; i < npx; i += AUG_THREADS) {
                        const int y = i / W, x = i - y * W;
                        const int32_t* e = tab + 4 * (W + y);
                        const int ymin = e[0] & 0xffffff, yn = e[0] >> 24;
                        const uint8_t* s = vsrc + (ymin * W + x) * 3;
                        int s0 = 1 << (PB - 1), s1 = s0, s2 = s0;
                        for (int t = 0; t < yn; ++t) {
                            const int w = e[1 + t];
                            s0 += s[t * W * 3] * w;
                            s1 += s[t * W * 3 + 1] * w;
                            s2 += s[t * W * 3 + 2] * w;
                        }
                        uint8_t* d = alt + i * 3;
                        d[0] = clip8(s0);
                        d[1] = clip8(s1);
                        d[2] = clip8(s2);
                    }
                    uint8_t* t = cur; cur = alt; alt = t;
                }
                break;
            }
            case FR_AUG_BRIGHTNESS: {
                const float f = (float)a[0];
                const bool inside = f >= 0.f && f <= 1.f;
                for (int i = tid; i < nby; i += AUG_THREADS) cur[i] = blend(0, cur[i], f, inside);
                break;
            }
            case FR_AUG_CONTRAST: {
                const float f = (float)a[0];
                const bool inside = f >= 0.f && f <= 1.f;
                int part = 0;
                for (int i = tid; i < npx; i += AUG_THREADS) part += luma(cur[i * 3], cur[i * 3 + 1], cur[i * 3 + 2]);
                for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
                if ((tid & 63) == 0) s_red[tid >> 6] = part;
                __syncthreads();
                long long sum = 0;
                for (int w = 0; w < AUG_THREADS / 64; ++w) sum += s_red[w];
                const int mean = (int)((2 * sum + npx) / (2 * (long long)npx));  // int(mean(L) + 0.5)
                for (int i = tid; i < nby; i += AUG_THREADS) cur[i] = blend(mean, cur[i], f, inside);
                break;
            }
            case FR_AUG_SATURATION: {
                const float f = (float)a[0];
                const bool inside = f >= 0.f && f <= 1.f;
                for (int i = tid; i < npx; i += AUG_THREADS) {
                    uint8_t* px = cur + i * 3;
                    const int r = px[0], g2 = px[1], b2 = px[2];
                    const int L = luma(r, g2, b2);
                    px[0] = blend(L, r, f, inside);
                    px[1] = blend(L, g2, f, inside);
                    px[2] = blend(L, b2, f, inside);
                }
                break;
            }
            case FR_AUG_HUE: {
                const int shift = (int)(a[0] * 255.0) & 255;  // numpy's uint8(f 255): truncate, then wrap
                for (int i = tid; i < npx; i += AUG_THREADS) hue_pixel(cur + i * 3, shift);
                break;
            }
            case FR_AUG_GRAYSCALE: {
                for (int i = tid; i < npx; i += AUG_THREADS) {
                    uint8_t* px = cur + i * 3;
                    px[0] = px[1] = px[2] = (uint8_t)luma(px[0], px[1], px[2]);
                }
                break;
            }
            case FR_AUG_GAUSS_BLUR: {
                const int kk = (int)a[0];  // validated: 3, 5 or 7 and kk / 2 < min(H, W)
                const int r = kk >> 1;
                for (int i = tid; i < npx; i += AUG_THREADS) {
                    const int y = i / W, x = i - y * W;
                    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
                    for (int dy = 0; dy < kk; ++dy) {
                        const uint8_t* row = cur + reflect(y + dy - r, H) * W * 3;
                        const float wy = (float)a[1 + dy];  // uniform: scalar loads
                        for (int dx = 0; dx < kk; ++dx) {
                            const uint8_t* s = row + reflect(x + dx - r, W) * 3;
                            const float w2 = wy * (float)a[1 + dx];
                            acc0 = acc0 + w2 * (float)s[0];
                            acc1 = acc1 + w2 * (float)s[1];
                            acc2 = acc2 + w2 * (float)s[2];
                        }
                    }
                    uint8_t* d = alt + i * 3;
                    d[0] = (uint8_t)(int)fminf(fmaxf(rintf(acc0), 0.f), 255.f);
                    d[1] = (uint8_t)(int)fminf(fmaxf(rintf(acc1), 0.f), 255.f);
                    d[2] = (uint8_t)(int)fminf(fmaxf(rintf(acc2), 0.f), 255.f);
                }
                uint8_t* t = cur; cur = alt; alt = t;
                break;
            }
            case FR_AUG_ERASE:
                er_i = (int)a[0];
                er_j = (int)a[1];
                er_h = (int)a[2];
                er_w = (int)a[3];
                break;
            default:  // FR_AUG_NOP
                break;
        }
        __syncthreads();
    }

    if (p.out_u8) {
        uint8_t* o = p.out_u8 + b * (size_t)nby;
        if ((nby & 3) == 0 && (((uintptr_t)o) & 3) == 0 && (((uintptr_t)cur) & 3) == 0) {
            for (int i = tid; i < nby / 4; i += AUG_THREADS) ((uint32_t*)o)[i] = ((const uint32_t*)cur)[i];
        } else {
            for (int i = tid; i < nby; i += AUG_THREADS) o[i] = cur[i];
        }
    }
    if (p.out_f32) {
        float* o = p.out_f32 + b * (size_t)nby;
        for (int i = tid; i < nby; i += AUG_THREADS) {
            const int c = i / npx, px = i - c * npx;
            const int y = px / W, x = px - y * W;
            const bool erased = y >= er_i && y < er_i + er_h && x >= er_j && x < er_j + er_w;
            o[i] = erased ? 0.f : s_norm[cur[px * 3 + c]];
        }
    }
}

}  // namespace

size_t augment_lds_bytes(int H, int W) {
    const size_t nby = ((size_t)H * W * 3 + 15) & ~(size_t)15;
    return 2 * nby + 16 * ((size_t)W + H);
}

hipError_t launch_augment(const uint8_t* in, int B, int H, int W, const int32_t* ops, const double* args, int n_ops,
                          const float* norm, float* out_f32, uint8_t* out_u8, hipStream_t s) {
    const int lds = (int)augment_lds_bytes(H, W);
    hipError_t e = lds_opt_in((const void*)augment_kernel, lds);
    if (e != hipSuccess) return e;
    AugParams p{in, ops, args, norm, out_f32, out_u8, H, W, n_ops};
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)B), dim3(AUG_THREADS), (size_t)lds, s, p);
    return hipGetLastError();
}

}  // namespace fr
