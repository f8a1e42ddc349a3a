// The implicit-GEMM conv epilogue, written once: what turns the f32 accumulators of NC consecutive output channels
// of one pixel (NC = 8 or 4) into stored activations,
//
//   v = acc [* wscale] + bias  ->  + bias9[border class]  ->  + residual  ->  ReLU / PReLU
//     ->  (amax)  ->  pack bf16 / f16 (or bf16 from an f16 conv)  ->  store y  ->  y2 = v * aff_s + aff_b
//
// in three steps that a kernel issues when it suits its own schedule: load() the per-channel vectors once per
// channel group, apply() per pixel on the accumulators and on the residual bits the kernel already holds, store().
// A kernel that claims conv_igemm tile 0's bits (convs.cpp K_IGEMM) takes its epilogue from here, so that half of the
// claim holds by construction; DESIGN.md lists the sites that keep a copy, with the measured reason.  Included by
// kernel files only, as lds_dma.h.
//
// The bias is added unconditionally (zeros where the conv has none, or has the border-class table instead): an
// accumulator that starts at +0 and is summed by MFMA or += is never -0, and x + (+0) == x bit for bit for every
// other x.  (The weight scales of the fp8 conv are positive, so acc * wscale is no -0 either.)
#pragma once
#include "kernels.h"
#include "lds_dma.h"

namespace fr {

// what a kernel's epilogue takes beyond bias, bias9, residual and activation
enum : int {
    EPI_Y2 = 1,      // the second output y2 = v * aff_s + aff_b
    EPI_YBF16 = 2,   // ConvArgs::y_bf16: the bf16 store of an f16 conv
    EPI_WSCALE = 4,  // the fp8 conv's per-channel weight scale
    EPI_BIAS9 = 8,   // the bias9 row of each pixel's border class, loaded where it is applied
};

// NC consecutive floats by 16-byte loads
template <int NC>
__device__ __forceinline__ void load_f(const float* src, float (&f)[NC]) {
    static_assert(NC % 4 == 0, "whole float4s");
#pragma unroll
    for (int q = 0; q < NC / 4; ++q) {
        const float4 t = *(const float4*)(src + 4 * q);
        f[4 * q] = t.x; f[4 * q + 1] = t.y; f[4 * q + 2] = t.z; f[4 * q + 3] = t.w;
    }
}

// NC 16-bit values: the residual bits a kernel loads, the packed value it stores
template <int NC> struct EpiBits;
template <> struct EpiBits<8> { typedef uint4 type; };
template <> struct EpiBits<4> { typedef uint2 type; };

template <bool F16>
__device__ __forceinline__ void unpack_f(const uint4& r, float (&f)[8]) { Num<F16>::unpack8(r, f); }
template <bool F16>
__device__ __forceinline__ void unpack_f(const uint2& r, float (&f)[4]) {
    float t[8];
    Num<F16>::unpack8(make_uint4(r.x, r.y, 0u, 0u), t);
    f[0] = t[0]; f[1] = t[1]; f[2] = t[2]; f[3] = t[3];
}
template <bool F16>
__device__ __forceinline__ uint4 pack_f(const float (&v)[8]) { return Num<F16>::pack8(v); }
template <bool F16>
__device__ __forceinline__ uint2 pack_f(const float (&v)[4]) { return pack4<F16>(v[0], v[1], v[2], v[3]); }

// Border class of output pixel m = (b, oh, ow) of the conv, for its bias9 table
__device__ __forceinline__ int border_class_of(const ConvArgs& p, int m) {
    const int r = m % (p.Ho * p.Wo);
    return border_class(r / p.Wo, r % p.Wo, p.Ho, p.Wo);
}

template <bool F16, int NC, int FEAT>
struct ConvEpilogue {
    typedef typename EpiBits<NC>::type bits;
    int n;                                                        // first channel of the group
    float wscale[NC], bias[NC], slope[NC], aff_s[NC], aff_b[NC];  // only what FEAT and the conv use is ever loaded

    // Once per channel group n .. n + NC - 1 (a valid address: the caller clamps a group past Cout).  Nothing is read
    // through a null pointer: slope only for PReLU, aff_* only with y2, bias9 takes precedence over bias.  on: the
    // lane takes part (others keep a zero bias and load nothing).
    __device__ __forceinline__ void load(const ConvArgs& p, int n_, bool on = true) {
        n = n_;
        // (only the zero bias is ever read unloaded; the others start defined because left undefined they cost
        // conv3x3_band_kernel<14, 14, 2, 4, 7, 4, 3> four more VGPR spills: 19 -> 23, scratch 80 -> 96 B)
#pragma unroll
        for (int e = 0; e < NC; ++e) bias[e] = slope[e] = aff_s[e] = aff_b[e] = 0.f;
        if (FEAT & EPI_WSCALE) load_f(p.wscale + n, wscale);
        if (p.bias && !p.bias9 && on) load_f(p.bias + n, bias);
        if (p.act == 2 && on) load_f(p.slope + n, slope);
        if ((FEAT & EPI_Y2) && p.y2) {
            load_f(p.aff_s + n, aff_s);
            load_f(p.aff_b + n, aff_b);
        }
    }
    // A kernel whose thread keeps one pixel (not EPI_BIAS9) loads that pixel's bias9 row in place of the zero bias,
    // before its K loop: acc + 0 + bias9 and acc + bias9 are the same bits
    __device__ __forceinline__ void load_bias9(const ConvArgs& p, int cls, bool on = true) {
        static_assert(!(FEAT & EPI_BIAS9), "one way or the other");
        if (p.bias9 && on) load_f(p.bias9 + (size_t)cls * p.Npad + n, bias);
    }

    // Per pixel, in place on the accumulators: bias, bias9 row of the pixel's border class cls (EPI_BIAS9), residual
    // (res, the bits the caller loaded, read when has_res), activation (1 = ReLU, 2 = PReLU).
    __device__ __forceinline__ void apply(const ConvArgs& p, float (&v)[NC], bool has_res, const bits& res,
                                          int cls = 0) const {
#pragma unroll
        for (int e = 0; e < NC; ++e) v[e] = (FEAT & EPI_WSCALE) ? v[e] * wscale[e] + bias[e] : v[e] + bias[e];
        if ((FEAT & EPI_BIAS9) && p.bias9) {
            float b9[NC];
            load_f(p.bias9 + (size_t)cls * p.Npad + n, b9);
#pragma unroll
            for (int e = 0; e < NC; ++e) v[e] += b9[e];
        }
        if (has_res) {
            float f[NC];
            unpack_f<F16>(res, f);
#pragma unroll
            for (int e = 0; e < NC; ++e) v[e] += f[e];
        }
        if (p.act == 1) {
#pragma unroll
            for (int e = 0; e < NC; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        } else if (p.act == 2) {
#pragma unroll
            for (int e = 0; e < NC; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * slope[e];
        }
    }

    // The stored bits of v (for a kernel with a store of its own, e.g. through a buffer resource)
    __device__ __forceinline__ bits pack(const ConvArgs& p, const float (&v)[NC]) const {
        return (FEAT & EPI_YBF16) && F16 && p.y_bf16 ? pack_f<false>(v) : pack_f<F16>(v);
    }

    // y (and y2) of output pixel m at channels n_ .. n_ + NC - 1 (n_: the group unclamped, in a kernel that clamped
    // the group it loaded): one 16-byte (NC = 8) or 8-byte (NC = 4) store each
    __device__ __forceinline__ void store(const ConvArgs& p, size_t m, int n_, const float (&v)[NC]) const {
        *(bits*)(p.y + m * p.Cy + p.y_off + n_) = pack(p, v);
        if ((FEAT & EPI_Y2) && p.y2) {
            float u[NC];
#pragma unroll
            for (int e = 0; e < NC; ++e) u[e] = v[e] * aff_s[e] + aff_b[e];
            *(bits*)(p.y2 + m * p.Cy2 + p.y2_off + n_) = pack_f<F16>(u);
        }
    }
};

// max |y| for an fp8 consumer's dynamic activation scale: fold a thread's stored values ...
template <int NC>
__device__ __forceinline__ float amax_fold(float amax, const float (&v)[NC]) {
#pragma unroll
    for (int e = 0; e < NC; ++e) amax = fmaxf(amax, fabsf(v[e]));
    return amax;
}
// ... then the wave's maximum into y_amax[slot] (amax >= 0: the f32 bit order is the value order)
__device__ __forceinline__ void amax_publish(float* y_amax, int slot, float amax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)y_amax + slot, __float_as_uint(amax));
}

}  // namespace fr
