// FP8 implicit-GEMM convolution for CDNA4 (gfx950): BASELINE config 5 ("ArcFace fp8 weights, CDNA4
// fp8 MFMA").  Same GEMM view, DMA staging and fused epilogue as conv_igemm.hip, but each K-step is
// 128 deep and runs on the block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, 2x the bf16
// MFMA rate):
//   * weights: OCP e4m3 [Npad][Kpad8] (Kpad8 % 128 == 0), per-output-channel f32 scale sw[n]
//     (host quantization, weights.py -> engine make_convw), applied in the epilogue;
//   * activations stay bf16 in HBM and LDS (the residual stream keeps bf16 precision); each MFMA
//     operand is converted in registers with v_cvt_scalef32_pk_fp8_bf16 (x / 2^e) and the MFMA's
//     e8m0 B-scale multiplies 2^e back, so no product leaves the fp8 range.  e is the per-tensor
//     power of two with amax(x) / 2^e <= 448, from the producer epilogue's atomic amax (dynamic
//     per-tensor scaling; the hardware converter does not saturate: > ~464 would become NaN).
// The epilogue optionally records amax(|y|) of what it stores (atomicMax on the f32 bit pattern) for
// the next conv.  Requirements: Cin % 64 == 0 (every IResNet100 conv but the bf16 stem).
#include "conv_epilogue.h"
#include "kernels.h"
#include "lds_dma.h"

#include <hip/hip_ext.h>

namespace fr {
namespace {

constexpr int KS = 128;                // K per step
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) short i16x2_t;

// power-of-two activation scale exponent: amax / 2^e <= 448
__device__ __forceinline__ int act_exp(const float* amax, int slots) {
    float a = 448.f;
    if (amax) {
        a = 0.f;
        for (int i = 0; i < slots; ++i) a = fmaxf(a, amax[i]);
    }
    if (!(a > 0.f)) return 0;
    int e = (int)ceilf(log2f(a / 448.f));
    return e < -60 ? -60 : (e > 60 ? 60 : e);
}

// 8 bf16 (one uint4) -> 8 e4m3 bytes (two dwords), x / 2^e
__device__ __forceinline__ uint2 cvt8(const uint4& v, float scale) {
    i16x2_t o0 = {0, 0}, o1 = {0, 0};
    o0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o0, __builtin_bit_cast(bf16x2_t, v.x), scale, false);
    o0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o0, __builtin_bit_cast(bf16x2_t, v.y), scale, true);
    o1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o1, __builtin_bit_cast(bf16x2_t, v.z), scale, false);
    o1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o1, __builtin_bit_cast(bf16x2_t, v.w), scale, true);
    return make_uint2(__builtin_bit_cast(uint32_t, o0), __builtin_bit_cast(uint32_t, o1));
}

// blocks per CU that the two LDS stages allow (2 x (2*BM + BN) x 128 B)
template <int BM, int BN>
struct Fp8Occ {
    static constexpr int value = 2 * (2 * BM + BN) * 128 <= 80 * 1024 ? 2 : 1;
};

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, (Fp8Occ<BM, BN>::value)) void conv_fp8_kernel(ConvArgs p, int tiles_n) {
    constexpr int NW = WM * WN, NT = 64 * NW;
    static_assert(NW == 4, "4 waves");
    constexpr int TWM = BM / WM, TWN = BN / WN;
    constexpr int FM = TWM / 16, FN = TWN / 16;
    constexpr int NA = BM / (8 * NW), NB = BN / (8 * NW);
    constexpr int SUB_A = BM * 128;                  // one 64-channel bf16 sub-tile
    constexpr int STAGE = 2 * SUB_A + BN * 128;      // [A0][A1][W]
    constexpr int EPI_LD = BN + 4;
    constexpr int LDS_BYTES = 2 * STAGE > BM * EPI_LD * 4 ? 2 * STAGE : BM * EPI_LD * 4;
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = lid / tiles_n, tn = lid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nkt = p.Kpad / KS;

    const int lrow = lane >> 3;
    const int cl = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);
    const uint32_t x_bytes = clamp31((size_t)p.B * p.H * p.W * p.Cx * 2);
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(p.x, x_bytes);
    const uint32_t w_bytes = clamp31((size_t)p.Npad * p.Kpad);
    const __amdgpu_buffer_rsrc_t wr = buffer_rsrc(p.w8, w_bytes);

    const int HoWo = p.Ho * p.Wo;
    int a_ih[NA], a_iw[NA];
    uint32_t a_base[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int m = m0 + 8 * (wave + NW * i) + lrow;
        if (m < p.M) {
            const int b = m / HoWo, r = m - b * HoWo;
            const int oh = r / p.Wo, ow = r - oh * p.Wo;
            a_ih[i] = oh * p.sh - p.ph;
            a_iw[i] = ow * p.sw - p.pw;
            a_base[i] = (uint32_t)((((b * p.H + a_ih[i]) * p.W + a_iw[i]) * p.Cx + p.x_off + 8 * cl) * 2);
        } else {
            a_ih[i] = -(1 << 28);
            a_iw[i] = 0;
            a_base[i] = 0;
        }
    }
    uint32_t b_base[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) b_base[j] = (uint32_t)((n0 + 8 * (wave + NW * j) + lrow) * p.Kpad + 16 * cl);

    // one 64-channel activation chunk q (k = 64q .. 64q+63: tap rs = 64q / Cin, channels c0 = 64q % Cin)
    auto issue_a = [&](int q, char* dst) {
        const int k0 = q * 64;
        const int rs = k0 / p.Cin, c0 = k0 - rs * p.Cin;
        const int r = rs / p.Kw, s = rs - r * p.Kw;
        const bool kin = k0 < p.K;
        const int soff = ((r * p.W + s) * p.Cx + c0) * 2;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int ih = a_ih[i] + r, iw = a_iw[i] + s;
            const bool ok = kin && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            dma16(xr, dst + (wave + NW * i) * 1024, ok ? a_base[i] + (uint32_t)soff : OOB);
        }
    };
    auto issue = [&](int kt, int buf) {
        char* st = smem + buf * STAGE;
        issue_a(2 * kt, st);
        issue_a(2 * kt + 1, st + SUB_A);
#pragma unroll
        for (int j = 0; j < NB; ++j) dma16(wr, st + 2 * SUB_A + (wave + NW * j) * 1024, b_base[j] + (uint32_t)(kt * KS));
    };

    const int ex = act_exp(p.x_amax, max(p.amax_slots, 1));
    const float xs = __builtin_bit_cast(float, (uint32_t)(127 + ex) << 23);  // 2^ex
    const int scale_b = 127 + ex;

    f32x4_t acc[FN][FM];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4;
    auto compute = [&](int buf) {
        const char* st = smem + buf * STAGE;
        i32x8_t wf[FN], af[FM];
#pragma unroll
        for (int i = 0; i < FN; ++i) {  // weights: 32 k-bytes per lane = 16-B chunks 2g, 2g+1
            const int row = wn * TWN + i * 16 + (lane & 15);
            const uint4 lo = *(const uint4*)(st + 2 * SUB_A + row * 128 + swz(row, 2 * g) * 16);
            const uint4 hi = *(const uint4*)(st + 2 * SUB_A + row * 128 + swz(row, 2 * g + 1) * 16);
            wf[i] = (i32x8_t){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        }
#pragma unroll
        for (int j = 0; j < FM; ++j) {  // activations: k = 32g .. 32g+31 -> sub-tile g>>1, chunks 4(g&1)..+3
            const int row = wm * TWM + j * 16 + (lane & 15);
            const char* sa = st + (g >> 1) * SUB_A + row * 128;
            uint2 q[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = cvt8(*(const uint4*)(sa + swz(row, 4 * (g & 1) + c) * 16), xs);
            af[j] = (i32x8_t){(int)q[0].x, (int)q[0].y, (int)q[1].x, (int)q[1].y, (int)q[2].x, (int)q[2].y, (int)q[3].x,
                              (int)q[3].y};
        }
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[i], af[j], acc[i][j], 0, 0, 0, 127, 0,
                                                                             scale_b);
    };

    if (nkt > 0) {
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    int buf = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) issue(kt + 1, buf ^ 1);
        compute(buf);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
    }

    // epilogue: accumulators -> LDS f32 tile -> 8-channel groups (fixed channel group per thread)
    float* sE = (float*)smem;
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) {
            const int ml = wm * TWM + j * 16 + (lane & 15);
            const int nl = wn * TWN + i * 16 + 4 * (lane >> 4);
            *(f32x4_t*)(sE + ml * EPI_LD + nl) = acc[i][j];
        }
    __syncthreads();
    constexpr int G = BN / 8, RS = NT / G, ITER = BM / RS;
    static_assert(NT % G == 0 && BM % RS == 0, "epilogue mapping");
    const int gg = tid % G, ml0 = tid / G;
    const int n = n0 + gg * 8;
    const bool nv = n < p.Cout;
    const int nn = nv ? n : 0;
    ConvEpilogue<false, 8, EPI_Y2 | EPI_WSCALE | EPI_BIAS9> ep;
    ep.load(p, nn);
    float amax = 0.f;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int ml = ml0 + it * RS, m = m0 + ml;
        if (m >= p.M || !nv) continue;
        float v[8];
        load_f(sE + ml * EPI_LD + gg * 8, v);
        uint4 r;
        if (p.res) r = *(const uint4*)(p.res + (size_t)m * p.Cres + p.res_off + n);
        ep.apply(p, v, p.res != nullptr, r, border_class_of(p, m));
        amax = amax_fold(amax, v);
        ep.store(p, m, n, v);
    }
    if (p.y_amax) amax_publish(p.y_amax, blockIdx.x % max(p.amax_slots, 1), amax);
}

template <int BM, int BN, int WM, int WN>
hipError_t launch_fp8_variant(const ConvArgs& a, hipStream_t s) {
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.Cout + BN - 1) / BN;
    dim3 grid(tiles_m * tiles_n), block(64 * WM * WN);
    auto k = conv_fp8_kernel<BM, BN, WM, WN>;
    if (a.ev0)
        hipExtLaunchKernelGGL(k, grid, block, 0, s, (hipEvent_t)a.ev0, (hipEvent_t)a.ev1, 0, a, tiles_n);
    else
        hipLaunchKernelGGL(k, grid, block, 0, s, a, tiles_n);
    return hipGetLastError();
}

}  // namespace

// Tile choice: the bf16 planner's shape classes (N <= 64 -> 128x64, else 64x128 or 128x128 by size).
int conv_fp8_tile(int M, int Cout) {
    if (Cout <= 64) return TILE_128x64;
    const long t128 = (long)((M + 127) / 128) * ((Cout + 127) / 128);
    return t128 >= 512 ? TILE_128x128 : TILE_64x128;
}

hipError_t launch_conv_fp8(const ConvArgs& a, hipStream_t s) {
    if (a.Cin % 64 != 0 || a.Kpad % KS != 0 || !a.w8 || !a.wscale || a.x2) return hipErrorInvalidValue;
    switch (a.tile) {
        // 4 x 1 waves: each wave converts only its own activation fragments (2 x 2 converted every
        // fragment twice; the bf16 -> e4m3 conversion costs as much issue time as the fp8 MFMAs)
        case TILE_128x64: return launch_fp8_variant<128, 64, 4, 1>(a, s);
        case TILE_64x128: return launch_fp8_variant<64, 128, 4, 1>(a, s);
        default: return launch_fp8_variant<128, 128, 4, 1>(a, s);
    }
}

}  // namespace fr
