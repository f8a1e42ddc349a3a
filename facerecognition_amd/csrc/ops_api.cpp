// C ABI of the stateless ops (include/frhip.h "op-level entry points", "crop preparation", "face detection"): one
// launch each on caller-owned buffers, no handle -- fr_op_*, the u8 image ops and the MTCNN layers.  How
// fr_op_conv2d_ex picks or forces a conv kernel is in convs.cpp.
#include <string>

#include "engine_internal.h"

using namespace fr;

extern "C" {

int fr_op_conv2d(const fr_conv_desc* d, void* stream) { return fr_op_conv2d_ex(d, nullptr, stream); }

int fr_op_conv2d_ex(const fr_conv_desc* d, const fr_conv_ext* e, void* stream) {
    if (!d || !d->x || !d->w || !d->y || d->B <= 0 || d->Cin <= 0 || d->Cin % 8 || d->Cx % 8 || d->x_off % 8 ||
        d->Cout <= 0 || d->Cout % 8 || d->Cy % 8 || d->y_off % 8 || d->Npad % 128 || d->Kpad % 64 ||
        d->Npad < d->Cout || d->Kpad < d->Kh * d->Kw * d->Cin || d->x_off + d->Cin > d->Cx ||
        d->y_off + d->Cout > d->Cy || (d->act == 2 && !d->slope) || (d->res && (d->Cres % 8 || d->res_off % 8)) ||
        (d->y2 && (!d->aff_s || !d->aff_b || d->Cy2 % 8 || d->y2_off % 8)) || d->stride_h <= 0 || d->stride_w <= 0) {
        set_error("fr_op_conv2d: bad descriptor (see alignment rules in frhip.h)");
        return FR_ERR_ARG;
    }
    ConvArgs a{};
    a.x = (const bf16_t*)d->x; a.B = d->B; a.H = d->H; a.W = d->W; a.Cx = d->Cx; a.x_off = d->x_off; a.Cin = d->Cin;
    a.w = (const bf16_t*)d->w; a.Kh = d->Kh; a.Kw = d->Kw; a.sh = d->stride_h; a.sw = d->stride_w;
    a.ph = d->pad_h; a.pw = d->pad_w; a.K = d->Kh * d->Kw * d->Cin; a.Kpad = d->Kpad;
    a.Ho = d->Ho ? d->Ho : (d->H + 2 * d->pad_h - d->Kh) / d->stride_h + 1;
    a.Wo = d->Wo ? d->Wo : (d->W + 2 * d->pad_w - d->Kw) / d->stride_w + 1;
    a.M = d->B * a.Ho * a.Wo; a.Cout = d->Cout; a.Npad = d->Npad;
    a.bias = d->bias; a.slope = d->slope; a.act = d->act; a.bias9 = d->bias9;
    a.res = (const bf16_t*)d->res; a.Cres = d->Cres; a.res_off = d->res_off;
    a.y = (bf16_t*)d->y; a.Cy = d->Cy; a.y_off = d->y_off;
    a.y2 = (bf16_t*)d->y2; a.Cy2 = d->Cy2; a.y2_off = d->y2_off; a.aff_s = d->aff_s; a.aff_b = d->aff_b;
    a.f16 = d->dtype == FR_DTYPE_F16;
    a.y_amax = d->y_amax;
    a.amax_slots = 1;
    int* splitk_cnt = nullptr;
    if (e) {
        // every refusal is made here, on the host, before any launch: a kernel that cannot run a field never sees it
        const auto refuse = [](const char* why) {
            set_error(std::string("fr_op_conv2d_ex: ") + why);
            return FR_ERR_ARG;
        };
        const int tile = d->tile;  // its kernel takes a field or not: convs.cpp's table
        const int takes = op_tile_takes(tile);
        if (e->amax_slots < 0) return refuse("amax_slots < 0");
        if (e->amax_slots > 0) a.amax_slots = e->amax_slots;
        if (e->x2) {
            if (d->dtype == FR_DTYPE_FP8) return refuse("the K-concatenated projection (x2) has no fp8 kernel");
            if (!(takes & CONV_TAKES_X2))
                return refuse(("the K-concatenated projection (x2) runs only on " + conv_takers(CONV_TAKES_X2)).c_str());
            if (e->st2 <= 0 || e->H2 <= 0 || e->W2 <= 0 || e->C2 <= 0 || e->x2_off < 0 || e->Cx2 % 8 || e->x2_off % 8 ||
                d->Cin % 64 || e->C2 % 64 || a.K + e->C2 > d->Kpad || e->x2_off + e->C2 > e->Cx2 ||
                (a.Ho - 1) * e->st2 >= e->H2 || (a.Wo - 1) * e->st2 >= e->W2)
                return refuse("bad projection (x2): needs Cin % 64 == 0, C2 % 64 == 0, Kh*Kw*Cin + C2 <= Kpad, "
                              "x2_off + C2 <= Cx2, Cx2 % 8 == 0, x2_off % 8 == 0, (Ho-1)*st2 < H2, (Wo-1)*st2 < W2");
            a.x2 = (const bf16_t*)e->x2; a.H2 = e->H2; a.W2 = e->W2; a.Cx2 = e->Cx2; a.x2_off = e->x2_off;
            a.C2 = e->C2; a.st2 = e->st2; a.K1 = a.K;
            a.K = a.K1 + a.C2;
        }
        if (e->y_bf16) {
            if (d->dtype != FR_DTYPE_F16 || d->res || d->y2) return refuse("y_bf16 needs FR_DTYPE_F16 and neither res nor y2");
            if (!(takes & CONV_TAKES_Y_BF16)) return refuse(("y_bf16 runs only on " + conv_takers(CONV_TAKES_Y_BF16)).c_str());
            a.y_bf16 = 1;
        }
        if (e->splitk_cnt) {
            if (!(takes & CONV_TAKES_SPLITK_CNT) || d->dtype == FR_DTYPE_FP8) return refuse("splitk_cnt (in-launch split-K) is for the implicit-GEMM tiles only");
            // (the in-launch slabs are addressed by 32-bit buffer offsets)
            if (d->split_k > 1 && (size_t)d->split_k * a.M * a.Npad * sizeof(float) >= 0x7fffffffull)
                return refuse("splitk_cnt: the partial workspace must stay below 2 GiB");
            splitk_cnt = e->splitk_cnt;
        }
    }
    if (d->dtype == FR_DTYPE_FP8) {
        if (!d->wscale || !d->x_amax || d->Cin % 64 || d->Kpad % 128 || d->split_k > 1) {
            set_error("fr_op_conv2d: fp8 needs wscale, x_amax, Cin % 64 == 0, Kpad % 128 == 0, no split-K");
            return FR_ERR_ARG;
        }
        a.w8 = (const uint8_t*)d->w; a.wscale = d->wscale; a.x_amax = d->x_amax;
        a.tile = conv_fp8_tile(a.M, a.Cout);
        if (d->tile > 0) {  // conv_fp8.hip has three tiles; any other id would run the 128x128 one under a wrong name
            a.tile = d->tile - 1;
            if (a.tile != TILE_128x128 && a.tile != TILE_128x64 && a.tile != TILE_64x128) {
                set_error("fr_op_conv2d: fp8 runs on FR_TILE_128x128, FR_TILE_128x64 and FR_TILE_64x128 only");
                return FR_ERR_ARG;
            }
        }
        FR_HIP_CHECK(launch_conv_fp8(a, (hipStream_t)stream));
        return FR_OK;
    }
    if (op_tile_forced_kind(d->tile))  // a specialised kernel (split_k: its own split, conv_small.hip's KS | NF << 8)
        return run_forced_kind(d->tile, a, d->split_k > 1 ? d->split_k : 1, (hipStream_t)stream);
    if (d->tile > 0) {
        if (!op_tile_is_igemm(d->tile)) {
            set_error("fr_op_conv2d: bad tile");
            return FR_ERR_ARG;
        }
        a.tile = d->tile - 1;
    } else {
        int tile, sp;
        conv_plan(a.M, a.Cout, a.Kpad, &tile, &sp);
        a.tile = tile;
    }
    if (d->split_k > 1) {
        if (!d->partial) { set_error("fr_op_conv2d: split_k > 1 needs partial workspace"); return FR_ERR_ARG; }
        a.split_k = d->split_k;
        a.partial = d->partial;
        a.splitk_cnt = splitk_cnt;  // non-null: the tiles' last workgroups reduce, no second launch
        FR_HIP_CHECK(launch_conv(a, (hipStream_t)stream));
        if (!a.splitk_cnt) FR_HIP_CHECK(launch_splitk_epilogue(a, (hipStream_t)stream));
    } else {
        a.split_k = 1;
        FR_HIP_CHECK(launch_conv(a, (hipStream_t)stream));
    }
    return FR_OK;
}

size_t fr_resize_u8_workspace(int B, int H, int W, int OH, int OW) {
    if (B <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return 0;
    return resize_u8_workspace(B, H, W, OH, OW);
}

int fr_resize_u8(const uint8_t* in, int B, int H, int W, uint8_t* out, int OH, int OW, void* ws, size_t ws_bytes,
                 void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || (size_t)B * H * W * 3 > 0x7fffffffull * 4) {
        set_error("fr_resize_u8: bad argument");
        return FR_ERR_ARG;
    }
    if (ws_bytes < resize_u8_workspace(B, H, W, OH, OW) || (!ws && ws_bytes == 0 && W != OW)) {
        set_error("fr_resize_u8: workspace smaller than fr_resize_u8_workspace()");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_resize_u8(in, B, H, W, out, OH, OW, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_warp_affine_u8(const uint8_t* in, int B, int H, int W, const double* M, uint8_t* out, int OH, int OW,
                      void* stream) {
    if (!in || !out || !M || B <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) {
        set_error("fr_warp_affine_u8: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_warp_affine_u8(in, B, H, W, M, out, OH, OW, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_preprocess(const void* in, int in_fmt, int B, int H, int W, void* out, int dtype, void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || (in_fmt != FR_IN_U8_NHWC && in_fmt != FR_IN_F32_NCHW)) {
        set_error("fr_op_preprocess: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_preprocess(in, in_fmt, B, H, W, (bf16_t*)out, dtype == FR_DTYPE_F16, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_maxpool(const void* x, int B, int H, int W, int Cx, int x_off, int C, int k, int stride, int pad, void* y,
                  int Cy, int y_off, int Ho, int Wo, int dtype, void* stream) {
    if (!x || !y || C % 8 || Cx % 8 || x_off % 8 || Cy % 8 || y_off % 8 || k <= 0 || stride <= 0 || pad < 0 ||
        pad >= k) {
        set_error("fr_op_maxpool: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_maxpool((const bf16_t*)x, B, H, W, Cx, x_off, C, k, stride, pad, (bf16_t*)y, Cy, y_off, Ho,
                                Wo, dtype == FR_DTYPE_F16, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_avgpool(const void* x, int B, int H, int W, int C, void* y, int dtype, void* stream) {
    if (!x || !y || C % 8) { set_error("fr_op_avgpool: bad argument"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_avgpool((const bf16_t*)x, B, H, W, C, (bf16_t*)y, dtype == FR_DTYPE_F16, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_linear(const void* x, int B, int K, const void* w, int N, int Npad, int Kpad, const float* bias,
                 int normalize, float* out, int split_k, float* partial, int dtype, void* stream) {
    if (!x || !w || !out || !partial || B <= 0 || K <= 0 || K % 8 || N <= 0 || N % 8 || Npad % 128 || Kpad % 64 ||
        Npad < N || Kpad < K || split_k <= 0) {
        set_error("fr_op_linear: bad argument");
        return FR_ERR_ARG;
    }
    ConvArgs a{};
    a.x = (const bf16_t*)x; a.B = B; a.H = 1; a.W = 1; a.Cx = K; a.x_off = 0; a.Cin = K;
    a.w = (const bf16_t*)w; a.Kh = 1; a.Kw = 1; a.sh = 1; a.sw = 1; a.K = K; a.Kpad = Kpad;
    a.Ho = 1; a.Wo = 1; a.M = B; a.Cout = N; a.Npad = Npad;
    a.split_k = split_k;
    a.partial = partial;
    a.f16 = dtype == FR_DTYPE_F16;
    {
        int tile, sp;
        conv_plan(a.M, a.Cout, a.Kpad, &tile, &sp);
        a.tile = tile;
    }
    FR_HIP_CHECK(launch_conv(a, (hipStream_t)stream));
    FR_HIP_CHECK(launch_head_finalize(partial, split_k, B, N, Npad, bias, normalize, out, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_head_gemv(const void* x, int B, int K, const void* w, int N, int Npad, int Kpad, const float* bias,
                    int normalize, float* out, int S, float* partial, int dtype, void* stream) {
    if (!x || !w || !out || !partial || K <= 0 || N <= 0 || Npad < N || S < 1 || Kpad % 8 || N % 4 || N > 1024 ||
        (dtype != FR_DTYPE_BF16 && dtype != FR_DTYPE_F16) || !head_gemv_supported(B, K, Kpad, Npad)) {
        set_error("fr_op_head_gemv: bad argument (1 <= B <= 8, K % 8 == 0, Kpad % 8 == 0, Kpad >= K, Npad % 16 == 0, "
                  "N % 4 == 0, N <= 1024, S >= 1, bf16 / f16)");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_head_gemv((const bf16_t*)x, B, K, (const bf16_t*)w, Kpad, N, Npad, S, dtype == FR_DTYPE_F16,
                                  partial, (hipStream_t)stream));
    FR_HIP_CHECK(launch_head_finalize(partial, S, B, N, Npad, bias, normalize, out, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_head_grad(const float* g, int B, int N, const void* w, int K, int Kpad, int dtype, float* v, void* stream) {
    if (!g || !w || !v || (dtype != FR_DTYPE_BF16 && dtype != FR_DTYPE_F16) || !head_grad_supported(B, N, K, Kpad)) {
        set_error("fr_op_head_grad: bad argument (B >= 1, 1 <= N <= 1024, K % 8 == 0, Kpad % 8 == 0, Kpad >= K, bf16 / f16)");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_head_grad(g, B, N, (const bf16_t*)w, K, Kpad, dtype == FR_DTYPE_F16, v, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_cam(const void* act, int B, int h, int w, int C, int dtype, const float* v, int v_layout, int S, float* cam,
              float* low, void* stream) {
    if (!act || !cam || (dtype != FR_DTYPE_BF16 && dtype != FR_DTYPE_F16) || v_layout < 0 || v_layout > 2 ||
        (v_layout != 2 && !v) || !cam_supported(B, h, w, C, S)) {
        set_error("fr_op_cam: bad argument (h * w <= 256, C % 8 == 0, C <= 4096, 1 <= S <= 4096, v_layout 0 / 1 with v, "
                  "2 without, bf16 / f16)");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_cam((const bf16_t*)act, B, h, w, C, dtype == FR_DTYPE_F16, v, v_layout == 0 ? C : h * w * C,
                            v_layout, S, cam, low, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_proj_l2(const float* x, int B, int K, const float* W, const float* bias, int N, int normalize, float* out,
                  void* stream) {
    if (!x || !W || !out || B <= 0 || K <= 0 || K > 1024 || N <= 0) {
        set_error("fr_op_proj_l2: bad argument (1 <= K <= 1024)");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_proj_l2(x, B, K, W, bias, N, normalize, out, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_l2norm_rows(float* x, int B, int D, void* stream) {
    if (!x || B <= 0 || D <= 0) { set_error("fr_op_l2norm_rows: bad argument"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_l2norm_rows(x, B, D, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_amax(const void* x, size_t n, int dtype, float* amax, int slots, void* stream) {
    if (!x || !amax || n == 0 || n % 8 || slots < 1 || (dtype != FR_DTYPE_BF16 && dtype != FR_DTYPE_F16)) {
        set_error("fr_op_amax: bad argument (n % 8 == 0, slots >= 1, bf16 / f16)");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_amax((const bf16_t*)x, n, dtype == FR_DTYPE_F16, amax, slots, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_maxpool_cvt(const void* x, int B, int H, int W, int Cx, int x_off, int C, int k, int stride, int pad, void* y,
                      int Cy, int y_off, int Ho, int Wo, void* stream) {
    if (!x || !y || B <= 0 || C <= 0 || C % 8 || Cx % 8 || x_off % 8 || Cy % 8 || y_off % 8 || k != 3 || stride <= 0 ||
        pad < 0 || pad >= k) {
        set_error("fr_op_maxpool_cvt: bad argument (the f16 -> bf16 pool is 3x3 only)");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_maxpool((const bf16_t*)x, B, H, W, Cx, x_off, C, k, stride, pad, (bf16_t*)y, Cy, y_off, Ho, Wo, 1,
                                (hipStream_t)stream, 1));
    return FR_OK;
}

/* ---- MTCNN face detector building blocks (mtcnn.hip) ---- */
int fr_area_resample_u8(const uint8_t* img, int H, int W, const int32_t* regions, int n, int oh, int ow, float* out,
                        void* stream) {
    if (!img || !regions || !out || H <= 0 || W <= 0 || n <= 0 || oh <= 0 || ow <= 0) {
        set_error("fr_area_resample_u8: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_area_resample(img, H, W, regions, n, oh, ow, out, (hipStream_t)stream));
    return FR_OK;
}

int fr_mtcnn_conv(const float* x, int B, int H, int W, int Cin, const float* w, const float* bias, const float* slope,
                  int Cout, int kh, int kw, float* y, void* stream) {
    if (!x || !w || !y || B <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || H < kh || W < kw) {
        set_error("fr_mtcnn_conv: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_mtcnn_conv(x, B, H, W, Cin, w, bias, slope, Cout, kh, kw, y, (hipStream_t)stream));
    return FR_OK;
}

int fr_mtcnn_maxpool(const float* x, int B, int H, int W, int C, int k, int stride, float* y, void* stream) {
    if (!x || !y || B <= 0 || C <= 0 || k <= 0 || stride <= 0 || H < 1 || W < 1) {
        set_error("fr_mtcnn_maxpool: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_mtcnn_maxpool(x, B, H, W, C, k, stride, pool_ceil_out(H, k, stride), pool_ceil_out(W, k, stride),
                                      y, (hipStream_t)stream));
    return FR_OK;
}

int fr_mtcnn_dense(const float* x, int B, int K, const float* w, const float* bias, const float* slope, int N, float* y,
                   void* stream) {
    if (!x || !w || !y || B <= 0 || K <= 0 || N <= 0) { set_error("fr_mtcnn_dense: bad argument"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_mtcnn_dense(x, B, K, w, bias, slope, N, y, (hipStream_t)stream));
    return FR_OK;
}

int fr_mtcnn_head(const float* x, int64_t M, int C, const float* w, const float* bias, int n_out, float* out,
                  void* stream) {
    if (!x || !w || !bias || !out || M <= 0 || C <= 0 || n_out < 2) { set_error("fr_mtcnn_head: bad argument"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_mtcnn_head(x, M, C, w, bias, n_out, out, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
