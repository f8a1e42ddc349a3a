// frhip conv kernels: how a conv of a forward plan (or of the op API) gets its kernel.  The implicit-GEMM tiles
// (conv_igemm.hip, with split-K) are the default; beside them stand the specialised kernels, each described once in
// the table below (ConvKindDesc): when it applies, when the engine may pick it, how it is launched, what packed
// operands it needs.  This file holds that table and everything that consults it: the fixed policy, the autotuner,
// the launch with its timing scope, the load-time packer, the op API's forced dispatch and fr_debug_plan's conv
// line.  DESIGN.md "Conv kernel kinds" lists the steps to add a kernel.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>

#include "engine_internal.h"

namespace fr {

// ------------------------------------------------------------------ the kinds
// Whether a kernel sums K in the implicit GEMM's order (tile 0's bits): FR_OPT_BATCH_INVARIANT runs only those.
enum KOrder { K_OWN, K_IGEMM, K_IGEMM_UNSPLIT };  // never; always; when (split & 255) == 1

struct ConvKindDesc {
    int id;                   // FR_TILE_* (include/frhip.h)
    const char* name;         // in error messages
    const char* ab_key;       // FR_AB key (null: none) ...
    bool opt_in;              // ... that turns the kernel on (else: off)
    int rank;                 // place in the fixed policy (default_choice), 0 = not in it; the tuner times the ranked
                              // kinds first, in rank order, the others after the implicit-GEMM tiles in table order
    KOrder korder;
    int takes;                // the op-API extension fields it accepts (CONV_TAKES_*)
    bool op_sync;             // the op API runs it synchronously (scratch from hipMalloc, as it always has)
    // what a forced launch (the op API) must satisfy; split: KS | NF << 8 of conv_small.hip, else unused
    bool (*applicable)(const ConvArgs& a, int split);
    // what the engine requires in addition before it picks the kernel itself (null: only its packed operands)
    bool (*auto_ok)(const ConvArgs& a);
    // the tuner's splits for this conv in the order they are timed (null: one candidate, split 1)
    void (*splits)(const ConvArgs& a, std::vector<int>& out);
    // launches on the caller's args (no copy: the event pair ProfScope::start hangs on them reaches the kernel)
    hipError_t (*launch)(ConvArgs& a, int split, int n_cu, hipStream_t s);
    std::string (*cls)(const ConvArgs& a);  // profiling class
    // packed operands (pack == null: none): the weight image's size and packer, where the plan keeps it and where
    // the launch reads it, and whether the kernel reads the negf / ep tables
    size_t (*img_elems)(const ConvArgs& a);
    hipError_t (*pack)(const ConvArgs& a, bf16_t* out, hipStream_t s);
    bf16_t* DevConvW::*slot;
    const bf16_t* ConvArgs::*img;
    bool negf, ep;
};

static int small_nf(int split) { return (split >> 8) ? (split >> 8) : 4; }

// The launching device's CU count, for a launch outside a handle (the op API).
static int device_cus() {
    int dev = 0;
    hipDeviceProp_t prop;
    return hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
}

static bool img_applicable(const ConvArgs& a, int want_ic) {
    int ic = 0;
    return img_shape_ok(a, &ic) && ic == want_ic;
}

// Launches with the kind's own weight image in ConvArgs::wimg, where its kernel reads it.
template <class F>
static hipError_t launch_with_image(ConvArgs& a, const bf16_t* img, F launch) {
    const bf16_t* keep = a.wimg;
    a.wimg = img;
    const hipError_t e = launch();
    a.wimg = keep;
    return e;
}

// small M (a few hundred pixels: small batches): one wave per 16 px x 64 ch, no LDS, no second launch (split 4 / 8:
// that many waves share a tile's K, summed through LDS); then one wave per 16 px x 32 / 16 channels at any M:
// narrow-N convs (FaceNet Block35's N = 32 / 96) waste half of every implicit-GEMM tile.
// FR_AB small_nf4: only the 64-channel tiles (A/B)
static void small_splits(const ConvArgs& a, std::vector<int>& out) {
    static const bool small_nf4 = [] { return ab_int("small_nf4", 0) != 0; }();
    if (a.M <= 8192)
        for (int sp : {1, 4, 8, 4 | 2 << 8, 8 | 2 << 8, 4 | 1 << 8, 8 | 1 << 8, 16 | 1 << 8})
            if (!small_nf4 || sp < 256) out.push_back(sp);
    if (!small_nf4 && a.Cout <= 96)
        for (int sp : {1 | 2 << 8, 1 | 1 << 8}) out.push_back(sp);
}

static const ConvKindDesc conv_kinds[] = {
    // persistent weight-resident 3x3/s1/p1 rows, Cin = 64 (conv_rows.hip)
    {FR_TILE_ROWS, "rows", "no_rows", false, 1, K_OWN, 0, true,
     [](const ConvArgs& a, int) { return rows_supported(a); }, nullptr, nullptr,
     [](ConvArgs& a, int, int n_cu, hipStream_t s) {
         return launch_with_image(a, a.wrows_, [&] { return launch_conv_rows(a, n_cu > 0 ? n_cu : device_cus(), s); });
     },
     [](const ConvArgs& a) { return "conv3x3_rows W" + std::to_string(a.W) + " N" + std::to_string(a.Cout); },
     [](const ConvArgs& a) { return rows_packed_elems(a.Cout); },
     [](const ConvArgs& a, bf16_t* out, hipStream_t s) { return rows_pack_weights(a.w, a.Kpad, a.Cout, out, s); },
     &DevConvW::wrows, &ConvArgs::wrows_, true, true},
    // layer2 band kernel (conv_img.hip): 80 us per conv vs 86 us for the implicit GEMM (profiles/r01_img28.txt)
    {FR_TILE_IMG28, "img28", "no_img28", false, 2, K_OWN, 0, false,
     [](const ConvArgs& a, int) { return img_applicable(a, 128); }, nullptr, nullptr,
     [](ConvArgs& a, int, int, hipStream_t s) { return launch_conv_img28(a, s); },
     [](const ConvArgs&) { return std::string("conv3x3_img W28"); },
     [](const ConvArgs&) { return img_packed_elems(128); },
     [](const ConvArgs& a, bf16_t* out, hipStream_t s) { return img_pack_weights(a.w, a.Kpad, 128, out, s); },
     &DevConvW::wimg, &ConvArgs::wimg, true, false},
    // the same for 56x56x64 (layer1); opt-in
    {FR_TILE_IMG56, "img56", "img56", true, 3, K_OWN, 0, false,
     [](const ConvArgs& a, int) { return img_applicable(a, 64); }, nullptr, nullptr,
     [](ConvArgs& a, int, int, hipStream_t s) { return launch_conv_img56(a, s); },
     [](const ConvArgs&) { return std::string("conv3x3_img W56"); },
     [](const ConvArgs&) { return img_packed_elems(64); },
     [](const ConvArgs& a, bf16_t* out, hipStream_t s) { return img_pack_weights(a.w, a.Kpad, 64, out, s); },
     &DevConvW::wimg, &ConvArgs::wimg, true, false},
    // row-band direct 3x3/s1/p1 (conv_band.hip): the engine picks only the software-pipelined 14x14 variant
    {FR_TILE_BAND, "band", "no_band", false, 4, K_OWN, 0, false,
     [](const ConvArgs& a, int) { int TH, v; return band_plan(a, &TH, &v); },
     [](const ConvArgs& a) { int TH, v; return !a.y_amax && band_plan(a, &TH, &v) && v >= 3; }, nullptr,
     [](ConvArgs& a, int, int, hipStream_t s) {
         int TH, v;
         return band_plan(a, &TH, &v) ? launch_conv_band(a, TH, v, s) : hipErrorInvalidValue;
     },
     [](const ConvArgs& a) {
         int TH = 0, v = 0;
         band_plan(a, &TH, &v);
         return "conv3x3_band W" + std::to_string(a.W) + " v" + std::to_string(v);
     },
     nullptr, nullptr, nullptr, nullptr, false, false},
    // implicit GEMM with a register weight ring (conv_wring.hip): competes per shape in the tuner
    {FR_TILE_WRING, "wring", "no_wring", false, 0, K_IGEMM, CONV_TAKES_X2 | CONV_TAKES_Y_BF16, false,
     [](const ConvArgs& a, int) { return wring_supported(a); }, nullptr, nullptr,
     [](ConvArgs& a, int, int, hipStream_t s) {
         return launch_with_image(a, a.wring_, [&] { return launch_conv_wring(a, s); });
     },
     [](const ConvArgs&) { return std::string("conv_wring"); },
     [](const ConvArgs& a) { return wring_packed_elems(a.Kpad, a.Npad); },
     [](const ConvArgs& a, bf16_t* out, hipStream_t s) { return wring_pack_weights(a.w, a.Kpad, a.Npad, out, s); },
     &DevConvW::wring, &ConvArgs::wring_, false, false},
    // persistent small-K direct conv (conv_direct.hip); it queries the device's CU count itself
    {FR_TILE_DIRECT, "direct", "no_direct", false, 0, K_IGEMM, CONV_TAKES_Y_BF16, false,
     [](const ConvArgs& a, int) { return direct_supported(a); }, nullptr, nullptr,
     [](ConvArgs& a, int, int, hipStream_t s) { return launch_conv_direct(a, 0, s); },
     [](const ConvArgs&) { return std::string("conv_direct"); },
     nullptr, nullptr, nullptr, nullptr, false, false},
    // small-M implicit GEMM, one wave per tile over the whole K (conv_small.hip)
    {FR_TILE_SMALL, "small-M", nullptr, false, 0, K_IGEMM_UNSPLIT, CONV_TAKES_X2 | CONV_TAKES_Y_BF16, false,
     [](const ConvArgs& a, int split) { return small_split_ok(split) && small_supported(a, small_nf(split)); }, nullptr,
     small_splits,
     [](ConvArgs& a, int split, int, hipStream_t s) { return launch_conv_small(a, split, s); },
     [](const ConvArgs&) { return std::string("conv_small"); },
     nullptr, nullptr, nullptr, nullptr, false, false},
};

// The kind that claims tile id `id`; null: an implicit-GEMM tile (or no tile at all).
static const ConvKindDesc* conv_kind(int id) {
    for (const auto& d : conv_kinds)
        if (d.id == id) return &d;
    return nullptr;
}

static const ConvKindDesc* ranked_kind(int rank) {
    for (const auto& d : conv_kinds)
        if (d.rank == rank) return &d;
    return nullptr;
}

static bool igemm_tile_valid(int t) {
    return (t >= 0 && t < NUM_TILE_IDS) || t == TILE_64x64_S3 || t == TILE_64x64 || t == TILE_32x64_S3;
}

// The FR_AB switches, read once per process.
static bool kind_enabled(const ConvKindDesc& d) {
    static const std::vector<char> on = [] {
        std::vector<char> v;
        for (const auto& k : conv_kinds) v.push_back(!k.ab_key || (ab_int(k.ab_key, 0) != 0) == k.opt_in);
        return v;
    }();
    return on[&d - conv_kinds] != 0;
}

// Whether the engine may run kind d on conv a: switched on, applicable, its packed operands in place.
static bool kind_usable(const ConvKindDesc& d, const ConvArgs& a, int split) {
    return kind_enabled(d) && (!d.pack || a.*d.img) && (!d.negf || a.negf) && (!d.ep || a.ep) &&
           d.applicable(a, split) && (!d.auto_ok || d.auto_ok(a));
}

// A conv's kernel: an FR_TILE_* id (an implicit-GEMM tile, or the kind that claims the id) and a split: the
// split-K factor of a tile (negative: reduced in-launch), the kind's own split otherwise.
struct ConvChoice {
    int tile = -1, split = 1;
};

static bool invariant_ok(const ConvChoice& c) {
    const ConvKindDesc* d = conv_kind(c.tile);
    if (!d) return c.split == 1;
    return d->korder == K_IGEMM || (d->korder == K_IGEMM_UNSPLIT && (c.split & 255) == 1);
}

// ------------------------------------------------------------------ packed operands
// The kind's packed operands for conv a (its [Npad][Kpad] rows a.w, bias / bias9, slope) into buffers from `alloc`,
// all on stream s; operands already in place are kept (a conv's kinds share one negf table).
typedef std::function<int(void** p, size_t bytes)> ConvAlloc;

// negf [Npad] = the activation's negative-side factor (PReLU slopes, 0 for ReLU, 1 for none); ep [9][Npad] = bias9, or
// the bias for all nine border classes.  Cout floats are read from the conv's vectors (the op API's hold no more).
static int prepare(const ConvKindDesc& d, ConvArgs& a, const ConvAlloc& alloc, hipStream_t s) {
    void* p = nullptr;
    int rc;
    if (!(a.*d.img)) {
        if ((rc = alloc(&p, d.img_elems(a) * sizeof(bf16_t)))) return rc;
        FR_HIP_CHECK(d.pack(a, (bf16_t*)p, s));
        a.*d.img = (const bf16_t*)p;
    }
    if (d.negf && !a.negf) {
        if ((rc = alloc(&p, (size_t)a.Npad * sizeof(float)))) return rc;
        const float fill = a.act == ACT_RELU ? 0.f : 1.f;
        uint32_t bits;
        std::memcpy(&bits, &fill, 4);
        FR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)p, (int)bits, a.Npad, s));
        if (a.act == ACT_PRELU && a.slope) FR_HIP_CHECK(hipMemcpyAsync(p, a.slope, a.Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
        a.negf = (const float*)p;
    }
    if (d.ep && !a.ep) {
        const size_t cls = (size_t)a.Npad * sizeof(float);
        if ((rc = alloc(&p, 9 * cls))) return rc;
        if (a.bias9) FR_HIP_CHECK(hipMemcpyAsync(p, a.bias9, 9 * cls, hipMemcpyDeviceToDevice, s));
        else FR_HIP_CHECK(hipMemsetAsync(p, 0, 9 * cls, s));
        for (int k = 0; k < 9 && !a.bias9 && a.bias; ++k)
            FR_HIP_CHECK(hipMemcpyAsync((char*)p + k * cls, a.bias, a.Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
        a.ep = (const float*)p;
    }
    return FR_OK;
}

// ------------------------------------------------------------------ an op's ConvArgs
// The ConvArgs of conv op `op` at batch B.  live: a forward is running, the activation pointers are the tensors';
// else (the load-time packer, fr_debug_plan) they are present (1) / absent flags, which is all the kinds'
// predicates read, and an e4m3 conv keeps its 16-bit description (its plan line states the 16-bit choice).
static ConvArgs conv_args(const fr_handle* h, const Op& op, int B, int f16, bool live) {
    const auto& cw = h->convw[op.wi];
    const auto& ti = h->tensors[op.in];
    const auto& to = h->tensors[op.out];
    const auto act_ptr = [&](int t) { return live ? h->tensors[t].dev : (bf16_t*)1; };
    ConvArgs a{};
    a.f16 = f16 || ti.f16;
    a.y_bf16 = ti.f16 && !to.f16;  // f16 section -> bf16 plan boundary
    a.x = act_ptr(op.in); a.B = B; a.H = ti.H; a.W = ti.W; a.Cx = ti.C; a.x_off = op.in_off; a.Cin = op.cin;
    a.w = cw.w; a.Kh = op.kh; a.Kw = op.kw; a.sh = op.sh; a.sw = op.sw; a.ph = op.ph; a.pw = op.pw;
    a.K = cw.K; a.Kpad = cw.Kpad;
    a.Ho = to.H; a.Wo = to.W; a.M = B * to.H * to.W; a.Cout = cw.Cout; a.Npad = cw.Npad;
    a.bias = cw.bias; a.slope = cw.slope; a.act = op.act; a.bias9 = cw.bias9; a.wimg = cw.wimg;
    a.negf = cw.negf; a.ep = cw.ep;
    a.wrows_ = cw.wrows; a.wring_ = cw.wring;
    if (op.res >= 0) { a.res = act_ptr(op.res); a.Cres = h->tensors[op.res].C; a.res_off = op.res_off; }
    if (op.x2 >= 0) {
        const auto& t2 = h->tensors[op.x2];
        a.x2 = act_ptr(op.x2); a.H2 = t2.H; a.W2 = t2.W; a.Cx2 = t2.C; a.x2_off = op.x2_off;
        a.C2 = cw.C2; a.st2 = op.st2; a.K1 = cw.K1;
    }
    a.y = act_ptr(op.out); a.Cy = to.C; a.y_off = op.out_off;
    if (h->amax && h->need_amax[op.out]) {
        a.y_amax = h->amax + (size_t)op.out * FR_AMAX_SLOTS;
        a.amax_slots = FR_AMAX_SLOTS;
    }
    if (live && h->amax && cw.w8 && op.in_off == 0) {
        a.w8 = cw.w8; a.wscale = cw.wscale; a.Kpad = cw.Kpad8;
        a.x_amax = h->amax + (size_t)op.in * FR_AMAX_SLOTS;
        a.amax_slots = FR_AMAX_SLOTS;  // every producer spreads its maxima over all the slots (read
                                       // them all, also when this conv records no amax itself)
    }
    return a;
}

// The packed operands of every kind that applies to a conv of the plan, packed on the device from the uploaded
// [Npad][Kpad] rows at load time (whether a kind then runs is the policy's or the tuner's decision per shape).
int pack_conv_weights(fr_handle* h) {
    const ConvAlloc persistent = [h](void** p, size_t bytes) -> int {
        const int rc = dev_alloc(p, bytes);
        if (!rc) h->weight_allocs.push_back(*p);
        return rc;
    };
    for (const auto& op : h->ops) {
        if (op.kind != OP_CONV || op.wi < 0) continue;
        DevConvW& cw = h->convw[op.wi];
        if (cw.w8) continue;  // e4m3 convs: conv_fp8.hip or the fp8 stage only
        ConvArgs a = conv_args(h, op, 1, h->dtype == FR_DTYPE_F16, false);
        for (const auto& d : conv_kinds) {
            if (!d.pack || !d.applicable(a, 1)) continue;
            const int rc = prepare(d, a, persistent, nullptr);
            if (rc) return rc;
            cw.*d.slot = const_cast<bf16_t*>(a.*d.img);
            cw.negf = const_cast<float*>(a.negf);
            cw.ep = const_cast<float*>(a.ep);
        }
    }
    FR_HIP_CHECK(hipDeviceSynchronize());
    return FR_OK;
}

// ------------------------------------------------------------------ choosing
static double conv_flops(const ConvArgs& a) { return 2.0 * (double)a.M * a.Cout * ((double)a.Cin * a.Kh * a.Kw + (a.x2 ? a.C2 : 0)); }

// Algorithmic HBM bytes of a conv launch: its input channels once (all input pixels), the projection
// input at the output's stride, the residual, the output and the weights once (activations 2 B; fp8
// weights 1 B).  Re-reads through L2 / MALL are not counted: this is the roofline's traffic floor.
static double conv_bytes(const ConvArgs& a) {
    const double act = 2.0;
    double b = (double)a.B * a.H * a.W * a.Cin * act;
    if (a.x2) b += (double)a.M * a.C2 * act;
    if (a.res) b += (double)a.M * a.Cout * act;
    b += (double)a.M * a.Cout * act * (a.y2 ? 2.0 : 1.0);
    b += (double)a.Cout * ((double)a.Cin * a.Kh * a.Kw + (a.x2 ? a.C2 : 0)) * (a.w8 ? 1.0 : 2.0);
    return b;
}

bool autotune_enabled() {
    static const bool on = [] { return ab_int("autotune", 1) != 0; }();
    return on;
}

static void shape_key(const ConvArgs& a, int* k) {
    const int v[13] = {a.M, a.Cout, a.Kpad, a.Cin, a.Kh, a.Kw, a.sh, a.sw, a.res ? 1 : 0, a.y2 ? 1 : 0, a.H, a.W, a.x2 ? 1 : 0};
    for (int i = 0; i < 13; ++i) k[i] = v[i];
}

static bool find_tuned(const fr_handle* h, const ConvArgs& a, ConvChoice* c) {
    int k[13];
    shape_key(a, k);
    for (const auto& t : h->tuned)
        if (std::memcmp(t.key, k, sizeof(k)) == 0) { *c = {t.tile, t.split}; return true; }
    return false;
}

// the split-K factor the partial workspace allows (reserve() sizes it for conv_plan's splits)
static int fit_split(const fr_handle* h, const ConvArgs& a, int split) {
    while (split > 1 && (size_t)split * a.M * a.Npad > h->partial_floats) split /= 2;
    return split;
}

// The fixed policy (no measurement: FR_AB autotune=0, a forced FR_AB conv_tile): the ranked kinds where they
// apply (each measured faster than the implicit GEMM at bs = 256), else conv_plan's cost-model tile and split.
static ConvChoice default_choice(const fr_handle* h, const ConvArgs& a) {
    ConvChoice c;
    if (h->invariant) {  // the cost model's tile, unsplit (every igemm tile sums K in the same order)
        conv_plan(a.M, a.Cout, a.Kpad, &c.tile, &c.split);
        c.split = 1;
        return c;
    }
    for (int rank = 1; const ConvKindDesc* d = ranked_kind(rank); ++rank)
        if (kind_usable(*d, a, 1)) { c.tile = d->id; return c; }
    conv_plan(a.M, a.Cout, a.Kpad, &c.tile, &c.split);
    c.split = fit_split(h, a, c.split);
    return c;
}

// Launches choice c (no timing scope; run_conv_args adds it).
static hipError_t launch_choice(fr_handle* h, ConvArgs& a, const ConvChoice& c, hipStream_t s) {
    a.split_k = 1;
    a.partial = nullptr;
    if (const ConvKindDesc* d = conv_kind(c.tile)) return d->launch(a, c.split, h->n_cu, s);
    a.tile = c.tile;
    a.splitk_cnt = nullptr;
    const int split = c.split < 0 ? -c.split : c.split;  // negative: reduced in-launch
    if (split > 1) {
        a.split_k = split;
        a.partial = h->partial;
        // in-launch: the last of each tile's split workgroups reduces (conv_igemm.hip), where the tile counters
        // fit; else the separate split-K epilogue launch
        const int64_t tiles = (int64_t)((a.M + conv_tile_bm(c.tile) - 1) / conv_tile_bm(c.tile)) *
                              ((a.Cout + conv_tile_bn(c.tile) - 1) / conv_tile_bn(c.tile));
        // (the in-launch slabs are addressed by 32-bit buffer offsets)
        if (c.split < 0 && a.y && h->splitk_cnt && tiles <= FR_SPLITK_TILES && h->splitk_inlaunch &&
            (size_t)split * a.M * a.Npad * sizeof(float) < 0x7fffffffull) {
            a.splitk_cnt = h->splitk_cnt;
            h->inlaunch_used = true;
        }
    }
    hipError_t e = launch_conv(a, s);
    if (e == hipSuccess && split > 1 && a.y && !a.splitk_cnt) e = launch_splitk_epilogue(a, s);
    return e;
}

static std::string choice_class(const ConvArgs& a, const ConvChoice& c) {
    if (const ConvKindDesc* d = conv_kind(c.tile)) return d->cls(a);
    return "conv_igemm tile" + std::to_string(c.tile) + (c.split > 1 ? " splitk" : c.split < -1 ? " splitk-inlaunch" : "");
}

// Time every usable kernel on this conv (1 warm + 3 timed launches each, three interleaved passes, the
// best time per candidate, HIP events on `s`) and remember the fastest for the shape.  Candidates: the ranked
// kinds, every implicit-GEMM tile unsplit, the other kinds (register weight ring, small-K direct, small M) and
// conv_plan's split-K plan when it splits (small M: a few tiles over a long K).  Runs
// only inside the eager tuning pass of embed_locked, so a batch size's choice is measured at that size
// (bs = 1 and bs = 256 pick differently).  Every candidate sums K in the same order except split-K, whose
// partial sums differ in f32 rounding only.
static int tune_conv(fr_handle* h, ConvArgs a, hipStream_t s) {
    std::vector<ConvChoice> cand;
    auto add = [&](int tile, int split) { cand.push_back({tile, split}); };
    const bool inv = h->invariant;  // only the kernels that sum K in the implicit GEMM's order (tile 0's bits)
    auto add_kind = [&](const ConvKindDesc& d) {
        std::vector<int> splits;
        if (d.splits) d.splits(a, splits);
        else splits.push_back(1);
        for (int sp : splits)
            if ((!inv || invariant_ok({d.id, sp})) && kind_usable(d, a, sp)) add(d.id, sp);
    };
    for (int rank = 1; const ConvKindDesc* d = ranked_kind(rank); ++rank) add_kind(*d);
    int tiles[16];
    const int nt = conv_tile_candidates(a.Cout, tiles);
    for (int i = 0; i < nt; ++i) add(tiles[i], 1);
    for (const auto& d : conv_kinds)
        if (!d.rank) add_kind(d);
    {
        int tile, split;
        conv_plan(a.M, a.Cout, a.Kpad, &tile, &split);
        split = fit_split(h, a, split);
        if (split > 1 && !inv) {
            add(tile, split);
            if (h->splitk_inlaunch) add(tile, -split);  // the same split reduced in-launch (negative split)
        }
    }
    hipEvent_t e0, e1;
    FR_HIP_CHECK(hipEventCreate(&e0));
    FR_HIP_CHECK(hipEventCreate(&e1));
    // three interleaved passes, best time per candidate: one pass in candidate order let clock ramps
    // and neighbours' cache state pick different tiles from run to run (profiles/r01_bench_runs.jsonl)
    std::vector<float> cand_ms(cand.size(), 1e30f);
    for (int pass = 0; pass < 3; ++pass) {
        for (size_t c = 0; c < cand.size(); ++c) {
            if (cand_ms[c] < 0.f) continue;  // failed to launch (a library candidate without an algorithm)
            if (launch_choice(h, a, cand[c], s) != hipSuccess) {
                (void)hipGetLastError();
                cand_ms[c] = -1.f;
                continue;
            }
            FR_HIP_CHECK(hipEventRecord(e0, s));
            for (int r = 0; r < 3; ++r) FR_HIP_CHECK(launch_choice(h, a, cand[c], s));
            FR_HIP_CHECK(hipEventRecord(e1, s));
            FR_HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            FR_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            cand_ms[c] = std::min(cand_ms[c], ms);
        }
    }
    // the 3-stage implicit-GEMM tiles are credited FR_AB tune_s3_bias percent (default 5): the tuner's
    // back-to-back launches run warm, where the deeper ring's latency hiding does not show, and in the
    // forward they win (IRV1 Block17 1x7: 12.0 vs 17.4 us per launch for 11.5 vs 11.5 us tuned)
    static const float s3_credit = 1.f - 0.01f * (float)ab_int("tune_s3_bias", 5);  // (the 64x64 3-stage tile too)
    for (size_t c = 0; c < cand.size(); ++c)
        if (cand_ms[c] >= 0.f && (cand[c].tile == TILE_128x64_S3 || cand[c].tile == TILE_64x128_S3 || cand[c].tile == TILE_64x64_S3 ||
                                  cand[c].tile == TILE_32x64_S3) &&
            cand[c].split == 1)
            cand_ms[c] *= s3_credit;
    size_t best = 0;
    while (best + 1 < cand.size() && cand_ms[best] < 0.f) ++best;
    for (size_t c = best + 1; c < cand.size(); ++c)
        if (cand_ms[c] >= 0.f && cand_ms[c] < cand_ms[best] * 0.99f) best = c;
    static const bool tune_log = ab_int("tune_log", 0) != 0;  // FR_AB tune_log=1: candidate times to stderr
    if (tune_log) {
        fprintf(stderr, "tune M=%d N=%d K=%d %dx%d:", a.M, a.Cout, a.Kpad, a.Kh, a.Kw);
        for (size_t c = 0; c < cand.size(); ++c)
            fprintf(stderr, " %d/%d=%.1f%s", cand[c].tile, cand[c].split, cand_ms[c] * 1000.f / 3.f, c == best ? "*" : "");
        fprintf(stderr, "\n");
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    fr_handle::Tuned t{{}, cand[best].tile, cand[best].split};
    shape_key(a, t.key);
    h->tuned.push_back(t);
    return FR_OK;
}

// The kernel choice of a conv launch: the measured one for its shape (tuned in the eager tuning forward of
// the batch size) while it still applies, else the fixed policy.
static ConvChoice conv_choice(const fr_handle* h, const ConvArgs& a) {
    ConvChoice c;
    if (autotune_enabled() && !conv_tile_forced() && find_tuned(h, a, &c) && (!h->invariant || invariant_ok(c))) {
        const ConvKindDesc* d = conv_kind(c.tile);
        if (d ? kind_usable(*d, a, c.split) : c.tile >= 0) return c;
    }
    return default_choice(h, a);
}

// A conv launch inside its timing scope: the e4m3 kernel for an fp8 conv, else the chosen kernel (tuned first in
// the tuning forward).
static int run_conv_args(fr_handle* h, ConvArgs& a, hipStream_t s) {
    ProfScope ps(h, s);
    ps.flops = conv_flops(a);
    ps.bytes = conv_bytes(a);
    if (a.w8) {  // FR_DTYPE_FP8 conv (conv_fp8.hip)
        a.tile = conv_fp8_tile(a.M, a.Cout);
        a.split_k = 1;
        ps.start("conv_fp8 tile" + std::to_string(a.tile), &a);
        FR_HIP_CHECK(launch_conv_fp8(a, s));
        return FR_OK;
    }
    ConvChoice c;
    if (autotune_enabled() && !conv_tile_forced() && !find_tuned(h, a, &c) && h->tuning) {
        const int rc = tune_conv(h, a, s);
        if (rc) return rc;
    }
    c = conv_choice(h, a);
    ps.start(choice_class(a, c), &a);  // the event pair rides on the launched args
    FR_HIP_CHECK(launch_choice(h, a, c, s));
    return FR_OK;
}

int run_conv_op(fr_handle* h, const Op& op, int B, int f16, hipStream_t s) {
    ConvArgs a = conv_args(h, op, B, f16, true);
    return run_conv_args(h, a, s);
}

// ------------------------------------------------------------------ the op API (fr_op_conv2d_ex)
bool op_tile_is_igemm(int tile) { return tile == 0 || (!conv_kind(tile - 1) && igemm_tile_valid(tile - 1)); }

int op_tile_takes(int tile) {
    if (op_tile_is_igemm(tile)) return CONV_TAKES_X2 | CONV_TAKES_Y_BF16 | CONV_TAKES_SPLITK_CNT;
    const ConvKindDesc* d = conv_kind(tile - 1);
    return d ? d->takes : 0;
}

std::string conv_takers(int field) {
    std::string out = "the implicit-GEMM tiles";
    for (const auto& d : conv_kinds)
        if (d.takes & field) out += std::string(", ") + d.name;
    return out;
}

bool op_tile_forced_kind(int tile) { return conv_kind(tile - 1) != nullptr; }

// The kind that descriptor tile id `tile` claims, on the caller's [Npad][Kpad] rows: its packed operands go into
// scratch on every call (no cache keyed on the caller's weight pointer: new weights in the same buffer are always
// repacked), stream-ordered unless the kind's row says otherwise.
int run_forced_kind(int tile, ConvArgs& a, int split, hipStream_t s) {
    const ConvKindDesc& d = *conv_kind(tile - 1);
    if (!d.applicable(a, split)) {
        set_error(std::string("fr_op_conv2d: ") + d.name + " kernel not applicable");
        return FR_ERR_ARG;
    }
    std::vector<void*> scratch;
    const bool sync = d.op_sync;
    const ConvAlloc alloc = [&](void** p, size_t bytes) -> int {
        FR_HIP_CHECK(sync ? hipMalloc(p, bytes) : hipMallocAsync(p, bytes, s));
        scratch.push_back(*p);
        return FR_OK;
    };
    if (sync) FR_HIP_CHECK(hipStreamSynchronize(s));
    int rc = d.pack ? prepare(d, a, alloc, s) : FR_OK;
    if (!rc) {
        const hipError_t e = d.launch(a, split, 0, s);  // n_cu 0: no handle, the kind asks the device
        if (e != hipSuccess) {
            set_error(std::string("fr_op_conv2d: ") + d.name + " kernel: " + hipGetErrorString(e));
            rc = FR_ERR_HIP;
        }
    }
    if (sync) (void)hipStreamSynchronize(s);
    for (void* p : scratch) (void)(sync ? hipFree(p) : hipFreeAsync(p, s));
    return rc;
}

// ------------------------------------------------------------------ fr_debug_plan
// "conv|head M N K Kpad tile split KhxKw <output>": the measured kernel (after a forward at B), else the policy
std::string conv_plan_line(const fr_handle* h, const Op& op, int B) {
    const auto& cw = h->convw[op.wi];
    const bool head = op.kind == OP_HEAD;
    const int M = head ? B : B * h->tensors[op.out].H * h->tensors[op.out].W;
    ConvChoice c;
    if (head) head_plan(M, cw.Cout, cw.Kpad, &c.tile, &c.split);
    else c = conv_choice(h, conv_args(h, op, B, h->dtype == FR_DTYPE_F16, false));
    const std::string nm = head ? "head" : h->tensors[op.out].name;
    return (head ? "head " : "conv ") + std::to_string(M) + " " + std::to_string(cw.Cout) + " " + std::to_string(cw.K) +
           " " + std::to_string(cw.Kpad) + " " + std::to_string(c.tile) + " " + std::to_string(c.split) + " " +
           std::to_string(op.kh) + "x" + std::to_string(op.kw) + " " + (nm.empty() ? "-" : nm) + "\n";
}

}  // namespace fr
