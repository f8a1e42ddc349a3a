// frhip engine: the C-ABI handle, its activation memory and the forward that runs a handle's plan.  See
// include/frhip.h for the boundary contract and DESIGN.md for the data layout.  What the networks are (the weight-blob
// parser and the per-arch plan builders) is in plan.cpp, the fused stages of a plan (their kinds, packers, launches) in
// stages.cpp, how a conv gets its kernel (the conv kernel kinds, the tuner, the op API's forced kernels) in convs.cpp,
// the gallery and matcher entry points in gallery_api.cpp, the stateless op entry points in ops_api.cpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "engine_internal.h"

namespace fr {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }

// A/B and debugging switches, all in one environment variable read once per process:
//   FR_AB="no_trans,no_wring,stage_variant=1,head_plan=8:14"  (a bare key = 1; DESIGN.md §7 lists the keys)
static const std::vector<std::pair<std::string, std::string>>& ab_table() {
    static const std::vector<std::pair<std::string, std::string>> t = [] {
        std::vector<std::pair<std::string, std::string>> r;
        const char* e = getenv("FR_AB");
        const std::string v = e ? e : "";
        size_t p = 0;
        while (p < v.size()) {
            size_t q = v.find(',', p);
            if (q == std::string::npos) q = v.size();
            const std::string tok = v.substr(p, q - p);
            const size_t eq = tok.find('=');
            if (!tok.empty()) r.emplace_back(tok.substr(0, eq), eq == std::string::npos ? "1" : tok.substr(eq + 1));
            p = q + 1;
        }
        return r;
    }();
    return t;
}
const char* ab_str(const char* key) {
    for (const auto& kv : ab_table())
        if (kv.first == key) return kv.second.c_str();
    return nullptr;
}
int ab_int(const char* key, int dflt) {
    const char* v = ab_str(key);
    return v ? atoi(v) : dflt;
}

hipError_t lds_opt_in(const void* kernel, int bytes) {
    struct Grant { const void* kernel; int device, bytes; };
    static std::mutex mu;
    static std::vector<Grant> grants;  // a few dozen entries: one per kernel instantiation that ran, per device
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    auto g = std::find_if(grants.begin(), grants.end(), [&](const Grant& x) { return x.kernel == kernel && x.device == device; });
    if (g != grants.end() && g->bytes >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    if (g != grants.end()) g->bytes = bytes;
    else grants.push_back({kernel, device, bytes});
    return hipSuccess;
}

int dev_alloc(void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        set_error(std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? FR_ERR_OOM : FR_ERR_HIP;
    }
    return FR_OK;
}
}  // namespace fr

using namespace fr;

namespace {

constexpr size_t FR_MAX_SPLIT_STAGES = 6;  // stage ops per plan (at most one per residual layer + the transition)

void drop_graphs(fr_handle* h) {
    if (h->graphs.empty()) return;
    (void)hipDeviceSynchronize();  // no exec may be destroyed while a replay of it is in flight
    for (auto& g : h->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->graphs.clear();
}

void free_acts(fr_handle* h) {
    drop_graphs(h);
    for (void* p : h->act_allocs) (void)hipFree(p);
    h->act_allocs.clear();
    h->stage_xchg = nullptr;
    h->stage_flags = nullptr;
    for (auto& t : h->tensors) t.dev = nullptr;
    h->partial = nullptr;
    h->partial_floats = 0;
    h->splitk_cnt = nullptr;
    h->emb_pre = nullptr;
    h->amax = nullptr;
    h->ex_g = h->ex_v = h->ex_emb = nullptr;
    h->max_batch = 0;
}

void free_weights(fr_handle* h) {
    drop_graphs(h);
    for (void* p : h->weight_allocs) (void)hipFree(p);
    h->weight_allocs.clear();
    h->convw.clear();
    h->stages.clear();
    h->proj_w = h->proj_b = nullptr;
    h->proj_d = 0;
}

// ------------------------------------------------------------------ execution
size_t partial_need(fr_handle* h, int B) {
    size_t need = 0;
    for (const auto& op : h->ops) {
        if (op.kind != OP_CONV && op.kind != OP_HEAD) continue;
        const auto& cw = h->convw[op.wi];
        const int M = op.kind == OP_HEAD ? B : B * h->tensors[op.out].H * h->tensors[op.out].W;
        int tile, sp;
        if (op.kind == OP_HEAD) head_plan(M, cw.Cout, cw.Kpad, &tile, &sp);
        else conv_plan(M, cw.Cout, cw.Kpad, &tile, &sp);
        if (sp > 1 || op.kind == OP_HEAD) need = std::max(need, (size_t)sp * M * cw.Npad);
        if (op.kind == OP_HEAD) {  // FR_OPT_BATCH_INVARIANT runs bs = 256's head split at every batch
            head_plan(256, cw.Cout, cw.Kpad, &tile, &sp);
            need = std::max(need, (size_t)sp * M * cw.Npad);
        }
    }
    return need;
}

int reserve(fr_handle* h, int maxB) {
    if (maxB <= h->max_batch) return FR_OK;
    free_acts(h);
    for (auto& t : h->tensors) {
        void* p = nullptr;
        int rc = dev_alloc(&p, (size_t)maxB * t.H * t.W * t.C * sizeof(bf16_t));
        if (rc) { free_acts(h); return rc; }
        h->act_allocs.push_back(p);
        t.dev = (bf16_t*)p;
    }
    size_t need = partial_need(h, maxB);
    for (int b = 1; b < maxB; b *= 2) need = std::max(need, partial_need(h, b));
    void* p = nullptr;
    int rc = dev_alloc(&p, need * sizeof(float));
    if (rc) { free_acts(h); return rc; }
    h->act_allocs.push_back(p);
    h->partial = (float*)p;
    h->partial_floats = need;
    {
        void* q = nullptr;
        if ((rc = dev_alloc(&q, FR_SPLITK_TILES * sizeof(int)))) { free_acts(h); return rc; }
        h->act_allocs.push_back(q);
        FR_HIP_CHECK(hipMemset(q, 0, FR_SPLITK_TILES * sizeof(int)));
        h->splitk_cnt = (int*)q;
    }
    h->max_batch = maxB;
    if (std::any_of(h->need_amax.begin(), h->need_amax.end(), [](char c) { return c != 0; })) {
        void* q = nullptr;
        rc = dev_alloc(&q, h->tensors.size() * FR_AMAX_SLOTS * sizeof(float));
        if (rc) { free_acts(h); return rc; }
        h->act_allocs.push_back(q);
        h->amax = (float*)q;
    }
    if (h->proj_d) {
        void* q = nullptr;
        rc = dev_alloc(&q, (size_t)maxB * h->embed_dim * sizeof(float));
        if (rc) { free_acts(h); return rc; }
        h->act_allocs.push_back(q);
        h->emb_pre = (float*)q;
    }
    if (h->ex_tensor >= 0) {  // fr_explain's scratch (the gradient buffers only where a gradient is taken)
        const DevConvW& hw = h->convw[h->ops.back().wi];  // the head is every plan's last op
        const size_t D = (size_t)(h->proj_d ? h->proj_d : h->embed_dim);
        float** dst[3] = {&h->ex_emb, &h->ex_g, &h->ex_v};
        const size_t n[3] = {maxB * D, h->ex_layout == 2 ? 0 : maxB * (size_t)hw.Cout,
                             h->ex_layout == 2 ? 0 : maxB * (size_t)hw.Kpad};
        for (int i = 0; i < 3; ++i) {
            if (!n[i]) continue;
            void* q = nullptr;
            rc = dev_alloc(&q, n[i] * sizeof(float));
            if (rc) { free_acts(h); return rc; }
            h->act_allocs.push_back(q);
            *dst[i] = (float*)q;
        }
    }
    if (std::any_of(h->stages.begin(), h->stages.end(), [](const StageRec& r) { return r.parts > 1; })) {
        if (h->stages.size() > FR_MAX_SPLIT_STAGES) { set_error("reserve: too many stage ops"); return FR_ERR_ARG; }
        void* q = nullptr;
        rc = dev_alloc(&q, split_stage_xchg_elems(maxB) * sizeof(bf16_t));
        if (rc) { free_acts(h); return rc; }
        h->act_allocs.push_back(q);
        h->stage_xchg = (bf16_t*)q;
        // one counter region per split stage ([maxB][4] each: the counters run on across launches, so
        // two stages with different part counts must not share slots); zeroed once here
        rc = dev_alloc(&q, (size_t)maxB * 4 * FR_MAX_SPLIT_STAGES * sizeof(int));
        if (rc) { free_acts(h); return rc; }
        h->act_allocs.push_back(q);
        FR_HIP_CHECK(hipMemset(q, 0, (size_t)maxB * 4 * FR_MAX_SPLIT_STAGES * sizeof(int)));
        h->stage_flags = (int*)q;
    }
    return fill_stage_dbg(h);
}

bool stem_fuse_enabled() {
    static const bool on = [] { return !ab_int("no_stem_fuse", 0); }();
    return on;
}

// Co-residency of a split stage's parts holds while the stage kernel is the only long-running kernel
// on the device.  Two split-stage forwards of different handles on one device could
// each hold CUs the other's parts need, so the forwards of handles that share a device (in this
// process) are chained on the GPU: each waits for the previous one's completion event and records its
// own.  Handles alone on their device pay nothing.  (Other processes on the same device are not seen:
// their kernels can only delay a wait, which the bounded wait and fr_embed's check then report.)
// The chain lock is per device (handles on other devices never wait for it); the registry lock only guards
// the per-device table and is held for a lookup.
struct DevSerial {
    struct Dev {
        std::mutex chain;       // held from the wait on `last` until `last` is re-recorded
        int count = 0;          // handles on the device with split stages
        hipEvent_t last = nullptr;
    };
    static std::mutex& reg_mu() { static std::mutex m; return m; }
    static Dev& dev(int d) {
        static std::unordered_map<int, std::unique_ptr<Dev>> m;  // entries are never erased: stable references
        std::lock_guard<std::mutex> lk(reg_mu());
        auto& p = m[d];
        if (!p) p.reset(new Dev());
        return *p;
    }
    static void reg(fr_handle* h, bool on) {
        Dev& d = dev(h->device);
        std::lock_guard<std::mutex> lk(reg_mu());
        if (on == h->split_registered) return;
        h->split_registered = on;
        d.count += on ? 1 : -1;
    }
    std::unique_lock<std::mutex> lk;
    hipEvent_t ev = nullptr;
    hipStream_t s = nullptr;
    DevSerial(fr_handle* h, bool split, hipStream_t s_) : s(s_) {
        if (!split) return;
        Dev& d = dev(h->device);
        {
            std::lock_guard<std::mutex> rl(reg_mu());
            if (d.count <= 1) return;
        }
        lk = std::unique_lock<std::mutex>(d.chain);
        hipEvent_t& e = d.last;
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
        ev = e;
        if (ev) (void)hipStreamWaitEvent(s, ev, 0);
    }
    void done() {
        if (ev) (void)hipEventRecord(ev, s);
        ev = nullptr;
        if (lk.owns_lock()) lk.unlock();
    }
    ~DevSerial() { done(); }
};

// Branch-parallel scheduling of a captured forward (h->ms_on, set by forward_graph; opt-in, see ms_enabled): a conv or max-pool
// that does not depend on the last op of the main stream goes to a second stream, with an event wait for
// each dependency on the other stream; every other op kind joins both streams.  Dependencies come from
// the channel ranges each op reads and writes (RAW / WAR / WAW), the split-K partials counting as one
// shared range.  In the captured graph these become edges: IRV1's Inception branches (Block35's 3x3 paths,
// mixed_6a / mixed_7a) and ResNet-50's downsample projections run concurrently.
namespace {
struct Rgn {
    int t, lo, hi;
};
constexpr int RGN_ALL = -3;  // the range of a joining op: overlaps everything
bool rgn_hit(const std::vector<Rgn>& a, const std::vector<Rgn>& b) {
    for (const auto& x : a)
        for (const auto& y : b)
            if (x.t == RGN_ALL || y.t == RGN_ALL || (x.t == y.t && x.lo < y.hi && y.lo < x.hi)) return true;
    return false;
}
}  // namespace

// Opt-in (FR_BRANCH_STREAMS=1, read at each capture): measured slower on IRV1 (104.2k vs 107.0k faces/s,
// 3 same-box pairs) and ResNet-50 (157.0-157.9k vs 157.8-158.5k): the branches' kernels size their grids
// for the whole GPU (persistent conv_direct / conv_rows, full igemm tile grids), so two of them at once
// share the CUs instead of filling idle ones.
// FR_AB no_head_gemv: the small-batch head runs on the implicit-GEMM tiles too (A/B timing)
static bool head_gemv_enabled() {
    static const bool on = [] { return !ab_int("no_head_gemv", 0); }();
    return on;
}

static bool ms_enabled() {
    const char* e = getenv("FR_BRANCH_STREAMS");
    return e && e[0] == '1';
}

}  // namespace

// (shared with stages.cpp: a stage's member ops run beside it when it is measured)
int fr::run_maxpool_op(fr_handle* h, const Op& op, int B, int f16, hipStream_t s) {
    ProfScope ps(h, s);
    ps.start("maxpool");
    const auto& ti = h->tensors[op.in];
    const auto& to = h->tensors[op.out];
    if (!ti.f16 && to.f16) {
        set_error("plan: maxpool from a bf16 tensor into an f16 section");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_maxpool(ti.dev, B, ti.H, ti.W, ti.C, 0, ti.C, op.pk, op.ps, op.pp, to.dev, to.C, op.out_off, to.H,
                                to.W, f16 || ti.f16, s, ti.f16 && !to.f16 ? 1 : 0));
    return FR_OK;
}

namespace {

int forward(fr_handle* h, const void* in, int in_fmt, int B, float* out, int flags, hipStream_t s_main) {
    const int f16 = h->dtype == FR_DTYPE_F16;
    const std::vector<char> stage_run = stage_plan(h, B);
    if (h->amax) FR_HIP_CHECK(hipMemsetAsync(h->amax, 0, h->tensors.size() * FR_AMAX_SLOTS * sizeof(float), s_main));
    // the split-K tile counters return to zero after every launch; re-zeroed per forward all the same (once an
    // in-launch split has run on this handle: zeroed at fr_reserve before that), so an aborted earlier launch
    // cannot leave a count behind.  The memset node is ~6 us of a 1 ms bs = 1 forward that may have no such split.
    if (h->splitk_cnt && h->inlaunch_used) FR_HIP_CHECK(hipMemsetAsync(h->splitk_cnt, 0, FR_SPLITK_TILES * sizeof(int), s_main));
    h->slot_done = false;
    h->slot_seen = 0;
    const bool ms = h->ms_on;
    const size_t nops = h->ops.size();
    std::vector<std::vector<Rgn>> rd, wr;
    std::vector<int> on_stream;
    int tail[2] = {-1, -1};      // last op launched on each stream
    int joined_aux = -1;         // last aux op the main stream has waited for
    hipStream_t strm[2] = {s_main, h->aux_stream};
    if (ms) {
        rd.resize(nops);
        wr.resize(nops);
        on_stream.assign(nops, -1);
        while (h->op_events.size() < nops + 1) {
            hipEvent_t e;
            FR_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->op_events.push_back(e);
        }
        // fork: the aux stream joins the capture behind everything issued so far
        FR_HIP_CHECK(hipEventRecord(h->op_events[nops], s_main));
        FR_HIP_CHECK(hipStreamWaitEvent(strm[1], h->op_events[nops], 0));
    }
    bool skip_next = false;
    for (size_t oi = 0; oi < h->ops.size(); ++oi) {
        const Op& op = h->ops[oi];
        if (skip_next) { skip_next = false; continue; }
        if (op_skipped(op, stage_run)) continue;
        int target = 0;
        if (ms) {
            // the op's ranges
            bool branchable = false;
            if (op.kind == OP_CONV && op.wi >= 0) {
                const auto& cw = h->convw[op.wi];
                rd[oi].push_back({op.in, op.in_off, op.in_off + op.cin});
                if (op.res >= 0) rd[oi].push_back({op.res, op.res_off, op.res_off + cw.Cout});
                if (op.x2 >= 0) rd[oi].push_back({op.x2, op.x2_off, op.x2_off + cw.C2});
                wr[oi].push_back({op.out, op.out_off, op.out_off + cw.Cout});
                int tile, split;
                const auto& to = h->tensors[op.out];
                conv_plan(B * to.H * to.W, cw.Cout, cw.Kpad, &tile, &split);
                if (split > 1) wr[oi].push_back({-2, 0, 1});  // the shared split-K partials
                branchable = true;
            } else if (op.kind == OP_MAXPOOL) {
                rd[oi].push_back({op.in, 0, h->tensors[op.in].C});
                wr[oi].push_back({op.out, op.out_off, op.out_off + h->tensors[op.in].C});
                branchable = true;
            }
            if (!branchable) wr[oi].push_back({RGN_ALL, 0, 1});  // joins both streams, runs on main
            auto dep = [&](int j) {
                return j >= 0 && (rgn_hit(rd[oi], wr[j]) || rgn_hit(wr[oi], rd[j]) || rgn_hit(wr[oi], wr[j]));
            };
            // main if it depends on main's last op (or is a joining op), else the second stream
            target = !branchable || tail[0] < 0 || dep(tail[0]) ? 0 : 1;
            // wait for the latest dependency on the other stream (stream order covers the earlier ones)
            const int other = 1 - target;
            for (int j = (int)oi - 1; j >= 0; --j)
                if (on_stream[j] == other && dep(j)) {
                    if (!(target == 0 && j <= joined_aux)) FR_HIP_CHECK(hipStreamWaitEvent(strm[target], h->op_events[j], 0));
                    if (target == 0 && j > joined_aux) joined_aux = j;
                    break;
                }
        }
        const hipStream_t s = strm[target];
        switch (op.kind) {
            case OP_STAGE: {
                const bool measure = h->tuning && h->stage_mode == 1 && !h->keep_inter && !h->prof &&
                                     stage_choice(h, op.grp, B) < 0;
                const int rc = measure ? measure_stage(h, op, B, f16, stage_run, s) : run_stage(h, op, B, f16, stage_run, s);
                if (rc) return rc;
                break;
            }
            case OP_PRE: {
                h->fwd_u8 = nullptr;
                if (in_fmt == FR_IN_U8_NHWC && oi + 1 < h->ops.size() && h->ops[oi + 1].kind == OP_STAGE &&
                    stage_takes_u8(h->stages[h->ops[oi + 1].stage]) &&
                    !op_skipped(h->ops[oi + 1], stage_run) &&
                    !(h->tuning && h->stage_mode == 1 && !h->keep_inter && !h->prof &&
                      stage_choice(h, h->ops[oi + 1].grp, B) < 0)) {
                    h->fwd_u8 = (const uint8_t*)in;  // conv_stem160 / conv_stem_r50 prepare the crops themselves
                    break;
                }
                ProfScope ps(h, s);
                // u8 crops: preprocess + stem conv in one launch (conv_stem.hip).  Not when an e4m3 conv
                // reads the stem output (it needs the amax from the conv epilogue).
                if (op.fuse_stem && in_fmt == FR_IN_U8_NHWC && stem_fuse_enabled() && oi + 1 < h->ops.size() &&
                    h->ops[oi + 1].kind == OP_CONV && !(h->amax && h->need_amax[h->ops[oi + 1].out])) {
                    const Op& cv = h->ops[oi + 1];
                    const auto& cw = h->convw[cv.wi];
                    const auto& to = h->tensors[cv.out];
                    if (stem_u8_supported(to.H, to.W, cv.cin, cw.K, cw.Kpad, cw.Cout, to.C, cv.out_off) && !cw.bias9 &&
                        cv.res < 0 && cv.sh == 1 && cv.ph == 1 && cv.kh == 3 && cv.kw == 3) {
                        ps.flops = 2.0 * B * to.H * to.W * cw.Cout * 27.0;
                        ps.bytes = (double)B * to.H * to.W * (3.0 + cw.Cout * 2.0);
                        ps.start("stem u8 fused");
                        FR_HIP_CHECK(launch_stem_u8((const uint8_t*)in, B, cw.w, cw.Kpad, cw.bias, cw.slope, cv.act,
                                                    to.dev, to.C, cv.out_off, f16, s));
                        skip_next = true;
                        break;
                    }
                }
                ps.start("preprocess");
                const auto& t = h->tensors[op.out];
                FR_HIP_CHECK(launch_preprocess(in, in_fmt, B, t.H, t.W, t.dev, f16 || t.f16, s));
                break;
            }
            case OP_CONV: {
                const int rc = run_conv_op(h, op, B, f16, s);
                if (rc) return rc;
                break;
            }
            case OP_MAXPOOL: {
                const int rc = run_maxpool_op(h, op, B, f16, s);
                if (rc) return rc;
                break;
            }
            case OP_AVGPOOL: {
                ProfScope ps(h, s);
                ps.start("avgpool");
                const auto& ti = h->tensors[op.in];
                FR_HIP_CHECK(launch_avgpool(ti.dev, B, ti.H, ti.W, ti.C, h->tensors[op.out].dev, f16, s));
                break;
            }
            case OP_HEAD: {
                ProfScope ps(h, s);
                ps.start("head");
                const auto& cw = h->convw[op.wi];
                const auto& ti = h->tensors[op.in];
                ps.flops = 2.0 * B * cw.Cout * (double)cw.K;
                ConvArgs a{};
                a.f16 = f16;
                a.x = ti.dev; a.B = B; a.H = 1; a.W = 1; a.Cx = cw.K; a.x_off = 0; a.Cin = cw.K;
                a.w = cw.w; a.Kh = 1; a.Kw = 1; a.sh = 1; a.sw = 1; a.K = cw.K; a.Kpad = cw.Kpad;
                a.Ho = 1; a.Wo = 1; a.M = B; a.Cout = cw.Cout; a.Npad = cw.Npad;
                int tile, split;
                // batch-invariant: bs = 256's plan at every batch (reserve() sizes the partials for it)
                head_plan(h->invariant ? 256 : B, cw.Cout, cw.Kpad, &tile, &split);
                while (split > 1 && (size_t)split * B * cw.Npad > h->partial_floats) split /= 2;
                // B <= 4 (the online bs = 1 path): a GEMV over 8 K chunks instead of 128-row MFMA tiles
                const bool gemv = B <= 4 && !h->invariant && head_gemv_enabled() &&
                                  head_gemv_supported(B, cw.K, cw.Kpad, cw.Npad) && (size_t)8 * B * cw.Npad <= h->partial_floats;
                if (gemv) split = 8;
                a.tile = tile;
                a.split_k = split;
                a.partial = h->partial;
                // input, weights, the f32 split-K partials written and read back, the f32 embeddings
                ps.bytes = (double)B * cw.K * 2.0 + (double)cw.K * cw.Cout * 2.0 + 2.0 * split * B * cw.Npad * 4.0 +
                           (double)B * cw.Cout * 4.0;
                if (gemv)
                    FR_HIP_CHECK(launch_head_gemv(ti.dev, B, cw.K, cw.w, cw.Kpad, cw.Cout, cw.Npad, split, f16 || ti.f16,
                                                  h->partial, s));
                else
                    FR_HIP_CHECK(launch_conv(a, s));
                if (h->proj_d) {  // IRV1 L2 (always: InceptionResnetV1 classify=False) -> projection -> L2
                    FR_HIP_CHECK(launch_head_finalize(h->partial, split, B, cw.Cout, cw.Npad, cw.bias, 1, h->emb_pre, s));
                    FR_HIP_CHECK(launch_proj_l2(h->emb_pre, B, cw.Cout, h->proj_w, h->proj_b, h->proj_d,
                                                (flags & FR_EMBED_RAW) ? 0 : 1, out, s));
                } else {
                    FR_HIP_CHECK(launch_head_finalize(h->partial, split, B, cw.Cout, cw.Npad, cw.bias,
                                                      (flags & FR_EMBED_RAW) ? 0 : 1, out, s));
                }
                break;
            }
        }
        if (ms) {
            FR_HIP_CHECK(hipEventRecord(h->op_events[oi], s));
            on_stream[oi] = target;
            tail[target] = (int)oi;
            if (skip_next) on_stream[oi + 1] = -1;  // the fused stem ran the next op (a joining op: covers it)
        }
    }
    if (ms && tail[1] > joined_aux) FR_HIP_CHECK(hipStreamWaitEvent(strm[0], h->op_events[tail[1]], 0));  // join
    return FR_OK;
}

bool valid_arch(int a) { return a == FR_ARCH_RESNET50_ARCFACE || a == FR_ARCH_IRESNET100 || a == FR_ARCH_IRV1_FACENET; }

}  // namespace

// ==================================================================== C ABI
extern "C" {

const char* fr_last_error(void) { return g_err.c_str(); }
int fr_abi_version(void) { return FR_ABI_VERSION; }

static int stage_default() { return ab_int("no_stage", 0) ? 0 : 1; }

int fr_create(fr_handle** out, int device, int arch, int dtype) {
    if (!out || !valid_arch(arch) || (dtype != FR_DTYPE_BF16 && dtype != FR_DTYPE_F16 && dtype != FR_DTYPE_FP8)) {
        set_error("fr_create: bad argument (arch/dtype)");
        return FR_ERR_ARG;
    }
    int n = 0;
    FR_HIP_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) {
        set_error("fr_create: device " + std::to_string(device) + " out of range (" + std::to_string(n) + ")");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(hipSetDevice(device));
    auto* h = new fr_handle();
    h->device = device;
    h->arch = arch;
    h->dtype = dtype;
    h->in_size = arch == FR_ARCH_IRV1_FACENET ? 160 : 112;
    h->stage_mode = stage_default();
    h->splitk_inlaunch = ab_int("splitk_inlaunch", 1) != 0;  // A/B timing
    {
        const int v = ab_int("stage_variant", 0);  // A/B timing
        h->stage_variant = v >= 1 && v <= 3 ? v : 0;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        h->n_cu = prop.multiProcessorCount;
    void* fh = nullptr;
    if (hipHostMalloc(&fh, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->fail_dev, fh, 0) != hipSuccess ||
        hipEventCreateWithFlags(&h->chk_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->async_ev, hipEventDisableTiming) != hipSuccess) {
        if (fh) (void)hipHostFree(fh);
        if (h->chk_ev) (void)hipEventDestroy(h->chk_ev);
        set_error("fr_create: host-mapped status word / event allocation failed");
        delete h;
        return FR_ERR_HIP;
    }
    h->fail_host = (int*)fh;
    *(volatile int*)h->fail_host = 0;
    *out = h;
    return FR_OK;
}

void fr_destroy(fr_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    free_acts(h);
    free_weights(h);
    if (h->gallery) (void)hipFree(h->gallery);
    if (h->g_hi) (void)hipFree(h->g_hi);
    if (h->match_fb) (void)hipFree(h->match_fb);
    if (h->cand_s) (void)hipFree(h->cand_s);
    if (h->cand_i) (void)hipFree(h->cand_i);
    drop_graphs(h);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    for (auto& pr : h->slot_events) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    for (auto e : h->op_events) (void)hipEventDestroy(e);
    for (auto& r : h->prof_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : h->ev_free) (void)hipEventDestroy(e);
    DevSerial::reg(h, false);
    if (h->chk_ev) (void)hipEventDestroy(h->chk_ev);
    if (h->async_ev) (void)hipEventDestroy(h->async_ev);
    if (h->fail_host) (void)hipHostFree(h->fail_host);
    delete h;
}

int fr_load_weights(fr_handle* h, const void* blob, size_t nbytes) {
    if (!h || !blob) { set_error("fr_load_weights: null argument"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    FR_HIP_CHECK(hipSetDevice(h->device));
    Blob W;
    int rc = parse_blob(blob, nbytes, W);
    if (rc) return rc;
    const int keep_batch = h->max_batch;
    free_acts(h);
    free_weights(h);
    h->tensors.clear();
    h->ops.clear();
    h->loaded = false;
    h->ex_tensor = h->ex_conv = -1;
    h->cut_l4in = -1;
    rc = build_plan(h, W);
    if (!rc) rc = pack_conv_weights(h);
    for (auto& op : h->ops) op.grp = op.stage;  // plan entries (stage_plan)
    // the tensors whose producers record amax: inputs of e4m3 convs that run per-conv (an fp8 stage
    // scales its own input; its member convs are its fallback when the stage does not run)
    h->need_amax.assign(h->tensors.size(), 0);
    for (const auto& op : h->ops)
        if (op.kind == OP_CONV && op.wi >= 0 && h->convw[op.wi].w8 && op.in_off == 0) h->need_amax[op.in] = 1;
    if (rc) {
        free_weights(h);
        h->tensors.clear();
        h->ops.clear();
        DevSerial::reg(h, false);
        return rc;
    }
    h->loaded = true;
    DevSerial::reg(h, std::any_of(h->stages.begin(), h->stages.end(), [](const StageRec& r) { return r.parts > 1; }));
    if (keep_batch > 0) return reserve(h, keep_batch);
    return FR_OK;
}

int fr_reserve(fr_handle* h, int max_batch) {
    if (!h || max_batch <= 0) { set_error("fr_reserve: bad argument"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->loaded) { set_error("fr_reserve: weights not loaded"); return FR_ERR_STATE; }
    FR_HIP_CHECK(hipSetDevice(h->device));
    return reserve(h, max_batch);
}

int fr_embed_dim(const fr_handle* h) { return h ? (h->proj_d ? h->proj_d : h->embed_dim) : 0; }
int fr_input_size(const fr_handle* h) { return h ? h->in_size : 0; }

static bool graphs_enabled() {
    static const bool on = [] { return !ab_int("no_graph", 0); }();
    return on;
}

// The ~110-launch forward replayed as one hipGraph: captured on an internal non-blocking stream (the
// caller's stream may be the legacy null stream, which cannot be captured) and launched on the
// caller's stream.  Eager when profiling (per-launch events) or when capture fails.
static int forward_graph(fr_handle* h, const void* in, int in_fmt, int B, float* out, int flags, hipStream_t s) {
    if (!graphs_enabled() || h->prof) return forward(h, in, in_fmt, B, out, flags, s);
    fr_handle::GraphEnt* e = nullptr;
    for (auto& g : h->graphs)
        if (g.in == in && g.out == out && g.fmt == in_fmt && g.B == B && g.flags == flags && g.slot == h->slot) e = &g;
    if (!e) {
        if (h->graphs.size() >= 8 + h->slot_events.size()) {  // evict the least recently used
            auto lru = h->graphs.begin();
            for (auto it = h->graphs.begin(); it != h->graphs.end(); ++it)
                if (it->used < lru->used) lru = it;
            if (lru->exec) {
                (void)hipDeviceSynchronize();
                (void)hipGraphExecDestroy(lru->exec);
            }
            h->graphs.erase(lru);
        }
        h->graphs.push_back({in, out, in_fmt, B, flags, h->slot, nullptr, false, ++h->tick});
        return forward(h, in, in_fmt, B, out, flags, s);  // first sighting: eager
    }
    e->used = ++h->tick;
    if (e->no_graph) return forward(h, in, in_fmt, B, out, flags, s);
    if (!e->exec) {
        if (!h->cap_stream) FR_HIP_CHECK(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
        // branch-parallel capture only without split stages (their parts must own the device, DevSerial)
        // and without the fp8 amax buffers
        h->ms_on = ms_enabled() && !split_runs(h, B) && !h->amax;
        if (h->ms_on && !h->aux_stream) FR_HIP_CHECK(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
        FR_HIP_CHECK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
        const int rc = forward(h, in, in_fmt, B, out, flags, h->cap_stream);
        h->ms_on = false;
        hipGraph_t g = nullptr;
        const hipError_t ec = hipStreamEndCapture(h->cap_stream, &g);
        hipGraphExec_t x = nullptr;
        if (rc == FR_OK && ec == hipSuccess && g && hipGraphInstantiate(&x, g, nullptr, nullptr, 0) == hipSuccess) {
            e->exec = x;
        } else {
            e->no_graph = true;
            (void)hipGetLastError();
        }
        if (g) (void)hipGraphDestroy(g);
        if (!e->exec) return forward(h, in, in_fmt, B, out, flags, s);
    }
    FR_HIP_CHECK(hipGraphLaunch(e->exec, s));
    return FR_OK;
}

static int embed_batch(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, float* out, int flags,
                       void* stream);

// Largest batch one forward runs: every activation tensor of the batch stays below 2 GiB, the range of the
// kernels' 32-bit buffer offsets (IResNet100: 1280 faces, layer1's 112^2 x 64); bigger calls run in chunks
// of that size, multiples of 256 (the tuned batch sizes' tiles).
static int embed_chunk(const fr_handle* h) {
    size_t per = 1;
    for (const auto& t : h->tensors) per = std::max(per, (size_t)t.H * t.W * t.C * sizeof(bf16_t));
    const size_t cap = 0x7fffffffull / per;
    return (int)std::max<size_t>(1, cap >= 512 ? cap / 256 * 256 : cap);
}

static int embed_locked(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, float* out, int flags,
                        void* stream) {
    const int cap = embed_chunk(h);
    if (B <= cap || !in || !out) return embed_batch(h, in, in_fmt, B, H, W, out, flags, stream);
    const size_t in_img = (size_t)H * W * 3 * (in_fmt == FR_IN_F32_NCHW ? sizeof(float) : 1);
    const size_t d = (size_t)fr_embed_dim(h);
    for (int b0 = 0; b0 < B; b0 += cap) {
        const int rc = embed_batch(h, (const char*)in + b0 * in_img, in_fmt, std::min(cap, B - b0), H, W,
                                   out + b0 * d, flags, stream);
        if (rc) return rc;
    }
    return FR_OK;
}

static int embed_batch(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, float* out, int flags,
                       void* stream) {
    if (!h->loaded) { set_error("fr_embed: weights not loaded"); return FR_ERR_STATE; }
    if (!in || !out || B <= 0) { set_error("fr_embed: bad argument"); return FR_ERR_ARG; }
    if (H != h->in_size || W != h->in_size) {
        set_error("fr_embed: input must be " + std::to_string(h->in_size) + "x" + std::to_string(h->in_size) +
                  " (got " + std::to_string(H) + "x" + std::to_string(W) + ")");
        return FR_ERR_ARG;
    }
    if (in_fmt != FR_IN_U8_NHWC && in_fmt != FR_IN_F32_NCHW) { set_error("fr_embed: bad in_fmt"); return FR_ERR_ARG; }
    if (flags & ~(FR_EMBED_RAW | FR_EMBED_ASYNC)) { set_error("fr_embed: unknown flag bits"); return FR_ERR_ARG; }
    FR_HIP_CHECK(hipSetDevice(h->device));
    // An earlier FR_EMBED_ASYNC forward's split stage ran out (sticky).  The flag is only read once the async
    // forwards it may come from have completed: a synchronous call waits for them (otherwise it would take their
    // failure as its own after its own forward, and clear it with its re-run), an async call checks without
    // blocking and leaves a failure of a forward still in flight to a later call or fr_sync_check (reading the
    // flag mid-forward would report the layer1 stage's run-out and miss the layer2 stage's, written later).
    bool flag_final = true;
    if (h->async_pending) {
        if (flags & FR_EMBED_ASYNC) {
            flag_final = hipEventQuery(h->async_ev) == hipSuccess;
            (void)hipGetLastError();  // hipErrorNotReady must not surface at the next launch check
        } else FR_HIP_CHECK(hipEventSynchronize(h->async_ev));
        if (flag_final) h->async_pending = false;
    }
    if (flag_final && *(volatile int*)h->fail_host) {
        *(volatile int*)h->fail_host = 0;
        set_error("fr_embed: a split stage's halo wait ran out in an earlier FR_EMBED_ASYNC forward on this "
                  "handle; the affected embeddings are NaN (reported once, see fr_sync_check)");
        return FR_ERR_STAGE;
    }
    if (B > h->max_batch) {
        int rc = reserve(h, B);
        if (rc) return rc;
    }
    const hipStream_t s = (hipStream_t)stream;
    const int fflags = flags & FR_EMBED_RAW;  // what the forward (and its graph key) depends on
    const bool split = split_runs(h, B);
    int rc;
    {
        DevSerial ser(h, split, s);
        if (autotune_enabled() && !h->prof &&
            std::find(h->tuned_batches.begin(), h->tuned_batches.end(), B) == h->tuned_batches.end()) {
            // first call at this batch size: eager forward that times the tile candidates of every igemm
            // shape on the way (results are exact: the last launch of each conv uses the chosen tile)
            h->tuning = true;
            rc = forward(h, in, in_fmt, B, out, fflags, s);
            h->tuning = false;
            if (!rc) h->tuned_batches.push_back(B);
        } else {
            rc = forward_graph(h, in, in_fmt, B, out, fflags, s);
        }
    }
    if (!rc && split && (flags & FR_EMBED_ASYNC)) {
        FR_HIP_CHECK(hipEventRecord(h->async_ev, s));
        h->async_pending = true;
    }
    if (rc || !split || (flags & FR_EMBED_ASYNC)) return rc;
    // synchronous check: wait for this forward; if a split stage's halo wait ran out, its images are
    // NaN-poisoned, so run the forward again on the per-conv path (no waits) and return that
    FR_HIP_CHECK(hipEventRecord(h->chk_ev, s));
    FR_HIP_CHECK(hipEventSynchronize(h->chk_ev));
    if (!*(volatile int*)h->fail_host) return FR_OK;
    *(volatile int*)h->fail_host = 0;
    ++h->stage_reruns;
    h->no_split = true;
    rc = forward(h, in, in_fmt, B, out, fflags, s);
    h->no_split = false;
    if (rc) return rc;
    FR_HIP_CHECK(hipEventRecord(h->chk_ev, s));
    FR_HIP_CHECK(hipEventSynchronize(h->chk_ev));
    return FR_OK;
}

int fr_embed(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, float* out, int flags, void* stream) {
    if (!h) { set_error("fr_embed: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    return embed_locked(h, in, in_fmt, B, H, W, out, flags, stream);
}

int fr_explain_shape(const fr_handle* h, int* th, int* tw, int* tc) {
    if (!h || !th || !tw || !tc) { set_error("fr_explain_shape: null argument"); return FR_ERR_ARG; }
    if (!h->loaded || h->ex_tensor < 0) { set_error("fr_explain_shape: weights not loaded"); return FR_ERR_STATE; }
    const auto& t = h->tensors[h->ex_tensor];
    *th = t.H; *tw = t.W; *tc = t.C;
    return FR_OK;
}

int fr_explain(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, const float* target, float* cam,
               float* low, float* emb, void* stream) {
    if (!h) { set_error("fr_explain: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->loaded || h->ex_tensor < 0) { set_error("fr_explain: weights not loaded"); return FR_ERR_STATE; }
    if (!cam) { set_error("fr_explain: cam is NULL"); return FR_ERR_ARG; }
    if (!in || B <= 0) { set_error("fr_explain: bad argument"); return FR_ERR_ARG; }
    if (h->max_batch <= 0) { set_error("fr_explain: nothing reserved (call fr_reserve first)"); return FR_ERR_STATE; }
    if (B > h->max_batch) {
        set_error("fr_explain: B = " + std::to_string(B) + " is above the reserved batch " + std::to_string(h->max_batch) +
                  " (fr_reserve)");
        return FR_ERR_ARG;
    }
    if (B > embed_chunk(h)) {  // a chunked forward leaves only its last chunk's activations behind
        set_error("fr_explain: B is above the largest single forward (" + std::to_string(embed_chunk(h)) + ")");
        return FR_ERR_ARG;
    }
    float* e = emb ? emb : h->ex_emb;
    // the forward: waited for and re-run when a split stage's wait ran out (no FR_EMBED_ASYNC), so the explained
    // tensor below is that of valid embeddings; B <= max_batch, so nothing is re-reserved
    int rc = embed_locked(h, in, in_fmt, B, H, W, e, FR_EMBED_RAW, stream);
    if (rc) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int f16 = h->dtype == FR_DTYPE_F16;
    const auto& t = h->tensors[h->ex_tensor];
    if (!cam_supported(B, t.H, t.W, t.C, h->in_size)) {
        set_error("fr_explain: explained tensor out of the map kernel's range");
        return FR_ERR_ARG;
    }
    if (h->ex_layout == 2) {
        Op op = h->ops[h->ex_conv];  // block8.conv2d without its residual
        op.res = -1;
        op.out = h->ex_tensor;
        op.out_off = 0;
        if ((rc = run_conv_op(h, op, B, f16, s))) return rc;
        FR_HIP_CHECK(launch_cam(t.dev, B, t.H, t.W, t.C, f16 || t.f16, nullptr, 0, 2, h->in_size, cam, low, s));
        return FR_OK;
    }
    const DevConvW& hw = h->convw[h->ops.back().wi];
    const int need = h->ex_layout == 0 ? t.C : t.H * t.W * t.C;
    if (hw.K != need || !head_grad_supported(B, hw.Cout, hw.K, hw.Kpad)) {
        set_error("fr_explain: head shape does not match the explained tensor");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_score_grad(e, target, B, hw.Cout, h->ex_g, s));
    FR_HIP_CHECK(launch_head_grad(h->ex_g, B, hw.Cout, hw.w, hw.K, hw.Kpad, f16, h->ex_v, s));
    FR_HIP_CHECK(launch_cam(t.dev, B, t.H, t.W, t.C, f16 || t.f16, h->ex_v, hw.Kpad, h->ex_layout, h->in_size, cam, low, s));
    return FR_OK;
}

int fr_features_dim(const fr_handle* h) {
    if (!h) { set_error("fr_features_dim: null handle"); return FR_ERR_ARG; }
    if (!h->loaded || h->ops.empty() || h->ops.back().kind != OP_HEAD) {
        set_error("fr_features_dim: weights not loaded");
        return FR_ERR_STATE;
    }
    return h->convw[h->ops.back().wi].K;
}

int fr_features(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, float* out, void* stream) {
    if (!h) { set_error("fr_features: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->loaded || h->ops.empty() || h->ops.back().kind != OP_HEAD) {
        set_error("fr_features: weights not loaded");
        return FR_ERR_STATE;
    }
    if (!in || !out || B <= 0) { set_error("fr_features: bad argument"); return FR_ERR_ARG; }
    if (h->max_batch <= 0) { set_error("fr_features: nothing reserved (call fr_reserve first)"); return FR_ERR_STATE; }
    if (B > h->max_batch) {
        set_error("fr_features: B = " + std::to_string(B) + " is above the reserved batch " + std::to_string(h->max_batch) +
                  " (fr_reserve)");
        return FR_ERR_ARG;
    }
    if (B > embed_chunk(h)) {  // a chunked forward leaves only its last chunk's activations behind
        set_error("fr_features: B is above the largest single forward (" + std::to_string(embed_chunk(h)) + ")");
        return FR_ERR_ARG;
    }
    const Op& head = h->ops.back();
    const auto& t = h->tensors[head.in];
    const int K = h->convw[head.wi].K, P = t.H * t.W;
    if (P * t.C != K || t.C % 8) { set_error("fr_features: head input does not match the head's K"); return FR_ERR_ARG; }
    // the forward is waited for (no FR_EMBED_ASYNC), so the head's input below is that of valid embeddings; the
    // embeddings themselves go to fr_explain's scratch
    if (!h->ex_emb) { set_error("fr_features: nothing reserved (call fr_reserve first)"); return FR_ERR_STATE; }
    const int rc = embed_locked(h, in, in_fmt, B, H, W, h->ex_emb, FR_EMBED_RAW, stream);
    if (rc) return rc;
    FR_HIP_CHECK(launch_features_cvt(t.dev, B, P, t.C, h->dtype == FR_DTYPE_F16 || t.f16, out, (hipStream_t)stream));
    return FR_OK;
}

int fr_features_at_shape(const fr_handle* h, int cut, int* th, int* tw, int* tc) {
    if (!h || !th || !tw || !tc) { set_error("fr_features_at_shape: null argument"); return FR_ERR_ARG; }
    if (cut != FR_CUT_LAYER4_IN) { set_error("fr_features_at_shape: unknown cut"); return FR_ERR_ARG; }
    if (h->arch != FR_ARCH_RESNET50_ARCFACE) {
        set_error("fr_features_at_shape: FR_CUT_LAYER4_IN exists for resnet50_arcface only");
        return FR_ERR_ARG;
    }
    if (!h->loaded || h->cut_l4in < 0) { set_error("fr_features_at_shape: weights not loaded"); return FR_ERR_STATE; }
    const auto& t = h->tensors[h->cut_l4in];
    *th = t.H; *tw = t.W; *tc = t.C;
    return FR_OK;
}

int fr_features_at(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, int cut, float* out, void* stream) {
    if (!h) { set_error("fr_features_at: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (cut != FR_CUT_LAYER4_IN) { set_error("fr_features_at: unknown cut"); return FR_ERR_ARG; }
    if (h->arch != FR_ARCH_RESNET50_ARCFACE) {
        set_error("fr_features_at: FR_CUT_LAYER4_IN exists for resnet50_arcface only");
        return FR_ERR_ARG;
    }
    if (h->dtype == FR_DTYPE_FP8) { set_error("fr_features_at: not available on an FR_DTYPE_FP8 handle"); return FR_ERR_ARG; }
    if (!h->loaded || h->cut_l4in < 0) { set_error("fr_features_at: weights not loaded"); return FR_ERR_STATE; }
    if (!in || !out || B <= 0) { set_error("fr_features_at: bad argument"); return FR_ERR_ARG; }
    if (h->max_batch <= 0 || !h->ex_emb) {
        set_error("fr_features_at: nothing reserved (call fr_reserve first)");
        return FR_ERR_STATE;
    }
    if (B > h->max_batch) {
        set_error("fr_features_at: B = " + std::to_string(B) + " is above the reserved batch " +
                  std::to_string(h->max_batch) + " (fr_reserve)");
        return FR_ERR_ARG;
    }
    if (B > embed_chunk(h)) {  // a chunked forward leaves only its last chunk's activations behind
        set_error("fr_features_at: B is above the largest single forward (" + std::to_string(embed_chunk(h)) + ")");
        return FR_ERR_ARG;
    }
    const auto& t = h->tensors[h->cut_l4in];
    if (t.C % 8) { set_error("fr_features_at: the cut tensor's channels are no multiple of 8"); return FR_ERR_ARG; }
    // The whole forward runs and is waited for (fr_features' rules).  Every plan tensor has an allocation of its own
    // (reserve()), so nothing after the cut overwrites it; and it is a tensor the per-conv ops layer4.0.conv1 and
    // layer4.0.downsample read, so whichever of the layer3 chain stage or its member convs ran has written it as plain
    // 16-bit NHWC (the chain's own layouts stay inside the launch).
    const int rc = embed_locked(h, in, in_fmt, B, H, W, h->ex_emb, FR_EMBED_RAW, stream);
    if (rc) return rc;
    FR_HIP_CHECK(launch_features_cvt(t.dev, B * t.H * t.W, 1, t.C, h->dtype == FR_DTYPE_F16 || t.f16, out,
                                     (hipStream_t)stream));
    return FR_OK;
}

int fr_embed_match(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, int k, float* emb_out,
                   float* scores, int32_t* idx, void* stream) {
    if (!h) { set_error("fr_embed_match: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = embed_locked(h, in, in_fmt, B, H, W, emb_out, 0, stream);
    if (rc) return rc;
    return match_locked(h, emb_out, B, k, scores, idx, stream);
}

int fr_segment_mean_normalize(const float* E, int D, const int32_t* seg_start, int n_seg, float* out, void* stream) {
    if (!E || !seg_start || !out || D <= 0 || n_seg <= 0) { set_error("fr_segment_mean_normalize: bad argument"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_segment_mean_normalize(E, D, seg_start, n_seg, out, (hipStream_t)stream));
    return FR_OK;
}

int fr_debug_plan(fr_handle* h, int B, char* buf, size_t n) {
    if (!h || !buf || n == 0 || B <= 0) { set_error("fr_debug_plan: bad argument"); return FR_ERR_ARG; }
    std::string out;
    const std::vector<char> stage_run = stage_plan(h, B);
    for (const auto& op : h->ops) {
        if (op_skipped(op, stage_run)) continue;
        if (op.kind == OP_STAGE) {
            out += stage_plan_line(h, op, B);
            continue;
        }
        if (op.kind != OP_CONV && op.kind != OP_HEAD) {
            out += std::string(op.kind == OP_PRE ? "pre" : op.kind == OP_MAXPOOL ? "maxpool" : "avgpool") + "\n";
            continue;
        }
        out += conv_plan_line(h, op, B);
    }
    std::snprintf(buf, n, "%s", out.c_str());
    return out.size() + 1 <= n ? FR_OK : FR_ERR_ARG;
}

int fr_set_option(fr_handle* h, int option, int value) {
    if (!h) { set_error("fr_set_option: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    switch (option) {
        case FR_OPT_STAGE:
            if (value < 0 || value > 2) { set_error("fr_set_option: FR_OPT_STAGE is 0, 1 or 2"); return FR_ERR_ARG; }
            h->stage_mode = value;
            break;
        case FR_OPT_STAGE_MIN_FILL:
            if (value < 0 || value > 100) { set_error("fr_set_option: FR_OPT_STAGE_MIN_FILL is 0..100"); return FR_ERR_ARG; }
            h->stage_min_fill = value;
            break;
        case FR_OPT_KEEP_INTERMEDIATES: h->keep_inter = value != 0; break;
        case FR_OPT_MATCH_EXACT: h->match_exact = value != 0; break;
        case FR_OPT_X3_MIN_ROWS:
            if (value < 1) { set_error("fr_set_option: FR_OPT_X3_MIN_ROWS must be >= 1"); return FR_ERR_ARG; }
            h->x3_min_rows = value;
            break;
        case FR_OPT_STAGE_SPIN_LIMIT: h->spin_limit = value; break;
        case FR_OPT_STAGE_VARIANT:
            if (value < 0 || value > 3) { set_error("fr_set_option: FR_OPT_STAGE_VARIANT is 0 .. 3"); return FR_ERR_ARG; }
            h->stage_variant = value;
            break;
        case FR_OPT_SPLITK_INLAUNCH: h->splitk_inlaunch = value != 0; break;
        case FR_OPT_BATCH_INVARIANT:
            // an e4m3 conv scales its activations by the amax of the whole batch (kernels.h need_amax), so an fp8
            // handle cannot promise batch-independent bits: refused rather than silently broken
            if (value != 0 && h->dtype == FR_DTYPE_FP8) {
                set_error("fr_set_option: FR_OPT_BATCH_INVARIANT is not available on FR_DTYPE_FP8 handles (their e4m3 "
                          "convs scale activations by a per-batch amax)");
                return FR_ERR_ARG;
            }
            if ((value != 0) != h->invariant) {  // the kernel choices are re-measured under the new rule
                h->invariant = value != 0;
                h->tuned.clear();
                h->tuned_batches.clear();
            }
            break;
        case FR_OPT_FUSED_MASK:
            if (value < 0 || value > 127) { set_error("fr_set_option: FR_OPT_FUSED_MASK is 0 .. 127"); return FR_ERR_ARG; }
            h->fused_mask = value;
            break;
        default: set_error("fr_set_option: unknown option " + std::to_string(option)); return FR_ERR_ARG;
    }
    drop_graphs(h);  // captured replays bake in the plan
    return FR_OK;
}

int fr_get_option(const fr_handle* h, int option) {
    if (!h) return FR_ERR_ARG;
    switch (option) {
        case FR_OPT_STAGE: return h->stages.empty() ? 0 : h->stage_mode;
        case FR_OPT_STAGE_MIN_FILL: return h->stage_min_fill;
        case FR_OPT_KEEP_INTERMEDIATES: return h->keep_inter ? 1 : 0;
        case FR_OPT_MATCH_EXACT: return h->match_exact ? 1 : 0;
        case FR_OPT_X3_MIN_ROWS: return (int)h->x3_min_rows;
        case FR_OPT_STAGE_SPIN_LIMIT: return h->spin_limit;
        case FR_OPT_STAGE_VARIANT: return h->stage_variant;
        case FR_OPT_SPLITK_INLAUNCH: return h->splitk_inlaunch ? 1 : 0;
        case FR_OPT_BATCH_INVARIANT: return h->invariant ? 1 : 0;
        case FR_OPT_FUSED_MASK: return h->fused_mask;
        default: return FR_ERR_ARG;
    }
}

int fr_debug_stage_timeouts(fr_handle* h) {
    if (!h) return FR_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->stage_spin) return 0;
    int v = 0;
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(hipDeviceSynchronize());
    FR_HIP_CHECK(hipMemcpy(&v, h->stage_spin, sizeof(int), hipMemcpyDeviceToHost));
    return v;
}

int fr_debug_stage_reruns(fr_handle* h) {
    if (!h) return FR_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    return (int)h->stage_reruns;
}

int fr_sync_check(fr_handle* h, void* stream) {
    if (!h) { set_error("fr_sync_check: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (h->async_pending) {  // the async forwards may have been issued on another stream
        FR_HIP_CHECK(hipEventSynchronize(h->async_ev));
        h->async_pending = false;
    }
    if (*(volatile int*)h->fail_host) {
        *(volatile int*)h->fail_host = 0;
        set_error("fr_sync_check: a split stage's halo wait ran out in an FR_EMBED_ASYNC forward on this handle; "
                  "the affected embeddings are NaN");
        return FR_ERR_STAGE;
    }
    return FR_OK;
}

int fr_prof_enable(fr_handle* h, int on) {
    if (!h) { set_error("fr_prof_enable: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    FR_HIP_CHECK(hipSetDevice(h->device));
    for (auto& r : h->prof_pending) {
        (void)hipEventSynchronize(r.b);
        h->ev_free.push_back(r.a);
        h->ev_free.push_back(r.b);
    }
    h->prof_pending.clear();
    h->prof_acc.clear();
    h->prof = on > 0;
    h->prof_stride = on > 0 ? on : 1;
    h->prof_seen = 0;
    return FR_OK;
}

int fr_prof_only(fr_handle* h, const char* kernel_class) {
    if (!h) { set_error("fr_prof_only: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    h->prof_only = kernel_class ? kernel_class : "";
    return FR_OK;
}

int fr_prof_slots(fr_handle* h, const char* kernel_class, int n) {
    if (!h || n < 0 || n > 4096 || (n > 0 && (!kernel_class || !*kernel_class))) {
        set_error("fr_prof_slots: bad argument");
        return FR_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(hipDeviceSynchronize());
    for (auto& g : h->graphs)  // graphs of the old slots hold the old events
        if (g.slot >= 0 && g.exec) (void)hipGraphExecDestroy(g.exec);
    h->graphs.erase(std::remove_if(h->graphs.begin(), h->graphs.end(), [](const fr_handle::GraphEnt& g) { return g.slot >= 0; }),
                    h->graphs.end());
    for (auto& pr : h->slot_events) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    h->slot_events.clear();
    h->slot = -1;
    h->slot_nl = 0;
    h->slot_work.assign(n > 0 ? n : 0, {0.0, 0.0});
    h->slot_class = n > 0 ? kernel_class : "";
    for (int i = 0; i < n; ++i) {
        hipEvent_t a, b;
        FR_HIP_CHECK(hipEventCreate(&a));
        FR_HIP_CHECK(hipEventCreate(&b));
        h->slot_events.push_back({a, b});
    }
    return FR_OK;
}

int fr_prof_slot_select(fr_handle* h, int slot) {
    if (!h || slot < -1 || slot >= (int)h->slot_events.size()) { set_error("fr_prof_slot_select: bad slot"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    h->slot = slot;
    return FR_OK;
}

int fr_prof_slot_ms(fr_handle* h, int slot, float* ms) {
    if (!h || !ms || slot < 0 || slot >= (int)h->slot_events.size()) { set_error("fr_prof_slot_ms: bad argument"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(hipEventSynchronize(h->slot_events[slot].second));
    FR_HIP_CHECK(hipEventElapsedTime(ms, h->slot_events[slot].first, h->slot_events[slot].second));
    return FR_OK;
}

int fr_prof_slot_work(fr_handle* h, int slot, double* flops, double* bytes) {
    if (!h || !flops || !bytes || slot < 0 || slot >= (int)h->slot_work.size()) {
        set_error("fr_prof_slot_work: bad argument");
        return FR_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    *flops = h->slot_work[slot].first;
    *bytes = h->slot_work[slot].second;
    return FR_OK;
}

int fr_prof_collect(fr_handle* h) {
    if (!h) { set_error("fr_prof_collect: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    FR_HIP_CHECK(hipSetDevice(h->device));
    for (auto& r : h->prof_pending) {
        FR_HIP_CHECK(hipEventSynchronize(r.b));
        float ms = 0.f;
        FR_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
        size_t i = 0;
        while (i < h->prof_acc.size() && h->prof_acc[i].first != r.cls) ++i;
        if (i == h->prof_acc.size()) h->prof_acc.push_back({r.cls, {}});
        auto& acc = h->prof_acc[i].second;
        acc.ms += ms;
        acc.launches += 1;
        acc.flops += r.flops;
        acc.bytes += r.bytes;
        h->ev_free.push_back(r.a);
        h->ev_free.push_back(r.b);
    }
    h->prof_pending.clear();
    return (int)h->prof_acc.size();
}

int fr_prof_get(const fr_handle* h, int i, char* name, size_t n, double* total_ms, int64_t* launches,
                double* flops) {
    if (!h || i < 0 || i >= (int)h->prof_acc.size()) { set_error("fr_prof_get: bad index"); return FR_ERR_ARG; }
    const auto& e = h->prof_acc[i];
    if (name && n) { std::strncpy(name, e.first.c_str(), n - 1); name[n - 1] = 0; }
    if (total_ms) *total_ms = e.second.ms;
    if (launches) *launches = e.second.launches;
    if (flops) *flops = e.second.flops;
    return FR_OK;
}

int fr_prof_get_bytes(const fr_handle* h, int i, double* bytes) {
    if (!h || i < 0 || i >= (int)h->prof_acc.size() || !bytes) { set_error("fr_prof_get_bytes: bad argument"); return FR_ERR_ARG; }
    *bytes = h->prof_acc[i].second.bytes;
    return FR_OK;
}

int fr_debug_tensor_count(const fr_handle* h) { return h ? (int)h->tensors.size() : 0; }

const char* fr_debug_tensor_name(const fr_handle* h, int t) {
    if (!h || t < 0 || t >= (int)h->tensors.size()) return "";
    return h->tensors[t].name.c_str();
}

int fr_debug_tensor_shape(const fr_handle* h, int t, int* H, int* W, int* C) {
    if (!h || t < 0 || t >= (int)h->tensors.size() || !H || !W || !C) { set_error("fr_debug_tensor_shape: bad argument"); return FR_ERR_ARG; }
    *H = h->tensors[t].H; *W = h->tensors[t].W; *C = h->tensors[t].C;
    return FR_OK;
}

int fr_debug_tensor_dtype(const fr_handle* h, int t) {
    if (!h || t < 0 || t >= (int)h->tensors.size()) { set_error("fr_debug_tensor_dtype: bad argument"); return FR_ERR_ARG; }
    return h->tensors[t].f16 ? FR_DTYPE_F16 : (h->dtype == FR_DTYPE_FP8 ? FR_DTYPE_BF16 : h->dtype);
}

int fr_debug_copy_tensor(fr_handle* h, int t, int B, void* dst, void* stream) {
    if (!h || t < 0 || t >= (int)h->tensors.size() || !dst || B <= 0 || B > h->max_batch || !h->tensors[t].dev) {
        set_error("fr_debug_copy_tensor: bad argument (tensor id / batch / not reserved)");
        return FR_ERR_ARG;
    }
    const auto& d = h->tensors[t];
    FR_HIP_CHECK(hipMemcpyAsync(dst, d.dev, (size_t)B * d.H * d.W * d.C * sizeof(bf16_t), hipMemcpyDeviceToDevice,
                                (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
