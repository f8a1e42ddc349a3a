// What engine.cpp (handle, reserve, forward, the handle's C ABI), plan.cpp (blob parser, plan builders), stages.cpp (the
// fused-stage kinds), convs.cpp (the conv kernel kinds: selection, tuning, launch) and gallery_api.cpp (gallery and
// matcher C ABI) share: the handle, the plan's records and a few helpers.  ops_api.cpp and the other *_api.cpp files hold
// the handle-free C ABI groups.  Nothing here is part of the library's ABI.
#pragma once
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/frhip.h"
#include "kernels.h"

#pragma GCC visibility push(hidden)

namespace fr {

struct DevConvW {
    bf16_t* w = nullptr;
    float* bias = nullptr;
    float* slope = nullptr;
    float* bias9 = nullptr;  // [9][Npad] border-class bias (input BN folded into a 3x3/s1/p1 conv)
    bf16_t* wimg = nullptr;  // conv_img.hip K-step slice images (convs its kernels apply to)
    float* negf = nullptr;   // conv_img / conv_rows: [Npad] activation negative-side factor (slope / 0 / 1)
    bf16_t* wrows = nullptr; // conv_rows.hip weight image (rows_pack_weights)
    float* ep = nullptr;     // conv_rows.hip: [9][Npad] bias per border class
    bf16_t* wring = nullptr; // conv_wring.hip substep images (wring_pack_weights)
    uint8_t* w8 = nullptr;   // FR_DTYPE_FP8: e4m3 [Npad][Kpad8] + per-channel scale
    float* wscale = nullptr;
    int Cout = 0, Kh = 1, Kw = 1, Cin = 0, K = 0, Npad = 0, Kpad = 0, Kpad8 = 0;
    int K1 = 0, C2 = 0;  // K-concatenated 1x1 projection: K = K1 + C2 (ConvArgs::x2), else K1 = K, C2 = 0
};

struct TensorDesc {
    int H, W, C;
    bf16_t* dev = nullptr;
    std::string name;  // oracle module whose output this tensor equals ("" = internal)
    bool f16 = false;  // stored as f16 in a bf16 plan (IRV1's f16 section, plan.cpp build_irv1)
};

enum OpKind { OP_PRE, OP_CONV, OP_MAXPOOL, OP_AVGPOOL, OP_HEAD, OP_STAGE };
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_PRELU = 2 };  // Op::act (and ConvArgs::act, fr_conv_desc::act)

struct Op {
    OpKind kind;
    int in = -1, in_off = 0, cin = 0;
    int out = -1, out_off = 0;
    int res = -1, res_off = 0;
    int kh = 1, kw = 1, sh = 1, sw = 1, ph = 0, pw = 0;
    int act = ACT_NONE;
    int wi = -1;
    int pk = 0, ps = 0, pp = 0;
    int stage = -1;  // OP_STAGE: its StageRec; OP_CONV: the stage that covers it (skipped when stages run)
    int x2 = -1, x2_off = 0, st2 = 1;  // OP_CONV with a K-concatenated downsample: its input tensor, stride
    bool fuse_stem = false;  // OP_PRE of IResNet100: u8 input runs preprocess + the next (stem) conv fused
    int grp = -1;    // index into the stage plan (stage_plan)
};

// The kinds of fused stage: one launch (STAGE_BNECK28: one per block) beside a run of member ops, the faster measured
// per batch size.  What depends on the kind alone is in stages.cpp's table; DESIGN.md "Fused stage kinds" lists
// the steps to add one.
enum StageKind {
    STAGE_LDS,        // stride-1 blocks of an IResNet100 layer, LDS-resident: conv_stage.hip (parts = 1, 14x14x256),
                      // conv_split_stage.hip (parts = 2 / 4 workgroups per image, 28x28x128 / 56x56x64), conv_stage8.hip (fp8)
    STAGE_TRANS,      // IResNet100 layer1.0 (conv_trans.hip): conv_ops = {conv1, conv2 + downsample}
    STAGE_STEM160,    // IRV1 conv2d_1a .. conv2d_3b (conv_stem160.hip): conv_ops = {1a, 2a, 2b, maxpool_3a, 3b}
    STAGE_CHAIN35,    // IRV1 repeat_1 (conv_chain35.hip): per block {branch1.0 + branch2.0 + branch0, branch1.1, branch2.1,
                      // branch2.2, conv2d}, x_tensors = the block outputs
    STAGE_CHAIN17,    // IRV1 repeat_2 (conv_chain.hip): per block {branch1.0 + branch0, 1x7, 7x1, conv2d}
    STAGE_CHAIN_R50,  // ResNet-50 layer3.1 .. 3.5 (conv_chain_r50.hip): per block {conv1, conv2, conv3}
    STAGE_BNECK28,    // ResNet-50 layer1 (conv_bneck28.hip): per block {conv1, conv2, conv3}, x_tensors = the block
                      // outputs; bn_ds: the first is layer1.0 (conv3 + K-concatenated downsample)
    STAGE_STEM_R50,   // ResNet-50 conv1 + maxpool (conv_stem_r50.hip): conv_ops = {conv1, maxpool}
    STAGE_NKINDS
};

struct StageRec {
    StageKind kind = STAGE_LDS;
    int in = -1, out = -1, nblk = 0;
    int parts = 1, H = 14, C = 256;
    std::vector<int> conv_ops;            // member op indices (per kind: StageKind)
    std::vector<int> t_tensors, x_tensors;  // per block: conv1 output, block output
    // STAGE_LDS
    bf16_t* w = nullptr;                  // packed K-step weight images
    StageConv* table = nullptr;           // [2*nblk]
    float* ep = nullptr;                  // [2*nblk][9][256] epilogue bias per border class
    float* slope = nullptr;               // [2*nblk][256] negative-side factor (slope / 0 / 1)
    bf16_t** dbg = nullptr;               // [2*nblk] device pointer table: x outputs then t outputs
    bool fp8 = false;                     // e4m3 stage (conv_stage8.hip): the members carry .wscale
    uint8_t* w8 = nullptr;                // fp8: stage8_pack_weights images of all convs
    float* wscale = nullptr;              // fp8: [2*nblk][256] per-channel weight scales
    // the conv after the stage (IResNet100 layer4.0.conv1 / layer3.0.conv1, 3x3/s1 C -> 2C + border-class bias +
    // PReLU) runs on the stage's final patch (conv_stage.hip run_tail); its weights and tables follow the blocks'
    // as two C-channel halves; tail_op is also the last entry of conv_ops
    int tail_op = -1;
    // STAGE_TRANS
    bf16_t* tw1 = nullptr;                // trans_pack_weights images of conv1 / conv2 + downsample
    bf16_t* tw2 = nullptr;
    float* tep1 = nullptr;                // [9][64] conv1 bias per border class
    float* tsl1 = nullptr;                // [64] conv1 PReLU slopes
    float* tb2 = nullptr;                 // [64] conv2 + downsample bias
    // the chain kinds
    bool bn_ds = false;
    bf16_t* cw = nullptr;                 // the packed weights of all blocks
    float* cbias = nullptr;               // the member convs' biases
};

}  // namespace fr

#pragma GCC visibility pop

struct fr_handle {
    int device = 0, arch = 0, dtype = 0;
    std::mutex mu;
    bool loaded = false;
    int in_size = 112, embed_dim = 512;
    std::vector<fr::TensorDesc> tensors;
    std::vector<fr::Op> ops;
    std::vector<fr::DevConvW> convw;
    std::vector<void*> weight_allocs;
    int max_batch = 0;
    std::vector<void*> act_allocs;
    float* partial = nullptr;
    size_t partial_floats = 0;
    int* splitk_cnt = nullptr;  // [FR_SPLITK_TILES] in-launch split-K arrival counters (conv_igemm), zero between launches
    bool splitk_inlaunch = true;  // FR_OPT_SPLITK_INLAUNCH
    bool inlaunch_used = false;   // an in-launch split-K conv has run (the per-forward counter memset is needed)
    // gallery
    float* gallery = nullptr;
    int64_t g_rows = 0;
    int64_t g_cap = 0;       // rows allocated (fr_gallery_write grows it geometrically)
    int g_dim = 0;
    int64_t g_base = 0;
    bf16_t* g_hi = nullptr;  // bf16 hi/lo split of the prepared gallery in chunk order (match_x3.hip), N >= X3_MIN_ROWS
    int* match_fb = nullptr;  // device counter of exact-rescan fallbacks (fr_debug_match_fallbacks)
    bool match_exact = false; // FR_OPT_MATCH_EXACT: always the f32-MFMA kernel
    int64_t x3_min_rows = fr::X3_MIN_ROWS;  // FR_OPT_X3_MIN_ROWS
    float* cand_s = nullptr;
    int32_t* cand_i = nullptr;
    size_t cand_cap = 0;
    // per-kernel-class event timing (fr_prof_*): events recorded on the launching stream
    struct ProfRec { std::string cls; hipEvent_t a, b; double flops, bytes; };
    struct ProfAcc { double ms = 0; int64_t launches = 0; double flops = 0, bytes = 0; };
    bool prof = false;
    int prof_stride = 1;        // time every n-th matching launch (sampling keeps the overhead small)
    uint64_t prof_seen = 0;
    std::string prof_only;  // non-empty: time only this kernel class
    std::vector<hipEvent_t> ev_free;
    std::vector<ProfRec> prof_pending;
    std::vector<std::pair<std::string, ProfAcc>> prof_acc;
    // forward replays as hipGraphs, keyed by the call's pointers / shape (captured on the second call
    // with a key; the first call runs eagerly and warms per-kernel attributes)
    struct GraphEnt { const void* in; float* out; int fmt, B, flags, slot; hipGraphExec_t exec; bool no_graph; uint64_t used; };
    // graph-slot timing (fr_prof_slots): an event pair per slot around one launch of one kernel class --
    // slot i times launch i mod (the class's launches per forward) -- captured into the graph of that slot,
    // so timed steps replay graphs and still time the class
    std::string slot_class;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> slot_events;
    std::vector<std::pair<double, double>> slot_work;  // the timed launch's algorithmic FLOPs and bytes
    int slot = -1;         // the slot the next forward captures / replays (-1: none)
    bool slot_done = false;  // the slot's pair is placed in the current forward
    int slot_seen = 0;     // launches of slot_class so far in the current forward
    int slot_nl = 0;       // launches of slot_class per forward (learned by the first slot forward)
    std::vector<GraphEnt> graphs;
    hipStream_t cap_stream = nullptr;
    // branch-parallel capture (forward_graph): a second capturing stream and one event per op
    hipStream_t aux_stream = nullptr;
    std::vector<hipEvent_t> op_events;
    bool ms_on = false;
    uint64_t tick = 0;
    // per-shape igemm tile autotuning (numerically invisible: every tile accumulates K in the same
    // order; split-K choices stay with the cost model)
    struct Tuned { int key[13]; int tile, split; };  // the measured kernel choice per conv shape (tune_conv)
    std::vector<Tuned> tuned;
    std::vector<int> tuned_batches;
    struct StageMeas { int stage, B, run; float t_stage, t_conv; };  // measured stage-vs-per-conv choice per batch
    std::vector<StageMeas> stage_meas;
    bool tuning = false;
    // fused stages (fr_set_option FR_OPT_STAGE / FR_OPT_KEEP_INTERMEDIATES / FR_OPT_FUSED_MASK)
    std::vector<fr::StageRec> stages;
    // FaceNet projection (Linear(512, d) + F.normalize after IRV1's own L2; facenet_model.py:20-23,32-35)
    float* proj_w = nullptr;
    float* proj_b = nullptr;
    int proj_d = 0;
    float* emb_pre = nullptr;  // [max_batch][512] IRV1 output before the projection
    float* amax = nullptr;     // FR_DTYPE_FP8: per-tensor max |x| of the current forward [ntensors]
    std::vector<char> need_amax;  // per tensor: the input of a per-conv e4m3 conv (its producer writes amax)
    bf16_t* stage_xchg = nullptr;  // split-stage boundary rows (split_stage_xchg_elems(max_batch), reserve)
    int* stage_flags = nullptr;    // split-stage progress counters [stage][max_batch][4], never reset
    int* stage_spin = nullptr;     // split-stage bounded-wait overruns (fr_debug_stage_timeouts)
    // split-stage failure reporting: a host-mapped flag the kernel sets when a halo wait runs out
    // (fail_host: host view, fail_dev: the device alias the kernel stores to)
    int* fail_host = nullptr;
    int* fail_dev = nullptr;
    int spin_limit = 0;            // FR_OPT_STAGE_SPIN_LIMIT (0: the kernel's default, < 0: every wait runs out)
    int stage_variant = 0;         // FR_OPT_STAGE_VARIANT (1: the legacy 14-fragment layer3 stage kernel, 2: one wave per SIMD,
                                   // 3: waves split by output channel)
    bool no_split = false;         // re-run of a failed forward: split stages off
    int64_t stage_reruns = 0;      // forwards re-run on the per-conv path after a run-out wait
    hipEvent_t chk_ev = nullptr;   // completion of the last synchronous-checked forward
    hipEvent_t async_ev = nullptr; // completion of the last FR_EMBED_ASYNC split-stage forward ...
    bool async_pending = false;    // ... not yet waited for (its failure is not yet latched)
    bool split_registered = false; // counted in the per-device split-stage handle registry (DevSerial)
    int stage_mode = 1;       // FR_OPT_STAGE: 0 off, 1 auto (stage_runs), 2 always
    int stage_min_fill = 80;  // FR_OPT_STAGE_MIN_FILL (percent)
    int n_cu = 256;
    bool keep_inter = false;
    // FR_OPT_BATCH_INVARIANT: every kernel choice sums K in the implicit GEMM's order (no split-K, no stage /
    // transition kernel, a fixed head split), so a face's embedding does not depend on its batch
    bool invariant = false;
    int fused_mask = 127;  // FR_OPT_FUSED_MASK
    const uint8_t* fwd_u8 = nullptr;  // the current forward's u8 crops when a fused stem prepares them itself
    // fr_explain (explain.hip): the explained tensor, how the head reads it (0 pooled, 1 flattened, 2 = the
    // activation map of ex_tensor, which op ex_conv writes when run again without its residual), and the scratch
    // of reserve(): the score gradient [max_batch][embed_dim], the head-input gradient [max_batch][head Kpad] and
    // the raw embeddings when the caller takes none
    int ex_tensor = -1, ex_layout = 0, ex_conv = -1;
    int cut_l4in = -1;  // fr_features_at(FR_CUT_LAYER4_IN): the tensor layer4.0 reads (ResNet-50 only)
    float* ex_g = nullptr;
    float* ex_v = nullptr;
    float* ex_emb = nullptr;
};

#pragma GCC visibility push(hidden)

namespace fr {

constexpr int FR_SPLITK_TILES = 1 << 16;  // in-launch split-K tile counters per handle

// ------------------------------------------------------------------ engine.cpp
int dev_alloc(void** p, size_t bytes);

template <class T>
int upload(fr_handle* h, T** dst, const std::vector<T>& src) {
    void* p = nullptr;
    int rc = dev_alloc(&p, src.size() * sizeof(T));
    if (rc) return rc;
    h->weight_allocs.push_back(p);
    FR_HIP_CHECK(hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = (T*)p;
    return FR_OK;
}

int run_maxpool_op(fr_handle* h, const Op& op, int B, int f16, hipStream_t s);

// Per-op skip rule: a stage op runs when its plan entry says so; its member ops run when it does not (Op::grp).
inline bool op_skipped(const Op& op, const std::vector<char>& run) {
    if (op.kind == OP_STAGE) return !run[op.grp];
    return op.grp >= 0 && run[op.grp];
}

inline hipEvent_t prof_event(fr_handle* h) {
    if (!h->ev_free.empty()) { hipEvent_t e = h->ev_free.back(); h->ev_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Brackets one launch with two events when profiling is on; `cls` names the kernel instantiation so
// the totals line up with rocprofv3's per-kernel rows.
struct ProfScope {
    fr_handle* h; hipStream_t s; hipEvent_t a = nullptr, b = nullptr; bool stamped = false;
    std::string cls; double flops = 0, bytes = 0;  // algorithmic FLOPs and HBM bytes of the launch
    ProfScope(fr_handle* h_, hipStream_t s_) : h(h_), s(s_) {}
    // Call right before the launch once the class is known.  With `ka` the pair is handed to the
    // conv launcher, which stamps it from the dispatch packet (hipExtLaunchKernel: no extra stream
    // commands); otherwise the pair is recorded around the launch(es) with hipEventRecord.
    bool slot_pair = false;
    void start(const std::string& c, ConvArgs* ka = nullptr) {
        cls = c;
        if (!h->prof && h->slot >= 0 && cls == h->slot_class) {  // graph-slot timing
            const int ord = h->slot_seen++;
            if (h->slot_seen > h->slot_nl) h->slot_nl = h->slot_seen;
            if (!h->slot_done && ord == h->slot % h->slot_nl) {
                (void)hipEventRecord(h->slot_events[h->slot].first, s);
                h->slot_done = true;
                slot_pair = true;
            }
            return;
        }
        if (!h->prof || (!h->prof_only.empty() && h->prof_only != cls)) return;
        if (h->prof_seen++ % h->prof_stride != 0) return;
        a = prof_event(h);
        b = a ? prof_event(h) : nullptr;
        if (!b) { if (a) h->ev_free.push_back(a); a = nullptr; return; }
        if (ka) { ka->ev0 = a; ka->ev1 = b; stamped = true; }
        else (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (slot_pair) {
            (void)hipEventRecord(h->slot_events[h->slot].second, s);
            h->slot_work[h->slot] = {flops, bytes};
        }
        if (!a) return;
        if (!stamped) (void)hipEventRecord(b, s);
        h->prof_pending.push_back({cls, a, b, flops, bytes});
    }
};

// ------------------------------------------------------------------ plan.cpp
struct HostT {  // one tensor of a weight blob
    std::vector<int64_t> dims;
    std::vector<float> v;
};
using Blob = std::unordered_map<std::string, HostT>;
// Parses an FRW1 weight blob; touches no handle.
int parse_blob(const void* blob, size_t n, Blob& out);
// Runs the builder of h->arch on a cleared handle: its tensors, ops, conv weights and fused stages (the head's
// weights join W under a conv's name).  Returns the builder's status; on failure the caller frees what was built.
int build_plan(fr_handle* h, Blob& W);

// ------------------------------------------------------------------ gallery_api.cpp
// fr_match_topk under the handle's lock, which the caller holds (fr_embed_match).
int match_locked(fr_handle* h, const float* P, int B, int k, float* scores, int32_t* idx, void* stream);

// ------------------------------------------------------------------ stages.cpp
// Runs the kind's weight packer on a record whose members are in place (Builder::close_stage).
int pack_stage(fr_handle* h, StageRec& r);
// Device pointer table of the stages' intermediate tensors (filled after every activation reserve).
int fill_stage_dbg(fr_handle* h);
// Per stage, whether it (1) or its member ops (0) run in a forward at batch B.
std::vector<char> stage_plan(const fr_handle* h, int B);
// Whether a forward at batch B runs a split stage (its parts wait for each other).
bool split_runs(const fr_handle* h, int B);
// The measured choice of stage `st` at batch B: 1 fused, 0 members, -1 not measured yet.
int stage_choice(const fr_handle* h, int st, int B);
// Whether the stage reads the forward's u8 crops itself (the preparation op is then skipped).
bool stage_takes_u8(const StageRec& r);
int run_stage(fr_handle* h, const Op& op, int B, int f16, const std::vector<char>& stage_run, hipStream_t s);
int measure_stage(fr_handle* h, const Op& op, int B, int f16, const std::vector<char>& stage_run, hipStream_t s);
// fr_debug_plan's line of a stage op.
std::string stage_plan_line(const fr_handle* h, const Op& op, int B);

// ------------------------------------------------------------------ convs.cpp
// Whether kernel choices are measured per shape and batch size (FR_AB autotune, default on).
bool autotune_enabled();
// Packs, at load time, the operands of every specialised kernel that applies to a conv of the plan.
int pack_conv_weights(fr_handle* h);
// One conv op: its ConvArgs from the plan's tensors and weights, then the kernel choice and the launch.
int run_conv_op(fr_handle* h, const Op& op, int B, int f16, hipStream_t s);
// fr_debug_plan's line of a conv or head op.
std::string conv_plan_line(const fr_handle* h, const Op& op, int B);
// The op API (fr_op_conv2d_ex), by descriptor tile id (0 = automatic, 1 + FR_TILE_*): whether the id names an
// implicit-GEMM tile; the extension fields its kernel takes, and the kernels that take a field (for the refusal);
// whether a specialised kernel claims it, and that kernel's checked launch on the caller's [Npad][Kpad] rows.
enum { CONV_TAKES_X2 = 1, CONV_TAKES_Y_BF16 = 2, CONV_TAKES_SPLITK_CNT = 4 };
bool op_tile_is_igemm(int tile);
int op_tile_takes(int tile);
std::string conv_takers(int field);
bool op_tile_forced_kind(int tile);
int run_forced_kind(int tile, ConvArgs& a, int split, hipStream_t s);

}  // namespace fr

#pragma GCC visibility pop
