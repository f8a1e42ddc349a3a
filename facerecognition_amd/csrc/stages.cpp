// frhip fused stages: one launch that replaces a run of member ops of a forward plan and is measured against them
// per batch size.  This file holds what the engine knows about each kind (StageKind): the table of its fixed
// facts, its weight packer, its launch, and the rules for when it runs.  The arch builders (plan.cpp) emit the
// stage ops and their members; DESIGN.md "Fused stage kinds" lists the steps to add a kind.
#include <algorithm>
#include <cstdio>

#include "engine_internal.h"

namespace fr {

// ------------------------------------------------------------------ the kinds
// The work model: per image `pix` output pixels, per unit (a block; a conv of STAGE_LDS) one N x K GEMM row per
// pixel.  run_stage's FLOPs and fr_debug_plan's M N K columns both come from it (stage_work).
struct StageKindDesc {
    const char* name;        // in error messages
    int mask_bit;            // FR_OPT_FUSED_MASK (include/frhip.h)
    const char* ab_off[2];   // FR_AB keys that turn the kind off (A/B timing: the member ops always run)
    const char* ab_off_split;  // ... and one that turns off its multi-workgroup form: = 1, or = the layer's H
    bool keeps_inter;        // writes its members' tensors: can run under FR_OPT_KEEP_INTERMEDIATES
    bool no_amax;            // records no amax: cannot run when an e4m3 conv reads its output
    bool takes_u8;           // reads the forward's u8 crops itself
    bool per_block;          // one launch per block
    const char* cls;         // profiling class (STAGE_LDS, STAGE_BNECK28: stage_class)
    const char* label;       // plan line
    const char* ksize;
    int pix, N, K;           // pix = 0: from the record (stage_work)
    int K_ds;                // K of a first block with a K-concatenated downsample (StageRec::bn_ds)
};

static const StageKindDesc kinds[STAGE_NKINDS] = {
    // N x K per pixel: two 3x3 C -> C convs per block (from the record)
    /* STAGE_LDS       */ {"stage", 1, {nullptr, nullptr}, "no_split_stage", true, false, false, false, nullptr, "stage", "3x3", 0, 0, 0, 0},
    // conv1 at 112^2 (4 x 576 per output pixel) + conv2 with the downsample (640)
    /* STAGE_TRANS     */ {"transition", 1, {"no_trans", nullptr}, nullptr, false, true, false, false, "trans layer1.0", "trans", "3x3", 3136, 64, 2944, 0},
    // per face: 79^2 x 32 x 72 + 77^2 x 32 x 288 + 77^2 x 64 x 288 + 38^2 x 80 x 64 MACs
    /* STAGE_STEM160   */ {"stem160", 2, {"no_stem160", nullptr}, nullptr, false, false, true, false, "stem160", "stem160", "3x3", 1, 1, 185697536, 0},
    // per block and pixel: 256 x 96 + 3 x 288 x 32 + 96 x 256 = 76,800 MACs
    /* STAGE_CHAIN35   */ {"chain35", 4, {"no_chain", "no_chain35"}, nullptr, false, false, false, false, "chain block35", "chain", "3x3", 289, 256, 300, 0},
    // 896 x 256 (branch1.0 + branch0) + 2 x 896 x 128 (1x7, 7x1) + 256 x 896 = 688,128 MACs
    /* STAGE_CHAIN17   */ {"chain", 8, {"no_chain", "no_chain17"}, nullptr, false, false, false, false, "chain block17", "chain", "1x1", 64, 896, 768, 0},
    // 1024 x 256 + 2304 x 256 + 256 x 1024 = 1,114,112 MACs
    /* STAGE_CHAIN_R50 */ {"chain_r50", 16, {"no_chain", "no_chain50"}, nullptr, false, false, false, false, "chain r50 layer3", "chain", "3x3", 49, 1024, 1088, 0},
    // 256 x 64 + 576 x 64 + 64 x 256 = 69,632 MACs; layer1.0: 64 x 64 + 576 x 64 + 128 x 256 = 73,728
    /* STAGE_BNECK28   */ {"bneck28", 32, {"no_chain", "no_bneck28"}, nullptr, false, false, false, true, nullptr, "chain", "3x3", 784, 256, 272, 288},
    // the 7x7 conv: K = 49 x 8 input channels
    /* STAGE_STEM_R50  */ {"stem_r50", 64, {"no_chain", "no_stem_r50"}, nullptr, false, false, true, false, "stem r50", "chain", "7x7", 3136, 64, 392, 0},
};

struct StageWork {
    int pix, N, K, units;
};

// The work of launch i of the stage (i < 0: of the whole op, as its plan line states it).
static StageWork stage_work(const StageRec& r, int i) {
    const StageKindDesc& d = kinds[r.kind];
    StageWork w = {d.pix, d.N, d.K, r.nblk};
    if (!d.pix) w = {r.H * r.H, r.C, 9 * r.C, 2 * r.nblk};
    if (d.per_block && i >= 0) {
        w.units = 1;
        if (r.bn_ds && i == 0) w.K = d.K_ds;
    }
    return w;
}

// Algorithmic HBM bytes of launch i: the input and output activations (2 B) and the weights once.
static double stage_bytes(const fr_handle* h, const StageRec& r, const StageWork& w, int B, int i) {
    const double in_px = h->fwd_u8 ? 3.0 : 16.0;  // a stem's input per pixel: u8 RGB or the prepared 8 channels
    switch (r.kind) {
        case STAGE_TRANS: return 2.0 * B * (12544.0 + 3136.0) * 64 + 2.0 * 64 * (576 + 640);
        case STAGE_STEM160: return (double)B * (in_px * 160 * 160 + 2.0 * 38 * 38 * 80);
        case STAGE_STEM_R50: return (double)B * (112.0 * 112 * in_px + 28.0 * 28 * 64 * 2);
        case STAGE_BNECK28: return 2.0 * B * w.pix * ((r.bn_ds && i == 0 ? 64.0 : 256.0) + w.N) + 2.0 * w.N * w.K;
        default: return 2.0 * 2.0 * B * w.pix * w.N + (r.fp8 ? 1.0 : 2.0) * w.N * w.K * w.units;
    }
}

static const char* stage_class(const StageRec& r, int i) {
    switch (r.kind) {
        case STAGE_LDS: return r.fp8 ? "stage8 layer3" : r.H == 14 ? "stage layer3" : r.H == 28 ? "stage layer2" : "stage layer1";
        case STAGE_BNECK28: return r.bn_ds && i == 0 ? "bneck28 layer1.0" : "bneck28 layer1";
        default: return kinds[r.kind].cls;
    }
}

bool stage_takes_u8(const StageRec& r) { return kinds[r.kind].takes_u8; }

// The FR_AB off-switches, read once per process.
static bool kind_enabled(const StageRec& r) {
    static const std::vector<int> off = [] {
        std::vector<int> v;  // per kind: any of its keys is set; then per kind: its split key's value
        for (const auto& d : kinds) v.push_back((d.ab_off[0] && ab_int(d.ab_off[0], 0)) || (d.ab_off[1] && ab_int(d.ab_off[1], 0)));
        for (const auto& d : kinds) v.push_back(d.ab_off_split ? ab_int(d.ab_off_split, 0) : 0);
        return v;
    }();
    const int split_off = off[STAGE_NKINDS + r.kind];
    return !off[r.kind] && !(r.parts > 1 && (split_off == 1 || split_off == r.H));
}

// ------------------------------------------------------------------ weight packers
// Packs an LDS-resident stage's weights (from the member convs' [Npad][Kpad] device images) and its epilogue table.
static int build_stage(fr_handle* h, StageRec& r) {
    const int nconv = 2 * r.nblk, C = r.C;
    const int ntail = r.tail_op >= 0 ? 2 : 0;  // the tail's two 256-channel halves follow the blocks' convs
    const int nall = nconv + ntail;
    const size_t wbytes = r.fp8 ? 0 : (r.parts > 1 ? split_stage_weight_bytes(C, nall) : stage_weight_bytes(nall));
    std::vector<bf16_t> packed(wbytes / sizeof(bf16_t));
    std::vector<uint8_t> packed8(r.fp8 ? stage8_weight_bytes(nconv) : 0);
    std::vector<float> wsc(r.fp8 ? (size_t)nconv * C : 0);
    std::vector<StageConv> tab(nconv);
    std::vector<float> ep((size_t)nall * 9 * C, 0.f), sl((size_t)nall * C, 0.f);
    const size_t per = packed.size() / nall;
    for (int c = 0; c < nconv; ++c) {
        const Op& op = h->ops[r.conv_ops[c]];
        const DevConvW& cw = h->convw[op.wi];
        if (cw.Cout != C || cw.Npad < C || cw.Kh != 3 || cw.Kw != 3 || cw.Cin != C) {
            set_error("plan: stage member conv is not 3x3 " + std::to_string(C) + "->" + std::to_string(C));
            return FR_ERR_ARG;
        }
        // the stage kernel's epilogues are specialised: conv1 = bias + PReLU, conv2 = bias + identity
        if ((c % 2 == 0 && (op.act != ACT_PRELU || !cw.slope)) || (c % 2 == 1 && (op.act != ACT_NONE || op.res < 0))) {
            set_error("plan: stage member conv has an unexpected activation / residual");
            return FR_ERR_ARG;
        }
        if (r.fp8) {
            if (!cw.w8 || !cw.wscale || cw.Kpad8 != 9 * C || C != 256) {
                set_error("plan: fp8 stage member conv without e4m3 weights");
                return FR_ERR_ARG;
            }
            std::vector<uint8_t> rows8((size_t)cw.Npad * cw.Kpad8);
            FR_HIP_CHECK(hipMemcpy(rows8.data(), cw.w8, rows8.size(), hipMemcpyDeviceToHost));
            stage8_pack_weights(rows8.data(), cw.Kpad8, packed8.data() + (size_t)c * (packed8.size() / nconv));
            FR_HIP_CHECK(hipMemcpy(wsc.data() + (size_t)c * C, cw.wscale, C * sizeof(float), hipMemcpyDeviceToHost));
        } else {
            std::vector<bf16_t> rows((size_t)cw.Npad * cw.Kpad);
            FR_HIP_CHECK(hipMemcpy(rows.data(), cw.w, rows.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
            if (r.parts > 1) split_stage_pack_weights(rows.data(), cw.Kpad, C, packed.data() + c * per);
            else stage_pack_weights(rows.data(), cw.Kpad, C, packed.data() + c * per);
        }
        tab[c].bias = cw.bias9 ? nullptr : cw.bias;
        tab[c].bias9 = cw.bias9;
        tab[c].slope = cw.slope;
        tab[c].act = op.act;
        // the epilogue's per-class bias: bias9 (which already carries the whole bias) or bias x 9
        // (bias9 rows are Npad apart)
        float* e = ep.data() + (size_t)c * 9 * C;
        if (cw.bias9) {
            for (int k = 0; k < 9; ++k)
                FR_HIP_CHECK(hipMemcpy(e + k * C, cw.bias9 + (size_t)k * cw.Npad, C * sizeof(float), hipMemcpyDeviceToHost));
        } else if (cw.bias) {
            FR_HIP_CHECK(hipMemcpy(e, cw.bias, C * sizeof(float), hipMemcpyDeviceToHost));
            for (int k = 1; k < 9; ++k) std::copy(e, e + C, e + k * C);
        }
        // negative-side factor of the activation: PReLU slope, 0 for ReLU, 1 for none
        float* f = sl.data() + (size_t)c * C;
        if (op.act == ACT_PRELU && cw.slope)
            FR_HIP_CHECK(hipMemcpy(f, cw.slope, C * sizeof(float), hipMemcpyDeviceToHost));
        else
            std::fill(f, f + C, op.act == ACT_RELU ? 0.f : 1.f);
    }
    if (ntail) {  // rows [C half, C half + C) of the tail conv (3x3 C -> 2C): bias9 halves, PReLU slopes
        const Op& op = h->ops[r.tail_op];
        const DevConvW& cw = h->convw[op.wi];
        std::vector<bf16_t> rows((size_t)cw.Npad * cw.Kpad);
        FR_HIP_CHECK(hipMemcpy(rows.data(), cw.w, rows.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
        std::vector<float> b9((size_t)9 * cw.Npad, 0.f), slope(cw.Cout);
        if (cw.bias9) {
            FR_HIP_CHECK(hipMemcpy(b9.data(), cw.bias9, b9.size() * sizeof(float), hipMemcpyDeviceToHost));
        } else if (cw.bias) {
            FR_HIP_CHECK(hipMemcpy(b9.data(), cw.bias, cw.Npad * sizeof(float), hipMemcpyDeviceToHost));
            for (int k = 1; k < 9; ++k) std::copy(b9.begin(), b9.begin() + cw.Npad, b9.begin() + (size_t)k * cw.Npad);
        }
        FR_HIP_CHECK(hipMemcpy(slope.data(), cw.slope, cw.Cout * sizeof(float), hipMemcpyDeviceToHost));
        for (int hf = 0; hf < 2; ++hf) {
            const int c = nconv + hf;
            if (r.parts > 1) split_stage_pack_weights(rows.data() + (size_t)hf * C * cw.Kpad, cw.Kpad, C, packed.data() + c * per);
            else stage_pack_weights(rows.data() + (size_t)hf * C * cw.Kpad, cw.Kpad, C, packed.data() + c * per);
            for (int k = 0; k < 9; ++k)
                std::copy(b9.begin() + (size_t)k * cw.Npad + hf * C, b9.begin() + (size_t)k * cw.Npad + hf * C + C,
                          ep.begin() + ((size_t)c * 9 + k) * C);
            std::copy(slope.begin() + hf * C, slope.begin() + hf * C + C, sl.begin() + (size_t)c * C);
        }
    }
    int rc = r.fp8 ? upload(h, &r.w8, packed8) : upload(h, &r.w, packed);
    if (rc) return rc;
    if (r.fp8 && (rc = upload(h, &r.wscale, wsc))) return rc;
    rc = upload(h, &r.table, tab);
    if (rc) return rc;
    if ((rc = upload(h, &r.ep, ep))) return rc;
    if ((rc = upload(h, &r.slope, sl))) return rc;
    void* d = nullptr;
    if ((rc = dev_alloc(&d, (size_t)nconv * sizeof(bf16_t*)))) return rc;
    h->weight_allocs.push_back(d);
    r.dbg = (bf16_t**)d;
    if (r.parts > 1 && !h->stage_spin) {
        if ((rc = dev_alloc(&d, sizeof(int)))) return rc;
        h->weight_allocs.push_back(d);
        h->stage_spin = (int*)d;
        FR_HIP_CHECK(hipMemset(h->stage_spin, 0, sizeof(int)));
    }
    return FR_OK;
}

int fill_stage_dbg(fr_handle* h) {
    for (auto& r : h->stages) {
        if (!kinds[r.kind].keeps_inter) continue;  // no intermediates: the member ops run when they are kept
        std::vector<bf16_t*> p(2 * r.nblk);
        for (int i = 0; i < r.nblk; ++i) {
            p[i] = h->tensors[r.x_tensors[i]].dev;
            p[r.nblk + i] = h->tensors[r.t_tensors[i]].dev;
        }
        FR_HIP_CHECK(hipMemcpy(r.dbg, p.data(), p.size() * sizeof(bf16_t*), hipMemcpyHostToDevice));
    }
    return FR_OK;
}

// Packs a fused transition block (conv_trans.hip) from its member convs' device weights.
static int build_trans(fr_handle* h, StageRec& r) {
    const DevConvW& c1 = h->convw[h->ops[r.conv_ops[0]].wi];
    const DevConvW& c2 = h->convw[h->ops[r.conv_ops[1]].wi];
    if (c1.K != 576 || c2.K != 640 || c2.K1 != 576 || c2.C2 != 64 || c1.Cout != 64 || c2.Cout != 64 || !c1.slope ||
        (!c1.bias9 && !c1.bias) || !c2.bias) {
        set_error("plan: transition block members do not match the fused kernel");
        return FR_ERR_ARG;
    }
    void* q = nullptr;
    int rc = dev_alloc(&q, trans_packed_elems(c1.K) * sizeof(bf16_t));
    if (rc) return rc;
    h->weight_allocs.push_back(q);
    r.tw1 = (bf16_t*)q;
    if ((rc = dev_alloc(&q, trans_packed_elems(c2.K) * sizeof(bf16_t)))) return rc;
    h->weight_allocs.push_back(q);
    r.tw2 = (bf16_t*)q;
    FR_HIP_CHECK(trans_pack_weights(c1.w, c1.Kpad, c1.K, r.tw1, 0));
    FR_HIP_CHECK(trans_pack_weights(c2.w, c2.Kpad, c2.K, r.tw2, 0));
    FR_HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> ep(9 * 64), sl(64), b2(64);
    if (c1.bias9) {
        for (int k = 0; k < 9; ++k)
            FR_HIP_CHECK(hipMemcpy(ep.data() + k * 64, c1.bias9 + (size_t)k * c1.Npad, 64 * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        FR_HIP_CHECK(hipMemcpy(ep.data(), c1.bias, 64 * sizeof(float), hipMemcpyDeviceToHost));
        for (int k = 1; k < 9; ++k) std::copy(ep.begin(), ep.begin() + 64, ep.begin() + k * 64);
    }
    FR_HIP_CHECK(hipMemcpy(sl.data(), c1.slope, 64 * sizeof(float), hipMemcpyDeviceToHost));
    FR_HIP_CHECK(hipMemcpy(b2.data(), c2.bias, 64 * sizeof(float), hipMemcpyDeviceToHost));
    if ((rc = upload(h, &r.tep1, ep))) return rc;
    if ((rc = upload(h, &r.tsl1, sl))) return rc;
    return upload(h, &r.tb2, b2);
}

// The chain packers' common opening: member k of block blk (`per` members per block), checked to be a bf16 / f16
// conv + bias + ReLU, with host copies of its [Npad][Kpad] weight rows and its Cout biases.
struct ChainMember {
    const Op* op;
    const DevConvW* cw;
    std::vector<bf16_t> rows;
    std::vector<float> bias;
};

static int chain_member(fr_handle* h, const StageRec& r, int per, int blk, int k, ChainMember& m) {
    const std::string name = kinds[r.kind].name;
    if ((int)r.conv_ops.size() != per * r.nblk) {
        set_error("plan: " + name + " member count");
        return FR_ERR_ARG;
    }
    m.op = &h->ops[r.conv_ops[per * blk + k]];
    if (m.op->kind == OP_CONV) m.cw = &h->convw[m.op->wi];
    if (m.op->kind != OP_CONV || m.cw->w8 || !m.cw->bias || m.cw->bias9 || m.op->act != ACT_RELU) {
        set_error("plan: " + name + " member conv is not bf16 / f16 + bias + ReLU");
        return FR_ERR_ARG;
    }
    m.rows.resize((size_t)m.cw->Npad * m.cw->Kpad);
    FR_HIP_CHECK(hipMemcpy(m.rows.data(), m.cw->w, m.rows.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
    m.bias.resize(m.cw->Cout);
    FR_HIP_CHECK(hipMemcpy(m.bias.data(), m.cw->bias, m.bias.size() * sizeof(float), hipMemcpyDeviceToHost));
    return FR_OK;
}

// ... and their common closing
static int chain_upload(fr_handle* h, StageRec& r, const std::vector<bf16_t>& packed, const std::vector<float>& bias) {
    const int rc = upload(h, &r.cw, packed);
    return rc ? rc : upload(h, &r.cbias, bias);
}

static int bad_shapes(const char* what) {
    set_error(std::string("plan: ") + what);
    return FR_ERR_ARG;
}

// Packs IRV1 repeat_2's member convs (per block: branch1.0 + branch0 as one 1x1 896 -> 256, the 1x7 and 7x1
// 128 -> 128, conv2d 256 -> 896 with the residual) into conv_chain.hip's per-wave streams and bias table.
static int build_chain17(fr_handle* h, StageRec& r) {
    const int nblk = r.nblk;
    std::vector<bf16_t> packed(chain17_weight_elems(nblk));
    std::vector<float> bias(chain17_bias_floats(nblk), 0.f);
    for (int blk = 0; blk < nblk; ++blk) {
        ChainMember m[4];
        const Op* op[4];
        const DevConvW* cw[4];
        for (int k = 0; k < 4; ++k) {
            if (int rc = chain_member(h, r, 4, blk, k, m[k])) return rc;
            op[k] = m[k].op;
            cw[k] = m[k].cw;
        }
        const bool shapes = cw[0]->Cout == 256 && cw[0]->K == 896 && cw[0]->Kh == 1 && cw[0]->Kw == 1 &&
                            cw[1]->Cout == 128 && cw[1]->K == 896 && cw[1]->Kh == 1 && cw[1]->Kw == 7 &&
                            cw[2]->Cout == 128 && cw[2]->K == 896 && cw[2]->Kh == 7 && cw[2]->Kw == 1 &&
                            cw[3]->Cout == 896 && cw[3]->K == 256 && cw[3]->Kh == 1 && cw[3]->Kw == 1 &&
                            op[3]->res >= 0 && op[3]->res_off == 0 && op[0]->res < 0 && op[1]->res < 0 && op[2]->res < 0;
        if (!shapes) return bad_shapes("chain member convs do not have Block17's shapes");
        chain17_pack_block(m[0].rows.data(), cw[0]->Kpad, m[1].rows.data(), cw[1]->Kpad, m[2].rows.data(), cw[2]->Kpad,
                           m[3].rows.data(), cw[3]->Kpad, blk, nblk, packed.data());
        // [A = branch1.0 | B = 1x7 | C = 7x1 | D = branch0 | E = conv2d]
        float* t = bias.data() + (size_t)blk * 1408;
        std::copy(m[0].bias.begin(), m[0].bias.begin() + 128, t);
        std::copy(m[1].bias.begin(), m[1].bias.end(), t + 128);
        std::copy(m[2].bias.begin(), m[2].bias.end(), t + 256);
        std::copy(m[0].bias.begin() + 128, m[0].bias.end(), t + 384);
        std::copy(m[3].bias.begin(), m[3].bias.end(), t + 512);
    }
    return chain_upload(h, r, packed, bias);
}

// Packs ResNet-50 layer3.1 .. layer3.5's member convs (per block: conv1 1x1 1024 -> 256, conv2 3x3 256 -> 256,
// conv3 1x1 256 -> 1024 with the residual; BN folded, each + bias + ReLU) into conv_chain_r50.hip's per-wave streams.
// Members without the kernel's shapes fail the load (no fall-back to the member ops).
static int build_chain_r50(fr_handle* h, StageRec& r) {
    const int nblk = r.nblk;
    std::vector<bf16_t> packed(chain_r50_weight_elems(nblk));
    std::vector<float> bias(chain_r50_bias_floats(nblk), 0.f);
    for (int blk = 0; blk < nblk; ++blk) {
        ChainMember m[3];
        const Op* op[3];
        const DevConvW* cw[3];
        for (int k = 0; k < 3; ++k) {
            if (int rc = chain_member(h, r, 3, blk, k, m[k])) return rc;
            op[k] = m[k].op;
            cw[k] = m[k].cw;
        }
        const bool shapes = cw[0]->Cout == 256 && cw[0]->K == 1024 && cw[0]->Kh == 1 && cw[0]->Kw == 1 &&
                            cw[1]->Cout == 256 && cw[1]->K == 2304 && cw[1]->Kh == 3 && cw[1]->Kw == 3 &&
                            op[1]->sh == 1 && op[1]->ph == 1 && op[1]->pw == 1 &&
                            cw[2]->Cout == 1024 && cw[2]->K == 256 && cw[2]->Kh == 1 && cw[2]->Kw == 1 &&
                            op[2]->res >= 0 && op[2]->res_off == 0 && op[0]->res < 0 && op[1]->res < 0;
        if (!shapes) return bad_shapes("chain_r50 member convs do not have layer3's Bottleneck shapes");
        chain_r50_pack_block(m[0].rows.data(), cw[0]->Kpad, m[1].rows.data(), cw[1]->Kpad, m[2].rows.data(), cw[2]->Kpad,
                             blk, nblk, packed.data());
        float* t = bias.data() + chain_r50_bias_floats(1) * blk;  // [conv1 256 | conv2 256 | conv3 1024]
        std::copy(m[0].bias.begin(), m[0].bias.end(), t);
        std::copy(m[1].bias.begin(), m[1].bias.end(), t + 256);
        std::copy(m[2].bias.begin(), m[2].bias.end(), t + 512);
    }
    return chain_upload(h, r, packed, bias);
}

// Packs ResNet-50 layer1.1 / layer1.2's member convs (conv1 1x1 256 -> 64, conv2 3x3 64 -> 64, conv3 1x1 64 -> 256
// with the residual; BN folded, each + bias + ReLU) into conv_bneck28.hip's per-quarter register images.
// Members without the kernel's shapes fail the load (no fall-back to the member ops).
static int build_bneck28(fr_handle* h, StageRec& r) {
    const int nblk = r.nblk;
    if ((int)r.x_tensors.size() != nblk) return bad_shapes("bneck28 member count");
    std::vector<bf16_t> packed(bneck28_block_elems(false) * nblk + (r.bn_ds ? bneck28_block_elems(true) - bneck28_block_elems(false) : 0));
    std::vector<float> bias((size_t)nblk * 384, 0.f);
    size_t w_off = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        const bool ds = r.bn_ds && blk == 0;
        ChainMember m[3];
        const Op* op[3];
        const DevConvW* cw[3];
        for (int k = 0; k < 3; ++k) {
            if (int rc = chain_member(h, r, 3, blk, k, m[k])) return rc;
            op[k] = m[k].op;
            cw[k] = m[k].cw;
        }
        const bool common = cw[0]->Cout == 64 && cw[0]->K == (ds ? 64 : 256) && cw[0]->Kh == 1 && cw[0]->Kw == 1 &&
                            cw[1]->Cout == 64 && cw[1]->K == 576 && cw[1]->Kh == 3 && cw[1]->Kw == 3 &&
                            op[1]->sh == 1 && op[1]->ph == 1 && op[1]->pw == 1 && cw[2]->Cout == 256 &&
                            cw[2]->Kh == 1 && cw[2]->Kw == 1 && op[0]->res < 0 && op[1]->res < 0 && op[0]->in_off == 0;
        // layer1.0: conv3's K = [t2 64 | maxpool output 64] at stride 1, no residual; 1.1 / 1.2: K 64 + the residual x
        const bool shapes = common && (ds ? cw[2]->K == 128 && cw[2]->K1 == 64 && cw[2]->C2 == 64 && op[2]->x2 == op[0]->in &&
                                                op[2]->x2_off == 0 && op[2]->st2 == 1 && op[2]->res < 0
                                          : cw[2]->K == 64 && op[2]->x2 < 0 && op[2]->res == op[0]->in && op[2]->res_off == 0);
        if (!shapes) return bad_shapes("bneck28 member convs do not have layer1's Bottleneck shapes");
        bneck28_pack_block(m[0].rows.data(), cw[0]->Kpad, m[1].rows.data(), cw[1]->Kpad, m[2].rows.data(), cw[2]->Kpad, ds,
                           packed.data() + w_off);
        w_off += bneck28_block_elems(ds);
        float* t = bias.data() + 384 * blk;  // [conv1 64 | conv2 64 | conv3 256]
        std::copy(m[0].bias.begin(), m[0].bias.end(), t);
        std::copy(m[1].bias.begin(), m[1].bias.end(), t + 64);
        std::copy(m[2].bias.begin(), m[2].bias.end(), t + 128);
    }
    return chain_upload(h, r, packed, bias);
}

// Packs IRV1 repeat_1's member convs (per block: branch1.0 + branch2.0 + branch0 as one 1x1 256 -> 96, branch1.1,
// branch2.1, branch2.2 3x3 32 -> 32, conv2d 96 -> 256 with the residual) for conv_chain35.hip.
static int build_chain35(fr_handle* h, StageRec& r) {
    const int nblk = r.nblk;
    if ((int)r.x_tensors.size() != nblk) return bad_shapes("chain35 member count");
    std::vector<bf16_t> packed(chain35_weight_elems(nblk));
    std::vector<float> bias(chain35_bias_floats(nblk), 0.f);
    for (int blk = 0; blk < nblk; ++blk) {
        ChainMember m[5];
        const Op* op[5];
        const DevConvW* cw[5];
        for (int k = 0; k < 5; ++k) {
            if (int rc = chain_member(h, r, 5, blk, k, m[k])) return rc;
            op[k] = m[k].op;
            cw[k] = m[k].cw;
        }
        bool shapes = cw[0]->Cout == 96 && cw[0]->K == 256 && cw[0]->Kh == 1 && cw[4]->Cout == 256 && cw[4]->K == 96 &&
                      cw[4]->Kh == 1 && op[4]->res >= 0 && op[4]->res_off == 0;
        for (int k = 1; k <= 3; ++k)
            shapes = shapes && cw[k]->Cout == 32 && cw[k]->K == 288 && cw[k]->Kh == 3 && cw[k]->Kw == 3 && op[k]->ph == 1 &&
                     op[k]->pw == 1 && op[k]->sh == 1 && op[k]->res < 0;
        if (!shapes) return bad_shapes("chain35 member convs do not have Block35's shapes");
        chain35_pack_block(m[0].rows.data(), cw[0]->Kpad, m[1].rows.data(), cw[1]->Kpad, m[2].rows.data(), cw[2]->Kpad,
                           m[3].rows.data(), cw[3]->Kpad, m[4].rows.data(), cw[4]->Kpad, blk, packed.data());
        chain35_pack_bias(m[0].bias.data(), m[1].bias.data(), m[2].bias.data(), m[3].bias.data(), m[4].bias.data(), blk,
                          bias.data());
    }
    return chain_upload(h, r, packed, bias);
}

int pack_stage(fr_handle* h, StageRec& r) {
    switch (r.kind) {
        case STAGE_LDS: return build_stage(h, r);
        case STAGE_TRANS: return build_trans(h, r);
        case STAGE_CHAIN35: return build_chain35(h, r);
        case STAGE_CHAIN17: return build_chain17(h, r);
        case STAGE_CHAIN_R50: return build_chain_r50(h, r);
        case STAGE_BNECK28: return build_bneck28(h, r);
        default: return FR_OK;  // the stems read their member convs' [Npad][Kpad] rows as they are
    }
}

// ------------------------------------------------------------------ when a stage runs
int stage_choice(const fr_handle* h, int st, int B) {
    for (const auto& m : h->stage_meas)
        if (m.stage == st && m.B == B) return m.run;
    return -1;
}

// Whether stage `st` runs at batch B.  The options and the kind's rules first (a kind that keeps no intermediates or
// records no amax leaves those forwards to its member ops); then, in auto mode, the measurement at this batch size
// (measure_stage).  Unmeasured, the fill rule of the LDS-resident stages decides: such a kernel puts one image on
// one CU (a split stage on `parts` CUs: a round is n_cu / parts images).  Up to one round it beats the per-conv
// launches at every batch size (tools/batch_sweep.py, profiles/r02_batch_sweep.jsonl: B = 1 3.76 vs 3.88 ms,
// B = 128 5.39 vs 5.73 ms): a small batch leaves CUs idle either way, since per-conv grids of B*196 positions are a
// handful of tiles.  Above one round a last round that is mostly empty costs a whole stage time, so auto mode then
// requires the rounds to be at least stage_min_fill % full (B = 512: 100 %, B = 257: 50 % -> per-conv).
static bool stage_runs(const fr_handle* h, int B, const StageRec& r, int st) {
    const StageKindDesc& d = kinds[r.kind];
    if (h->stage_mode == 0 || h->invariant) return false;
    if (!(h->fused_mask & d.mask_bit)) return false;
    if (h->keep_inter && !d.keeps_inter) return false;
    if (d.no_amax && h->amax && h->need_amax[r.out]) return false;
    if (!kind_enabled(r) || (r.parts > 1 && h->no_split)) return false;
    if (h->stage_mode == 1) {  // measured at this batch size (measure_stage)
        const int c = stage_choice(h, st, B);
        if (c >= 0) return c == 1;
    }
    const int cap = std::max(1, h->n_cu / r.parts);
    if (h->stage_mode == 2 || B <= cap) return true;
    const int64_t rounds = (B + cap - 1) / cap;
    return (int64_t)B * 100 >= (int64_t)h->stage_min_fill * rounds * cap;
}

std::vector<char> stage_plan(const fr_handle* h, int B) {
    std::vector<char> run(h->stages.size());
    for (size_t i = 0; i < h->stages.size(); ++i) run[i] = stage_runs(h, B, h->stages[i], (int)i);
    return run;
}

bool split_runs(const fr_handle* h, int B) {
    for (size_t i = 0; i < h->stages.size(); ++i)
        if (h->stages[i].parts > 1 && stage_runs(h, B, h->stages[i], (int)i)) return true;
    return false;
}

// ------------------------------------------------------------------ launches
// One function per kind: fills the kernel's args struct and launches (launch i of the stage).
static hipError_t run_lds(fr_handle* h, const Op& op, const StageRec& r, int B, int f16, bool tail_in, hipStream_t s) {
    StageArgs a{};
    a.x = h->tensors[r.in].dev;
    a.y = h->tensors[r.out].dev;
    a.w = r.w;
    a.conv = r.table;
    a.ep = r.ep;
    a.slope = r.slope;
    if (h->keep_inter) { a.dbg_x = r.dbg; a.dbg_t = r.dbg + r.nblk; }
    a.B = B;
    a.nblk = r.nblk;
    a.f16 = f16;
    a.xchg = h->stage_xchg;
    a.flags = h->stage_flags + (size_t)h->max_batch * 4 * op.stage;  // the stage's own counter region
    a.spin_timeouts = h->stage_spin;
    a.fail_host = h->fail_dev;
    a.spin_limit = h->spin_limit;
    a.variant = h->stage_variant;
    if (tail_in) {
        a.ntail = 2;
        a.y2 = h->tensors[h->ops[r.tail_op].out].dev;
    }
    if (r.fp8) {
        a.w = (const bf16_t*)r.w8;
        a.wscale = r.wscale;
        return launch_stage8(a, s);
    }
    return r.parts > 1 ? launch_split_stage(a, r.H, r.C, s) : launch_stage(a, s);
}

static hipError_t run_trans(fr_handle* h, const StageRec& r, int B, int f16, hipStream_t s) {
    TransArgs t{};
    t.x = h->tensors[r.in].dev;
    t.y = h->tensors[r.out].dev;
    t.w1 = r.tw1; t.w2 = r.tw2; t.ep1 = r.tep1; t.slope1 = r.tsl1; t.b2 = r.tb2;
    t.B = B; t.f16 = f16;
    return launch_trans(t, s);
}

static hipError_t run_stem160(fr_handle* h, const StageRec& r, int B, int f16, hipStream_t s) {
    const DevConvW* cw[4];
    for (int k = 0, j = 0; k < 5; ++k)
        if (h->ops[r.conv_ops[k]].kind == OP_CONV) cw[j++] = &h->convw[h->ops[r.conv_ops[k]].wi];
    Stem160Args a{};
    a.x = h->tensors[r.in].dev;
    a.u8 = h->fwd_u8;  // the crops when the forward skipped the preparation op (forward, OP_PRE)
    a.y = h->tensors[r.out].dev;
    a.w1 = cw[0]->w; a.w2 = cw[1]->w; a.w3 = cw[2]->w; a.w4 = cw[3]->w;
    a.b1 = cw[0]->bias; a.b2 = cw[1]->bias; a.b3 = cw[2]->bias; a.b4 = cw[3]->bias;
    a.kp1 = cw[0]->Kpad; a.kp2 = cw[1]->Kpad; a.kp3 = cw[2]->Kpad; a.kp4 = cw[3]->Kpad;
    a.B = B; a.f16 = f16;
    return launch_stem160(a, s);
}

static hipError_t run_stem_r50(fr_handle* h, const StageRec& r, int B, int f16, hipStream_t s) {
    const DevConvW& cw = h->convw[h->ops[r.conv_ops[0]].wi];
    StemR50Args a{};
    a.x = h->tensors[r.in].dev;
    a.u8 = h->fwd_u8;  // the crops when the forward skipped the preparation op (forward, OP_PRE)
    a.y = h->tensors[r.out].dev;
    a.w = cw.w; a.bias = cw.bias; a.Kpad = cw.Kpad; a.B = B; a.f16 = f16;
    return launch_stem_r50(a, s);
}

static hipError_t run_chain35(fr_handle* h, const StageRec& r, int B, int f16, hipStream_t s) {
    Chain35Args c{};
    c.io[0] = h->tensors[r.in].dev;
    for (int i = 0; i < r.nblk; ++i) c.io[i + 1] = h->tensors[r.x_tensors[i]].dev;
    c.w = r.cw; c.bias = r.cbias; c.B = B; c.nblk = r.nblk; c.f16 = f16;
    return launch_chain35(c, s);
}

// chain17 / chain_r50: the whole chain from r.in to r.out
static Chain17Args chain_args(fr_handle* h, const StageRec& r, int B, int f16) {
    Chain17Args c{};
    c.x = h->tensors[r.in].dev;
    c.y = h->tensors[r.out].dev;
    c.w = r.cw; c.bias = r.cbias; c.B = B; c.nblk = r.nblk; c.f16 = f16;
    return c;
}

static hipError_t run_bneck28(fr_handle* h, const StageRec& r, int B, int f16, int i, hipStream_t s) {
    const bool ds = r.bn_ds && i == 0;
    Chain17Args c{};
    c.B = B; c.nblk = 1; c.f16 = f16;
    c.x = h->tensors[i ? r.x_tensors[i - 1] : r.in].dev;
    c.y = h->tensors[r.x_tensors[i]].dev;
    c.w = r.cw + (i ? bneck28_block_elems(r.bn_ds) + (size_t)(i - 1) * bneck28_block_elems(false) : 0);
    c.bias = r.cbias + 384 * i;
    return launch_bneck28(c, ds, s);
}

// One fused stage (+ the tail conv the legacy LDS kernel leaves out, + the amax pass an e4m3 reader of its output needs).
int run_stage(fr_handle* h, const Op& op, int B, int f16, const std::vector<char>& stage_run, hipStream_t s) {
    const StageRec& r = h->stages[op.stage];
    const int kf16 = f16 || h->tensors[r.in].f16;  // an f16 section of a bf16 plan (build_irv1)
    // the tail conv runs inside the stage kernel, except under the legacy 14-fragment kernel (variant 1), which
    // has no tail: there it runs as its own conv after the stage
    const bool tail_in = r.tail_op >= 0 && (r.parts > 1 || h->stage_variant != 1);
    const int nlaunch = kinds[r.kind].per_block ? r.nblk : 1;
    for (int i = 0; i < nlaunch; ++i) {
        const StageWork w = stage_work(r, i);
        ProfScope ps(h, s);
        ps.flops = 2.0 * B * w.pix * (double)w.N * w.K * w.units;
        ps.bytes = stage_bytes(h, r, w, B, i);
        if (tail_in) {  // + the tail conv: 3x3 C -> 2C at H x H, its 2C-channel output and weights
            ps.flops += 2.0 * B * w.pix * 2.0 * w.N * w.K;
            ps.bytes += 2.0 * B * w.pix * 2.0 * w.N + 2.0 * w.K * 2.0 * w.N;
        }
        ps.start(stage_class(r, i));
        hipError_t e = hipSuccess;
        switch (r.kind) {
            case STAGE_LDS: e = run_lds(h, op, r, B, kf16, tail_in, s); break;
            case STAGE_TRANS: e = run_trans(h, r, B, kf16, s); break;
            case STAGE_STEM160: e = run_stem160(h, r, B, kf16, s); break;
            case STAGE_CHAIN35: e = run_chain35(h, r, B, kf16, s); break;
            case STAGE_CHAIN17: e = launch_chain17(chain_args(h, r, B, kf16), s); break;
            case STAGE_CHAIN_R50: e = launch_chain_r50(chain_args(h, r, B, kf16), s); break;
            case STAGE_BNECK28: e = run_bneck28(h, r, B, kf16, i, s); break;
            case STAGE_STEM_R50: e = run_stem_r50(h, r, B, kf16, s); break;
            case STAGE_NKINDS: e = hipErrorInvalidValue; break;
        }
        FR_HIP_CHECK(e);
    }
    if (r.tail_op >= 0 && !tail_in) {
        const int rc = run_conv_op(h, h->ops[r.tail_op], B, f16, s);
        if (rc) return rc;
    }
    // the stages have no amax epilogue: when a per-conv e4m3 conv reads the stage output (e.g.
    // layer4.0 under FR_FP8_PLAN=all), its activation scale comes from one reduction pass here
    if (h->amax && h->need_amax[r.out] &&
        std::any_of(h->ops.begin(), h->ops.end(), [&](const Op& c) {  // a per-conv e4m3 reader runs
            return c.kind == OP_CONV && c.in == r.out && c.in_off == 0 && c.wi >= 0 && h->convw[c.wi].w8 &&
                   !op_skipped(c, stage_run);
        })) {
        const auto& t = h->tensors[r.out];
        ProfScope pa(h, s);
        pa.bytes = 2.0 * B * t.H * t.W * t.C;
        pa.start("amax");
        FR_HIP_CHECK(launch_amax(t.dev, (size_t)B * t.H * t.W * t.C, f16 || t.f16,
                                 h->amax + (size_t)r.out * FR_AMAX_SLOTS, FR_AMAX_SLOTS, s));
    }
    return FR_OK;
}

// Stage or member launches for a stage's blocks at batch B, measured (FR_OPT_STAGE = 1, the default): in the
// eager tuning forward of a new batch size the member convs run (and tune their kernels), then the member
// sequence and the stage are timed with HIP events, and the faster is kept for B.  The winner runs last, so the
// tuning forward's output equals every later forward's.
int measure_stage(fr_handle* h, const Op& op, int B, int f16, const std::vector<char>& stage_run, hipStream_t s) {
    const std::vector<int>& mem = h->stages[op.stage].conv_ops;
    auto fused = [&]() { return run_stage(h, op, B, f16, stage_run, s); };
    auto members = [&]() {
        for (int oi : mem) {
            const Op& mo = h->ops[oi];
            const int rc = mo.kind == OP_MAXPOOL ? run_maxpool_op(h, mo, B, f16, s) : run_conv_op(h, mo, B, f16, s);
            if (rc) return rc;
        }
        return (int)FR_OK;
    };
    int rc = members();  // tunes the member convs' kernels
    if (!rc) rc = fused();  // warm
    if (rc) return rc;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (auto& e : ev) FR_HIP_CHECK(hipEventCreate(&e));
    float t_conv = 1e30f, t_stage = 1e30f;
    for (int pass = 0; pass < 2 && !rc; ++pass) {  // best of two, interleaved
        FR_HIP_CHECK(hipEventRecord(ev[0], s));
        rc = members();
        FR_HIP_CHECK(hipEventRecord(ev[1], s));
        if (!rc) rc = fused();
        FR_HIP_CHECK(hipEventRecord(ev[2], s));
        FR_HIP_CHECK(hipEventSynchronize(ev[2]));
        float a = 0.f, b = 0.f;
        FR_HIP_CHECK(hipEventElapsedTime(&a, ev[0], ev[1]));
        FR_HIP_CHECK(hipEventElapsedTime(&b, ev[1], ev[2]));
        t_conv = std::min(t_conv, a);
        t_stage = std::min(t_stage, b);
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc) return rc;
    const int run = t_stage <= t_conv ? 1 : 0;
    h->stage_meas.push_back({op.grp, B, run, t_stage, t_conv});
    return run ? FR_OK : members();  // the stage's output is in place; else the per-conv one replaces it
}

// ------------------------------------------------------------------ fr_debug_plan
// "<label> M N K K units 1 <ksize> <output>" + " <fused ms> <members ms>" once measured at batch B (measure_stage)
std::string stage_plan_line(const fr_handle* h, const Op& op, int B) {
    const StageRec& r = h->stages[op.stage];
    const StageKindDesc& d = kinds[r.kind];
    const StageWork w = stage_work(r, -1);
    const std::string K = std::to_string(w.K);
    std::string line = std::string(d.label) + (r.fp8 ? "8 " : " ") + std::to_string(B * w.pix) + " " + std::to_string(w.N) +
                       " " + K + " " + K + " " + std::to_string(w.units) + " 1 " + d.ksize + " " + h->tensors[r.out].name;
    for (const auto& m : h->stage_meas)
        if (m.stage == op.grp && m.B == B) {
            char t[64];
            std::snprintf(t, sizeof t, " %.4f %.4f", m.t_stage, m.t_conv);
            line += t;
            break;
        }
    return line + "\n";
}

}  // namespace fr
