// frhip plans: the weight-blob parser and the static per-arch forward plans.  build_plan() turns a parsed blob into the
// handle's tensors, ops, conv weights and fused stages; engine.cpp (fr_load_weights) calls it and runs the plan.  The
// fused stages of a plan (their kinds, packers, launches) are in stages.cpp, how a conv gets its kernel in convs.cpp.
//
// The forward plans restate the reference backbones as a list of fused ops:
//   FR_ARCH_RESNET50_ARCFACE  models/arcface/arcface_model.py:118-132 + head :192-196
//   FR_ARCH_IRESNET100        insightface iresnet100 (IBasicBlock; README.md:72)
//   FR_ARCH_IRV1_FACENET      facenet_pytorch InceptionResnetV1 (facenet_model.py:12-16)
// BN is folded into the conv weights/bias by the Python importer
// (facerecognition_amd/weights.py); this file only knows tensor names.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "engine_internal.h"

using namespace fr;

// ------------------------------------------------------------------ weight blob
// FRW1 := "FRW1" u32 count { u32 name_len, name, u32 ndim, i64 dims[ndim], f32 data[prod] }*
int fr::parse_blob(const void* blob, size_t n, Blob& out) {
    const uint8_t* p = (const uint8_t*)blob;
    const uint8_t* end = p + n;
    auto need = [&](size_t k) { return (size_t)(end - p) >= k; };
    if (!need(8) || std::memcmp(p, "FRW1", 4) != 0) {
        set_error("weight blob: bad magic (expected FRW1)");
        return FR_ERR_WEIGHTS;
    }
    p += 4;
    uint32_t count;
    std::memcpy(&count, p, 4);
    p += 4;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t nl, nd;
        if (!need(4)) goto trunc;
        std::memcpy(&nl, p, 4);
        p += 4;
        if (!need(nl + 4)) goto trunc;
        {
            std::string name((const char*)p, nl);
            p += nl;
            std::memcpy(&nd, p, 4);
            p += 4;
            if (nd > 8 || !need(8ull * nd)) goto trunc;
            HostT t;
            t.dims.resize(nd);
            std::memcpy(t.dims.data(), p, 8ull * nd);
            p += 8ull * nd;
            size_t cnt = 1;
            for (auto d : t.dims) cnt *= (size_t)d;
            if (!need(4 * cnt)) goto trunc;
            t.v.resize(cnt);
            std::memcpy(t.v.data(), p, 4 * cnt);
            p += 4 * cnt;
            out[name] = std::move(t);
        }
    }
    return FR_OK;
trunc:
    set_error("weight blob: truncated");
    return FR_ERR_WEIGHTS;
}

namespace {

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ------------------------------------------------------------------ plan builder
// One conv of a plan.  names[i].w is [Cout_i, kh, kw, <= cin] f32; several names: one conv over their concatenated
// output channels.  It reads channels [in_off, in_off + cin) of tensor `in` and writes [out_off, out_off + Cout) of `out`,
// after adding the same channels of `res` from res_off (res >= 0).  ds (single name only): a 1x1 conv [Cout, 1, 1, c2]
// of tensor x2 at stride st2 whose weights are appended to every row (K = kh*kw*cin + c2) and whose bias is added: a
// residual block's downsample folded into its last conv.
struct ConvSpec {
    std::vector<std::string> names;
    int in = -1, in_off = 0, cin = 0;
    int out = -1, out_off = 0;
    int kh = 1, kw = 1, sh = 1, sw = 1, ph = 0, pw = 0;
    int act = ACT_NONE;
    int res = -1, res_off = 0;
    std::string ds;
    int x2 = -1, c2 = 0, st2 = 1;
};

// a square kernel k at stride s with pad p
ConvSpec sq(ConvSpec c, int k, int s, int p) {
    c.kh = c.kw = k;
    c.sh = c.sw = s;
    c.ph = c.pw = p;
    return c;
}

// One max-pool of a plan: window k at stride s with pad p over all channels of `in`, written from out_off of `out`.
struct PoolSpec {
    int in = -1;
    int out = -1, out_off = 0;
    int k = 3, s = 2, p = 0;
};

struct Builder {
    fr_handle* h;
    Blob& W;
    int rc = FR_OK;

    // f16: stored as f16 in a bf16 plan (IRV1's f16 section)
    int tensor(int H, int Wd, int C, const std::string& name = "", bool f16 = false) {
        h->tensors.push_back({H, Wd, C, nullptr, name, f16});
        return (int)h->tensors.size() - 1;
    }

    const HostT* find(const std::string& n) {
        auto it = W.find(n);
        return it == W.end() ? nullptr : &it->second;
    }

    bool stem = false;  // next conv is the network stem: fold 1/255 + hi/lo split (see launch_preprocess)

    bool pack_f16 = false;  // the conv being built reads an f16 tensor: f16 weights (set by conv)

    float round16(float v) const {  // stem hi/lo split in the activation dtype (bf16 for FR_DTYPE_FP8)
        return pack_f16 ? host_h2f(host_f2h(v)) : host_bf2f(host_f2bf(v));
    }

    // Packs and uploads the weights of one conv (ConvSpec: names, kh, kw, cin, act, ds, c2); returns its index.
    int make_convw(const ConvSpec& c) {
        const std::vector<std::string>& names = c.names;
        const int kh = c.kh, kw = c.kw, cin = c.cin, c2 = c.c2;
        const std::string& kcat = c.ds;
        const bool stem_split = stem;
        stem = false;
        DevConvW cw;
        cw.Kh = kh;
        cw.Kw = kw;
        cw.Cin = cin;
        cw.K = kh * kw * cin;
        std::vector<float> wrows, bias, slope;
        int cout = 0;
        for (const auto& nm : names) {
            const HostT* w = find(nm + ".w");
            if (!w || w->dims.size() != 4 || w->dims[1] != kh || w->dims[2] != kw || w->dims[3] > cin) {
                set_error("weights: missing or mis-shaped tensor " + nm + ".w");
                rc = FR_ERR_WEIGHTS;
                return -1;
            }
            const int co = (int)w->dims[0], ci = (int)w->dims[3];
            if (stem_split && (ci != 3 || cin != 8)) {
                set_error("plan: stem conv " + nm + " must have 3 input channels");
                rc = FR_ERR_WEIGHTS;
                return -1;
            }
            for (int o = 0; o < co; ++o)
                for (int r = 0; r < kh; ++r)
                    for (int s = 0; s < kw; ++s)
                        for (int ch = 0; ch < cin; ++ch) {
                            if (stem_split) {
                                // input channels are [q, q, 0, 0], q = 255*x: weights [hi, lo, 0, 0] of w/255
                                const float wv = w->v[(((size_t)o * kh + r) * kw + s) * ci + (ch % 3)] / 255.0f;
                                const float hi = round16(wv);
                                wrows.push_back(ch < 3 ? hi : (ch < 6 ? wv - hi : 0.f));
                            } else {
                                wrows.push_back(ch < ci ? w->v[(((size_t)o * kh + r) * kw + s) * ci + ch] : 0.f);
                            }
                        }
            const HostT* b = find(nm + ".b");
            for (int o = 0; o < co; ++o) bias.push_back(b ? b->v[o] : 0.f);
            if (c.act == ACT_PRELU) {
                const HostT* sl = find(nm + ".slope");
                if (!sl) {
                    set_error("weights: missing " + nm + ".slope");
                    rc = FR_ERR_WEIGHTS;
                    return -1;
                }
                for (int o = 0; o < co; ++o) slope.push_back(sl->v[o]);
            }
            cout += co;
        }
        cw.Cout = cout;
        cw.K1 = cw.K;
        if (!kcat.empty()) {
            const HostT* w2 = find(kcat + ".w");
            if (names.size() != 1 || !w2 || w2->dims.size() != 4 || w2->dims[0] != cout || w2->dims[1] != 1 ||
                w2->dims[2] != 1 || w2->dims[3] != c2) {
                set_error("weights: missing or mis-shaped tensor " + kcat + ".w");
                rc = FR_ERR_WEIGHTS;
                return -1;
            }
            std::vector<float> cat((size_t)cout * (cw.K + c2));
            for (int o = 0; o < cout; ++o) {
                std::copy(wrows.begin() + (size_t)o * cw.K, wrows.begin() + (size_t)(o + 1) * cw.K,
                          cat.begin() + (size_t)o * (cw.K + c2));
                std::copy(w2->v.begin() + (size_t)o * c2, w2->v.begin() + (size_t)(o + 1) * c2,
                          cat.begin() + (size_t)o * (cw.K + c2) + cw.K);
            }
            wrows.swap(cat);
            const HostT* b2 = find(kcat + ".b");
            if (b2)
                for (int o = 0; o < cout; ++o) bias[o] += b2->v[o];
            cw.C2 = c2;
            cw.K += c2;
        }
        cw.Npad = round_up(cout, 128);
        cw.Kpad = round_up(cw.K, 64);
        std::vector<bf16_t> packed((size_t)cw.Npad * cw.Kpad, 0);
        const bool f16 = pack_f16;
        for (int o = 0; o < cout; ++o)
            for (int k = 0; k < cw.K; ++k) {
                const float v = wrows[(size_t)o * cw.K + k];
                packed[(size_t)o * cw.Kpad + k] = f16 ? host_f2h(v) : host_f2bf(v);
            }
        bias.resize(cw.Npad, 0.f);
        if ((rc = upload(h, &cw.w, packed))) return -1;
        if (h->dtype == FR_DTYPE_FP8 && names.size() == 1 && !stem_split && cin % 64 == 0 && kcat.empty()) {
            const HostT* ws = find(names[0] + ".wscale");
            if (ws) {  // e4m3 weights: the blob carries e4m3-representable values w/s and the scales s
                if ((int)ws->v.size() != cout) {
                    set_error("weights: mis-sized " + names[0] + ".wscale");
                    rc = FR_ERR_WEIGHTS;
                    return -1;
                }
                cw.Kpad8 = round_up(cw.K, 128);
                std::vector<uint8_t> q((size_t)cw.Npad * cw.Kpad8, 0);
                for (int o = 0; o < cout; ++o)
                    for (int k = 0; k < cw.K; ++k) q[(size_t)o * cw.Kpad8 + k] = host_f2e4m3(wrows[(size_t)o * cw.K + k]);
                std::vector<float> sc(ws->v);
                sc.resize(cw.Npad, 0.f);
                if ((rc = upload(h, &cw.w8, q))) return -1;
                if ((rc = upload(h, &cw.wscale, sc))) return -1;
                // the bf16 copy (debug / op paths) holds the dequantized weights
                for (int o = 0; o < cout; ++o)
                    for (int k = 0; k < cw.K; ++k)
                        packed[(size_t)o * cw.Kpad + k] = host_f2bf(wrows[(size_t)o * cw.K + k] * ws->v[o]);
                if (hipMemcpy(cw.w, packed.data(), packed.size() * sizeof(bf16_t), hipMemcpyHostToDevice) != hipSuccess) {
                    set_error("hipMemcpy of dequantized fp8 weights failed");
                    rc = FR_ERR_HIP;
                    return -1;
                }
            }
        }
        if ((rc = upload(h, &cw.bias, bias))) return -1;
        if (names.size() == 1) {
            const HostT* b9 = find(names[0] + ".b9");
            if (b9 && !kcat.empty()) {  // bias9 replaces `bias`, which carries the folded downsample's bias
                set_error("plan: conv " + names[0] + " has both a border-class bias (.b9) and a K-concatenated "
                          "downsample; the downsample bias would be dropped");
                rc = FR_ERR_WEIGHTS;
                return -1;
            }
            if (b9) {
                if (b9->dims.size() != 2 || b9->dims[0] != 9 || b9->dims[1] != cout || kh != 3 || kw != 3) {
                    set_error("weights: mis-shaped " + names[0] + ".b9 (expects [9, Cout] on a 3x3 conv)");
                    rc = FR_ERR_WEIGHTS;
                    return -1;
                }
                std::vector<float> t9((size_t)9 * cw.Npad, 0.f);
                for (int cl = 0; cl < 9; ++cl)
                    for (int o = 0; o < cout; ++o) t9[(size_t)cl * cw.Npad + o] = b9->v[(size_t)cl * cout + o];
                if ((rc = upload(h, &cw.bias9, t9))) return -1;
            }
        }
        if (c.act == ACT_PRELU) {
            slope.resize(cw.Npad, 0.f);
            if ((rc = upload(h, &cw.slope, slope))) return -1;
        }
        h->convw.push_back(cw);
        return (int)h->convw.size() - 1;
    }

    // Emits one conv op (its tensors must already exist) and returns the op's index, -1 when the load has failed.
    int conv(const ConvSpec& c) {
        if (rc) return -1;
        Op op;
        op.kind = OP_CONV;
        op.in = c.in; op.in_off = c.in_off; op.cin = c.cin;
        op.out = c.out; op.out_off = c.out_off;
        op.res = c.res; op.res_off = c.res_off;
        op.kh = c.kh; op.kw = c.kw; op.sh = c.sh; op.sw = c.sw; op.ph = c.ph; op.pw = c.pw; op.act = c.act;
        op.x2 = c.ds.empty() ? -1 : c.x2;
        op.st2 = c.st2;
        pack_f16 = h->dtype == FR_DTYPE_F16 || h->tensors[c.in].f16;
        // inside an f16 section of a bf16 plan a residual must be f16 too and the output stays f16 (the kernels' y_bf16
        // boundary store takes no residual)
        const bool res_ok = c.res < 0 || (h->tensors[c.res].f16 && h->tensors[c.out].f16);
        if (h->tensors[c.in].f16 && (!res_ok || !c.ds.empty() || h->dtype != FR_DTYPE_BF16)) {
            set_error("plan: f16 section conv " + c.names[0] + " with a residual / second output / projection");
            rc = FR_ERR_ARG;
            return -1;
        }
        op.wi = make_convw(c);
        if (op.wi < 0) return -1;
        const auto& ti = h->tensors[c.in];
        const auto& to = h->tensors[c.out];
        const int Ho = (ti.H + 2 * c.ph - c.kh) / c.sh + 1, Wo = (ti.W + 2 * c.pw - c.kw) / c.sw + 1;
        const int cout = h->convw[op.wi].Cout;
        if (Ho != to.H || Wo != to.W || c.out_off + cout > to.C || c.in_off + c.cin > ti.C ||
            (c.res >= 0 && (h->tensors[c.res].H != Ho || c.res_off + cout > h->tensors[c.res].C)) ||
            (op.x2 >= 0 && (h->tensors[c.x2].C != c.c2 || (Ho - 1) * c.st2 >= h->tensors[c.x2].H ||
                            (Wo - 1) * c.st2 >= h->tensors[c.x2].W || c.cin % 64 != 0 || c.c2 % 64 != 0))) {
            set_error("plan: shape mismatch at conv " + c.names[0]);
            rc = FR_ERR_ARG;
            return -1;
        }
        h->ops.push_back(op);
        return (int)h->ops.size() - 1;
    }

    // whether conv `name` runs in e4m3 (FR_DTYPE_FP8 and the blob's plan gave it a .wscale)
    bool is_fp8(const std::string& name) { return h->dtype == FR_DTYPE_FP8 && find(name + ".wscale"); }
    // whether a residual block's downsample folds into its last conv (igemm K-concatenation): not for
    // e4m3 convs (the fp8 kernel has no projection source) and only on the 64-channel fast-K path;
    // FR_AB no_ds_fuse keeps the separate downsample conv (A/B)
    bool fuse_ds(int cin, int c2, const std::string& pre) {
        static const bool off = [] { return ab_int("no_ds_fuse", 0) != 0; }();
        return !off && !is_fp8(pre + ".conv2") && !is_fp8(pre + ".downsample") && cin % 64 == 0 && c2 % 64 == 0;
    }
    void pre(int out, bool fuse_stem = false) {
        Op op;
        op.kind = OP_PRE;
        op.out = out;
        op.fuse_stem = fuse_stem;
        h->ops.push_back(op);
    }
    void maxpool(const PoolSpec& m) {
        Op op;
        op.kind = OP_MAXPOOL;
        op.in = m.in; op.out = m.out; op.out_off = m.out_off; op.pk = m.k; op.ps = m.s; op.pp = m.p;
        op.cin = h->tensors[m.in].C;
        h->ops.push_back(op);
    }
    void avgpool(int in, int out) {
        Op op;
        op.kind = OP_AVGPOOL;
        op.in = in; op.out = out;
        h->ops.push_back(op);
    }
    void head(int in) {
        if (rc) return;
        const HostT* w = find("head.w");
        const auto& t = h->tensors[in];
        const int K = t.H * t.W * t.C;
        if (!w || w->dims.size() != 2 || w->dims[1] != K) {
            set_error("weights: missing or mis-shaped head.w (expected [N, " + std::to_string(K) + "])");
            rc = FR_ERR_WEIGHTS;
            return;
        }
        W["head.__as_conv.w"] = HostT{{w->dims[0], 1, 1, K}, w->v};
        if (find("head.b")) W["head.__as_conv.b"] = *find("head.b");
        Op op;
        op.kind = OP_HEAD;
        op.in = in;
        op.wi = make_convw({.names = {"head.__as_conv"}, .cin = K});
        if (op.wi < 0) return;
        h->embed_dim = h->convw[op.wi].Cout;
        h->ops.push_back(op);
    }
    // optional FaceNet projection "proj.w" [d, 512] + "proj.b" [d] after the (L2-normalized) head
    void projection() {
        if (rc) return;
        const HostT* w = find("proj.w");
        if (!w) return;
        const HostT* bb = find("proj.b");
        if (w->dims.size() != 2 || w->dims[1] != h->embed_dim || w->dims[1] > 1024 || !bb ||
            (int64_t)bb->v.size() != w->dims[0]) {
            set_error("weights: mis-shaped proj.w / proj.b (expects [d, " + std::to_string(h->embed_dim) + "], [d])");
            rc = FR_ERR_WEIGHTS;
            return;
        }
        if ((rc = upload(h, &h->proj_w, w->v))) return;
        if ((rc = upload(h, &h->proj_b, bb->v))) return;
        h->proj_d = (int)w->dims[0];
    }

    // A fused stage beside its member ops (stages.cpp).  Opening pushes the OP_STAGE op, ahead of the members the
    // caller emits next, and returns its index.
    int open_stage() {
        Op op;
        op.kind = OP_STAGE;
        op.stage = (int)h->stages.size();
        h->ops.push_back(op);
        return (int)h->ops.size() - 1;
    }
    // The one way to name a stage's members: note mark() before emitting a run of ops, add_members() after it.
    int mark() const { return (int)h->ops.size(); }
    void add_members(StageRec& r, int op0) {
        for (int k = op0; k < (int)h->ops.size(); ++k) r.conv_ops.push_back(k);
    }
    // Closing takes the finished record (its members in conv_ops): the members point at the stage, the kind's
    // weight packer runs, and the record joins the plan.  fits = false: the members do not have the fused kernel's
    // shapes, so the plan keeps the member ops only.
    void close_stage(int st_op, StageRec& r, bool fits = true) {
        if (rc) return;
        if (!fits) {
            h->ops.erase(h->ops.begin() + st_op);
            for (auto& op : h->ops)
                if (op.kind == OP_STAGE && op.stage >= (int)h->stages.size()) --op.stage;
            return;
        }
        for (int oi : r.conv_ops) h->ops[oi].stage = h->ops[st_op].stage;
        rc = pack_stage(h, r);
        h->stages.push_back(r);
    }
};

std::string L(int l, int i) { return "layer" + std::to_string(l) + "." + std::to_string(i); }

void build_iresnet100(Builder& b) {
    fr_handle* h = b.h;
    h->in_size = 112;
    const int in = b.tensor(112, 112, 8);
    b.pre(in, true);  // u8 input: preparation + conv1 in one launch (conv_stem.hip)
    // Each block's pre-conv bn1 is folded into its conv1 (weights scaled per input channel, the shift in
    // a border-class bias table .b9: weights.fold_state_dict), so conv1 reads the previous block's output
    // directly and no producer writes a second (bn1) output.
    int x = b.tensor(112, 112, 64, "prelu");
    b.stem = true;
    b.conv(sq({.names = {"conv1"}, .in = in, .cin = 8, .out = x, .act = ACT_PRELU}, 3, 1, 1));
    const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 13, 30, 3};
    int H = 112, C = 64;
    // the bf16 layer3 stage stays open until layer4.0.conv1 is emitted: that conv becomes its tail
    StageRec tail_rec;
    int tail_st_op = -1;
    for (int l = 0; l < 4; ++l) {
        const int P = planes[l], Ho = H / 2;
        // layer3 blocks 1.. (stride 1, 14x14x256) and layer2 / layer1 blocks 1..: also emitted as
        // LDS-resident stage ops.  Under FR_DTYPE_FP8 the blocks whose convs carry .wscale (the mixed
        // plan, weights.FP8_PLAN) form an e4m3 stage of their own (14x14x256 only), the rest bf16 stages.
        int st_op = -1;
        StageRec rec;
        auto end_run = [&](bool layer_end) {
            if (st_op < 0) return;
            rec.out = x;
            rec.nblk = (int)rec.t_tensors.size();
            // tail candidates: the bf16 layer3 stage (-> layer4.0.conv1) and the layer2 split stage (-> layer3.0.conv1)
            if (!b.rc && layer_end && !rec.fp8 &&
                ((l == 2 && rec.parts == 1 && rec.C == 256) || (l == 1 && rec.parts == 2 && rec.C == 128 && rec.H == 28))) {
                tail_rec = rec;
                tail_st_op = st_op;
            } else {
                b.close_stage(st_op, rec);
            }
            st_op = -1;
        };
        for (int i = 0; i < nblk[l]; ++i) {
            const bool s14 = stage_supported(1, Ho, Ho, P);
            const int parts = split_stage_parts(Ho, Ho, P);
            const std::string pre = L(l + 1, i);
            const bool f8 = b.is_fp8(pre + ".conv1") && b.is_fp8(pre + ".conv2");
            const bool mixed = b.is_fp8(pre + ".conv1") != b.is_fp8(pre + ".conv2");
            const bool can = i >= 1 && P == C && !mixed && (f8 ? s14 : (s14 || parts > 0));
            if (st_op >= 0 && (!can || f8 != rec.fp8)) end_run(false);
            if (can && st_op < 0) {
                st_op = b.open_stage();
                rec = StageRec{};
                rec.kind = STAGE_LDS;
                rec.in = x;
                rec.parts = s14 ? 1 : parts;
                rec.H = Ho;
                rec.C = P;
                rec.fp8 = f8;
            }
            const int Hin = i == 0 ? H : Ho, st = i == 0 ? 2 : 1;
            const bool fuse = i == 0 && b.fuse_ds(P, C, pre);
            // layer1.0 as one fused launch (conv_trans.hip) beside its member convs (measured per batch size)
            const bool tr = i == 0 && fuse && !b.is_fp8(pre + ".conv1") && !b.is_fp8(pre + ".conv2") &&
                            trans_supported(1, H, H, C, P, P, 9 * C, 9 * P + C);
            const int tr_op = tr ? b.open_stage() : -1;
            const int op0 = b.mark();  // the block's ops: conv1, (a separate downsample,) conv2
            const int hmid = b.tensor(Hin, Hin, P, pre + ".prelu");
            const int c1 = b.conv(sq({.names = {pre + ".conv1"}, .in = x, .cin = C, .out = hmid, .act = ACT_PRELU}, 3, 1, 1));
            if (tail_st_op >= 0 && !b.rc) {  // layer4.0.conv1: the layer3 stage's tail when it fits, then close it
                const Op& op = h->ops[c1];
                const DevConvW& cw = h->convw[op.wi];
                static const bool no_tail = ab_int("no_stage_tail", 0) != 0;  // FR_AB no_stage_tail: A/B timing
                const int TC = tail_rec.C;
                if (!no_tail && h->dtype != FR_DTYPE_FP8 && !cw.w8 && op.act == ACT_PRELU && cw.slope && cw.Cout == 2 * TC &&
                    cw.Npad >= 2 * TC && cw.Cin == TC && cw.Kh == 3 && cw.Kw == 3 && op.sh == 1 && op.sw == 1 && op.ph == 1 &&
                    op.pw == 1 && op.in == tail_rec.out && op.in_off == 0 && op.out_off == 0 && op.res < 0 && op.x2 < 0 &&
                    h->tensors[hmid].C == 2 * TC && !h->tensors[hmid].f16)
                    tail_rec.tail_op = c1;
                if (tail_rec.tail_op >= 0) tail_rec.conv_ops.push_back(c1);  // (the packer reads the blocks' 2 * nblk first)
                b.close_stage(tail_st_op, tail_rec);
                tail_st_op = -1;
            }
            int res = x;
            if (i == 0 && !fuse) {
                res = b.tensor(Ho, Ho, P, pre + ".downsample");
                b.conv({.names = {pre + ".downsample"}, .in = x, .cin = C, .out = res, .sh = 2, .sw = 2});
            }
            const int y = b.tensor(Ho, Ho, P, pre);
            if (fuse)  // y = conv2(t) + downsample(x) in one K loop (no downsample tensor)
                b.conv(sq({.names = {pre + ".conv2"}, .in = hmid, .cin = P, .out = y,
                           .ds = pre + ".downsample", .x2 = x, .c2 = C, .st2 = 2}, 3, st, 1));
            else
                b.conv(sq({.names = {pre + ".conv2"}, .in = hmid, .cin = P, .out = y, .res = res}, 3, st, 1));
            if (tr && !b.rc) {
                StageRec t;
                t.kind = STAGE_TRANS;
                t.in = x; t.out = y; t.nblk = 1; t.H = H; t.C = P;
                b.add_members(t, op0);
                t.t_tensors = {hmid};
                t.x_tensors = {y};
                b.close_stage(tr_op, t);
            }
            if (st_op >= 0 && !b.rc) {
                b.add_members(rec, op0);
                rec.t_tensors.push_back(hmid);
                rec.x_tensors.push_back(y);
            }
            x = y;
            C = P;
        }
        end_run(true);
        H = Ho;
    }
    h->ex_tensor = x;  // fr_explain: Grad-CAM on layer4.2, which the head reads flattened (NHWC order)
    h->ex_layout = 1;
    b.head(x);
}

void build_resnet50(Builder& b) {
    fr_handle* h = b.h;
    h->in_size = 112;
    const int in = b.tensor(112, 112, 8);
    b.pre(in);
    const int c1 = b.tensor(56, 56, 64, "backbone.relu");
    // conv1 + maxpool are also emitted as one launch (conv_stem_r50.hip) beside the member ops
    const bool st = h->dtype != FR_DTYPE_FP8;
    const int st_op = st ? b.open_stage() : -1;
    const int op0 = b.mark();
    b.stem = true;
    b.conv(sq({.names = {"backbone.conv1"}, .in = in, .cin = 8, .out = c1, .act = ACT_RELU}, 7, 2, 3));
    int x = b.tensor(28, 28, 64, "backbone.maxpool");
    b.maxpool({.in = c1, .out = x, .k = 3, .s = 2, .p = 1});
    if (st && !b.rc) {
        StageRec sr;
        sr.kind = STAGE_STEM_R50;
        sr.in = in; sr.out = x; sr.H = 112; sr.C = 8; sr.nblk = 1;
        b.add_members(sr, op0);
        const Op& cv = h->ops[sr.conv_ops[0]];
        const DevConvW& cw = h->convw[cv.wi];
        // a stem without the fused kernel's shape fails the load (no fall-back to the member ops)
        if (!stem_r50_supported(112, 112, cv.cin, cw.K, cw.Kpad, cw.Cout) || cw.w8 || !cw.bias || cv.act != ACT_RELU ||
            cv.sh != 2 || cv.ph != 3 || cv.res >= 0 || h->ops[sr.conv_ops[1]].kind != OP_MAXPOOL) {
            set_error("plan: ResNet-50 stem does not have the fused kernel's shape");
            b.rc = FR_ERR_ARG;
        }
        b.close_stage(st_op, sr);
    }
    const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 4, 6, 3}, strd[4] = {1, 2, 2, 2};
    int H = 28, C = 64;
    // layer3.1 .. layer3.5 (7x7x1024) are also emitted as one chain launch (conv_chain_r50.hip) beside their member
    // convs; the faster is measured per batch size
    int ch_op = -1, bn_op = -1;
    StageRec ch, bn;
    for (int l = 0; l < 4; ++l) {
        const int P = planes[l];
        for (int i = 0; i < nblk[l]; ++i) {
            const std::string pre = "backbone." + L(l + 1, i);
            // layer1 (28x28) likewise, one launch per block (conv_bneck28.hip): from layer1.0 when its downsample folds
            // into conv3 (fuse_ds), else from layer1.1
            const bool bn_ds = i == 0 && C == P && b.fuse_ds(P, C, pre);
            if (l == 0 && bn_op < 0 && (bn_ds || i == 1) && h->dtype != FR_DTYPE_FP8 && bneck28_supported(H, H, 4 * P, P)) {
                bn_op = b.open_stage();
                bn.kind = STAGE_BNECK28;
                bn.bn_ds = bn_ds;
                bn.in = x; bn.H = H; bn.C = C; bn.nblk = nblk[l] - i;
            }
            if (l == 2 && i == 1 && h->dtype != FR_DTYPE_FP8 && H == 7 && chain_r50_supported(H, H, C, nblk[l] - 1)) {
                ch_op = b.open_stage();
                ch.kind = STAGE_CHAIN_R50;
                ch.in = x; ch.H = H; ch.C = C; ch.nblk = nblk[l] - 1;
            }
            const int blk0 = b.mark();
            const int s = i == 0 ? strd[l] : 1;
            const int Ho = (H + 2 - 3) / s + 1;
            const int h1 = b.tensor(H, H, P);
            b.conv({.names = {pre + ".conv1"}, .in = x, .cin = C, .out = h1, .act = ACT_RELU});
            const int h2 = b.tensor(Ho, Ho, P);
            b.conv(sq({.names = {pre + ".conv2"}, .in = h1, .cin = P, .out = h2, .act = ACT_RELU}, 3, s, 1));
            int id = x;
            const bool fuse = i == 0 && b.fuse_ds(P, C, pre);
            if (i == 0 && !fuse) {
                id = b.tensor(Ho, Ho, 4 * P, pre + ".downsample");
                b.conv({.names = {pre + ".downsample"}, .in = x, .cin = C, .out = id, .sh = s, .sw = s});
            }
            const int y = b.tensor(Ho, Ho, 4 * P, pre);
            if (fuse)  // y = relu(conv3(h2) + downsample(x)) in one K loop
                b.conv({.names = {pre + ".conv3"}, .in = h2, .cin = P, .out = y, .act = ACT_RELU,
                        .ds = pre + ".downsample", .x2 = x, .c2 = C, .st2 = s});
            else
                b.conv({.names = {pre + ".conv3"}, .in = h2, .cin = P, .out = y, .act = ACT_RELU, .res = id});
            if (ch_op >= 0 && l == 2 && i >= 1) b.add_members(ch, blk0);
            if (bn_op >= 0 && l == 0) {
                b.add_members(bn, blk0);
                bn.x_tensors.push_back(y);
            }
            x = y;
            C = 4 * P;
            H = Ho;
        }
        if (bn_op >= 0 && l == 0) {
            bn.out = x;
            b.close_stage(bn_op, bn);
        }
        if (ch_op >= 0 && l == 2) {
            ch.out = x;
            b.close_stage(ch_op, ch);
        }
        if (l == 2) h->cut_l4in = x;  // fr_features_at: what layer4.0.conv1 and layer4.0.downsample read
    }
    h->ex_tensor = x;  // fr_explain: Grad-CAM on backbone.layer4 (the avg-pool's input)
    h->ex_layout = 0;
    const int pool = b.tensor(1, 1, C, "backbone.avgpool");
    b.avgpool(x, pool);
    b.head(pool);
}

void build_irv1(Builder& b) {
    fr_handle* h = b.h;
    h->in_size = 160;
    const std::string m = "model.";
    // bf16 plan: the high-resolution stem (input .. conv2d_4a) is stored and multiplied in f16.  Its
    // activations are ~90 % of the forward's bf16 rounding drift (profiles/r02_irv1_drift_bf16_vs_f16.txt:
    // 1.28e-2 of 1.61e-2 relative error is in place at conv2d_4b); f16 MFMAs run at the bf16 rate, and
    // conv2d_4b writes bf16 for the rest of the network.  FR_IRV1_BF16_STEM=1 keeps it bf16 (A/B).
    static const bool bf16_stem = [] {
        const char* e = getenv("FR_IRV1_BF16_STEM");
        return e && e[0] == '1';
    }();
    // Round 6: the f16 section also covers conv2d_4b's output, repeat_1 (Block35 x5) and mixed_6a's inner branch
    // tensors; mixed_6a's convs and max-pool write the bf16 concat (the section boundary).  With the stem alone in f16
    // the bf16 body still moved bs = 256 embeddings up to 8.9e-4 (1 - cos) from the fp32 oracle and flipped 7 % of
    // the non-planted top-1 matches; f16 MFMAs run at the bf16 rate.  FR_AB irv1_f16_mid=0: the
    // round-5 boundary at conv2d_4b (A/B).
    // FR_AB irv1_f16_mid=2 (default): through repeat_2 (Block17 x10) too, the boundary at mixed_7a's outputs
    static const int f16_mid = ab_int("irv1_f16_mid", 2);
    const bool stem16 = h->dtype == FR_DTYPE_BF16 && !bf16_stem;
    const bool mid16 = stem16 && f16_mid >= 1;
    const bool mid16b = mid16 && f16_mid >= 2;
    const int in = b.tensor(160, 160, 8, "", stem16);
    b.pre(in);
    const int a = b.tensor(79, 79, 32, m + "conv2d_1a", stem16);
    const int bb = b.tensor(77, 77, 32, m + "conv2d_2a", stem16);
    const int c = b.tensor(77, 77, 64, m + "conv2d_2b", stem16);
    const int d = b.tensor(38, 38, 64, m + "maxpool_3a", stem16);
    const int e = b.tensor(38, 38, 80, m + "conv2d_3b", stem16);
    const int f = b.tensor(36, 36, 192, m + "conv2d_4a", stem16);
    int x = b.tensor(17, 17, 256, m + "conv2d_4b", mid16);
    b.stem = true;
    // conv2d_1a .. conv2d_3b also as one launch (conv_stem160.hip) beside the member ops, measured per batch size
    const int st_op = h->dtype != FR_DTYPE_FP8 ? b.open_stage() : -1;
    const int op0 = b.mark();
    b.conv(sq({.names = {m + "conv2d_1a"}, .in = in, .cin = 8, .out = a, .act = ACT_RELU}, 3, 2, 0));
    b.conv(sq({.names = {m + "conv2d_2a"}, .in = a, .cin = 32, .out = bb, .act = ACT_RELU}, 3, 1, 0));
    b.conv(sq({.names = {m + "conv2d_2b"}, .in = bb, .cin = 32, .out = c, .act = ACT_RELU}, 3, 1, 1));
    b.maxpool({.in = c, .out = d, .k = 3, .s = 2, .p = 0});
    b.conv({.names = {m + "conv2d_3b"}, .in = d, .cin = 64, .out = e, .act = ACT_RELU});
    if (st_op >= 0 && !b.rc) {
        StageRec sr;
        sr.kind = STAGE_STEM160;
        sr.in = in; sr.out = e; sr.H = 160; sr.C = 80; sr.nblk = 1;
        b.add_members(sr, op0);  // {1a, 2a, 2b, maxpool_3a, 3b}
        const Op& o1 = h->ops[sr.conv_ops[0]];
        const Op& o2 = h->ops[sr.conv_ops[1]];
        const Op& o3 = h->ops[sr.conv_ops[2]];
        const Op& o4 = h->ops[sr.conv_ops[4]];
        const DevConvW& c1 = h->convw[o1.wi];
        const DevConvW& c2 = h->convw[o2.wi];
        const DevConvW& c3 = h->convw[o3.wi];
        const DevConvW& c4 = h->convw[o4.wi];
        bool ok = stem160_supported(160, 160, 8, c1.K, c2.K, c3.K, c4.K, c1.Cout, c2.Cout, c3.Cout, c4.Cout) &&
                  h->tensors[in].f16 == h->tensors[e].f16 && o1.act == ACT_RELU && o2.act == ACT_RELU &&
                  o3.act == ACT_RELU && o4.act == ACT_RELU;
        for (const DevConvW* cw : {&c1, &c2, &c3, &c4}) ok = ok && cw->bias && !cw->bias9 && !cw->w8;
        b.close_stage(st_op, sr, ok);  // not ok falls back (fits = false): no fused stem, the member ops only
    }
    b.conv(sq({.names = {m + "conv2d_4a"}, .in = e, .cin = 80, .out = f, .act = ACT_RELU}, 3, 1, 0));
    b.conv(sq({.names = {m + "conv2d_4b"}, .in = f, .cin = 192, .out = x, .act = ACT_RELU}, 3, 2, 0));
    // repeat_1: Block35 x5 @17x17. cat layout [t1 | t2 | b0 | b1 | b2]; conv2d reads [64:160].  Also emitted as one
    // chain launch (conv_chain35.hip) beside its member convs; the faster is measured per batch size.
    int c35_op = -1;
    StageRec c35;
    if (h->dtype != FR_DTYPE_FP8 && chain35_supported(17, 17, 256, 5)) {
        c35_op = b.open_stage();
        c35.kind = STAGE_CHAIN35;
        c35.in = x; c35.H = 17; c35.C = 256; c35.nblk = 5;
    }
    for (int i = 0; i < 5; ++i) {
        const std::string p = m + "repeat_1." + std::to_string(i) + ".";
        const int blk0 = b.mark();
        const int cat = b.tensor(17, 17, 160, "", mid16);
        b.conv({.names = {p + "branch1.0", p + "branch2.0", p + "branch0"}, .in = x, .cin = 256, .out = cat, .act = ACT_RELU});
        b.conv(sq({.names = {p + "branch1.1"}, .in = cat, .cin = 32, .out = cat, .out_off = 96, .act = ACT_RELU}, 3, 1, 1));
        const int t = b.tensor(17, 17, 32, "", mid16);
        b.conv(sq({.names = {p + "branch2.1"}, .in = cat, .in_off = 32, .cin = 32, .out = t, .act = ACT_RELU}, 3, 1, 1));
        b.conv(sq({.names = {p + "branch2.2"}, .in = t, .cin = 32, .out = cat, .out_off = 128, .act = ACT_RELU}, 3, 1, 1));
        const int y = b.tensor(17, 17, 256, m + "repeat_1." + std::to_string(i), mid16);
        b.conv({.names = {p + "conv2d"}, .in = cat, .in_off = 64, .cin = 96, .out = y, .act = ACT_RELU, .res = x});
        if (c35_op >= 0) {
            b.add_members(c35, blk0);
            c35.x_tensors.push_back(y);
        }
        x = y;
    }
    if (c35_op >= 0) {
        c35.out = x;
        b.close_stage(c35_op, c35);
    }
    {  // mixed_6a
        const std::string p = m + "mixed_6a.";
        const int cat = b.tensor(8, 8, 896, m + "mixed_6a", mid16b);
        b.conv(sq({.names = {p + "branch0"}, .in = x, .cin = 256, .out = cat, .act = ACT_RELU}, 3, 2, 0));
        const int u = b.tensor(17, 17, 192, "", mid16), v = b.tensor(17, 17, 192, "", mid16);
        b.conv({.names = {p + "branch1.0"}, .in = x, .cin = 256, .out = u, .act = ACT_RELU});
        b.conv(sq({.names = {p + "branch1.1"}, .in = u, .cin = 192, .out = v, .act = ACT_RELU}, 3, 1, 1));
        b.conv(sq({.names = {p + "branch1.2"}, .in = v, .cin = 192, .out = cat, .out_off = 384, .act = ACT_RELU}, 3, 2, 0));
        b.maxpool({.in = x, .out = cat, .out_off = 640, .k = 3, .s = 2, .p = 0});
        x = cat;
    }
    // repeat_2: Block17 x10 @8x8. cat layout [t1 | b0 | b1]; conv2d reads [128:384].  Also emitted as one
    // chain launch (conv_chain.hip) beside its member convs; the faster is measured per batch size.
    int ch_op = -1;
    StageRec ch;
    if (h->dtype != FR_DTYPE_FP8 && chain17_supported(8, 8, 896, 10)) {
        ch_op = b.open_stage();
        ch.kind = STAGE_CHAIN17;
        ch.in = x; ch.H = 8; ch.C = 896; ch.nblk = 10;
    }
    for (int i = 0; i < 10; ++i) {
        const std::string p = m + "repeat_2." + std::to_string(i) + ".";
        const int blk0 = b.mark();
        const int cat = b.tensor(8, 8, 384, "", mid16b);
        const int t = b.tensor(8, 8, 128, "", mid16b);
        const int y = b.tensor(8, 8, 896, m + "repeat_2." + std::to_string(i), mid16b);
        b.conv({.names = {p + "branch1.0", p + "branch0"}, .in = x, .cin = 896, .out = cat, .act = ACT_RELU});
        b.conv({.names = {p + "branch1.1"}, .in = cat, .cin = 128, .out = t, .kw = 7, .pw = 3, .act = ACT_RELU});
        b.conv({.names = {p + "branch1.2"}, .in = t, .cin = 128, .out = cat, .out_off = 256, .kh = 7, .ph = 3, .act = ACT_RELU});
        b.conv({.names = {p + "conv2d"}, .in = cat, .in_off = 128, .cin = 256, .out = y, .act = ACT_RELU, .res = x});
        if (ch_op >= 0) b.add_members(ch, blk0);
        x = y;
    }
    if (ch_op >= 0) {
        ch.out = x;
        b.close_stage(ch_op, ch);
    }
    {  // mixed_7a
        const std::string p = m + "mixed_7a.";
        const int cat = b.tensor(3, 3, 1792, m + "mixed_7a");
        const int u = b.tensor(8, 8, 768, "", mid16b);
        b.conv({.names = {p + "branch0.0", p + "branch1.0", p + "branch2.0"}, .in = x, .cin = 896, .out = u, .act = ACT_RELU});
        b.conv(sq({.names = {p + "branch0.1"}, .in = u, .cin = 256, .out = cat, .act = ACT_RELU}, 3, 2, 0));
        b.conv(sq({.names = {p + "branch1.1"}, .in = u, .in_off = 256, .cin = 256, .out = cat, .out_off = 384, .act = ACT_RELU}, 3, 2, 0));
        const int v = b.tensor(8, 8, 256, "", mid16b);
        b.conv(sq({.names = {p + "branch2.1"}, .in = u, .in_off = 512, .cin = 256, .out = v, .act = ACT_RELU}, 3, 1, 1));
        b.conv(sq({.names = {p + "branch2.2"}, .in = v, .cin = 256, .out = cat, .out_off = 640, .act = ACT_RELU}, 3, 2, 0));
        b.maxpool({.in = x, .out = cat, .out_off = 896, .k = 3, .s = 2, .p = 0});
        x = cat;
    }
    // repeat_3: Block8 x5 + final block8 (noReLU) @3x3. cat layout [t1 | b0 | b1]; conv2d reads [192:576].
    int last = -1;
    for (int i = 0; i < 6; ++i) {
        const std::string p = i < 5 ? m + "repeat_3." + std::to_string(i) + "." : m + "block8.";
        const int cat = b.tensor(3, 3, 576);
        b.conv({.names = {p + "branch1.0", p + "branch0"}, .in = x, .cin = 1792, .out = cat, .act = ACT_RELU});
        const int t = b.tensor(3, 3, 192);
        b.conv({.names = {p + "branch1.1"}, .in = cat, .cin = 192, .out = t, .kw = 3, .pw = 1, .act = ACT_RELU});
        b.conv({.names = {p + "branch1.2"}, .in = t, .cin = 192, .out = cat, .out_off = 384, .kh = 3, .ph = 1, .act = ACT_RELU});
        const int y = b.tensor(3, 3, 1792, i < 5 ? m + "repeat_3." + std::to_string(i) : m + "block8");
        last = b.conv({.names = {p + "conv2d"}, .in = cat, .in_off = 192, .cin = 384, .out = y,
                       .act = i < 5 ? ACT_RELU : ACT_NONE, .res = x});
        x = y;
    }
    // fr_explain: the activation map of block8.conv2d's own output.  That conv writes conv + x, so fr_explain runs
    // it once more without the residual into this scratch tensor (never the difference of two bf16 tensors)
    if (!b.rc) {
        h->ex_conv = last;
        h->ex_tensor = b.tensor(3, 3, 1792);
        h->ex_layout = 2;
    }
    const int pool = b.tensor(1, 1, 1792, m + "avgpool_1a");
    b.avgpool(x, pool);
    b.head(pool);
    b.projection();
}

}  // namespace

int fr::build_plan(fr_handle* h, Blob& W) {
    Builder b{h, W};
    if (h->arch == FR_ARCH_IRESNET100) build_iresnet100(b);
    else if (h->arch == FR_ARCH_RESNET50_ARCFACE) build_resnet50(b);
    else build_irv1(b);
    return b.rc;
}
