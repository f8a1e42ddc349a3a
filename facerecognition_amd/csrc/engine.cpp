// frhip engine: C-ABI handle, weight-blob loader, static per-arch forward plans and the
// gallery/match entry points.  See include/frhip.h for the boundary contract and
// DESIGN.md for the data layout.  The fused stages of a plan (their kinds, packers, launches) are in stages.cpp,
// how a conv gets its kernel (the conv kernel kinds, the tuner, the op API's forced kernels) in convs.cpp.
//
// The forward plans restate the reference backbones as a list of fused ops:
//   FR_ARCH_RESNET50_ARCFACE  models/arcface/arcface_model.py:118-132 + head :192-196
//   FR_ARCH_IRESNET100        insightface iresnet100 (IBasicBlock; README.md:72)
//   FR_ARCH_IRV1_FACENET      facenet_pytorch InceptionResnetV1 (facenet_model.py:12-16)
// BN is folded into the conv weights/bias by the Python importer
// (facerecognition_amd/weights.py); this file only knows tensor names.
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

struct HostT {
    std::vector<int64_t> dims;
    std::vector<float> v;
};

int round_up(int x, int m) { return (x + m - 1) / m * m; }

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

// ------------------------------------------------------------------ weight blob
// FRW1 := "FRW1" u32 count { u32 name_len, name, u32 ndim, i64 dims[ndim], f32 data[prod] }*
int parse_blob(const void* blob, size_t n, std::unordered_map<std::string, HostT>& out) {
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

// ------------------------------------------------------------------ plan builder
struct Builder {
    fr_handle* h;
    std::unordered_map<std::string, HostT>& W;
    int rc = FR_OK;

    int tensor(int H, int Wd, int C, const std::string& name = "") {
        h->tensors.push_back({H, Wd, C, nullptr, name});
        return (int)h->tensors.size() - 1;
    }

    const HostT* find(const std::string& n) {
        auto it = W.find(n);
        return it == W.end() ? nullptr : &it->second;
    }

    bool stem = false;  // next conv is the network stem: fold 1/255 + hi/lo split (see launch_preprocess)

    bool pack_f16 = false;  // the conv being built reads an f16 tensor: f16 weights (set by conv_ds)

    float round16(float v) const {  // stem hi/lo split in the activation dtype (bf16 for FR_DTYPE_FP8)
        return pack_f16 ? host_h2f(host_f2h(v)) : host_bf2f(host_f2bf(v));
    }

    // Build one (possibly N-concatenated) conv weight: names[i].w is [Cout_i, kh, kw, Cin_w] f32.
    // kcat (single name only): a 1x1 conv [Cout, 1, 1, c2] whose weights are appended to every row
    // (K = kh*kw*cin + c2) and whose bias is added: a residual block's downsample folded into its last conv.
    int make_convw(const std::vector<std::string>& names, int kh, int kw, int cin, int act, const std::string& aff,
                   const std::string& kcat = "", int c2 = 0) {
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
                        for (int c = 0; c < cin; ++c) {
                            if (stem_split) {
                                // input channels are [q, q, 0, 0], q = 255*x: weights [hi, lo, 0, 0] of w/255
                                const float wv = w->v[(((size_t)o * kh + r) * kw + s) * ci + (c % 3)] / 255.0f;
                                const float hi = round16(wv);
                                wrows.push_back(c < 3 ? hi : (c < 6 ? wv - hi : 0.f));
                            } else {
                                wrows.push_back(c < ci ? w->v[(((size_t)o * kh + r) * kw + s) * ci + c] : 0.f);
                            }
                        }
            const HostT* b = find(nm + ".b");
            for (int o = 0; o < co; ++o) bias.push_back(b ? b->v[o] : 0.f);
            if (act == 2) {
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
                for (int c = 0; c < 9; ++c)
                    for (int o = 0; o < cout; ++o) t9[(size_t)c * cw.Npad + o] = b9->v[(size_t)c * cout + o];
                if ((rc = upload(h, &cw.bias9, t9))) return -1;
            }
        }
        if (act == 2) {
            slope.resize(cw.Npad, 0.f);
            if ((rc = upload(h, &cw.slope, slope))) return -1;
        }
        if (!aff.empty()) {
            const HostT* s = find(aff + ".s");
            const HostT* t = find(aff + ".t");
            if (!s || !t || (int)s->v.size() != cout || (int)t->v.size() != cout) {
                set_error("weights: missing or mis-sized affine " + aff + ".s/.t");
                rc = FR_ERR_WEIGHTS;
                return -1;
            }
            std::vector<float> sv = s->v, tv = t->v;
            sv.resize(cw.Npad, 0.f);
            tv.resize(cw.Npad, 0.f);
            if ((rc = upload(h, &cw.aff_s, sv))) return -1;
            if ((rc = upload(h, &cw.aff_b, tv))) return -1;
        }
        h->convw.push_back(cw);
        return (int)h->convw.size() - 1;
    }

    // conv op; returns output spatial size through the out tensor (must already exist).
    void conv(const std::vector<std::string>& names, int in, int in_off, int cin, int out, int out_off, int kh, int kw,
              int sh, int sw, int ph, int pw, int act, int res = -1, int res_off = 0, int out2 = -1,
              const std::string& aff = "") {
        conv_ds(names, in, in_off, cin, out, out_off, kh, kw, sh, sw, ph, pw, act, res, res_off, out2, aff, "", -1, 0, 1);
    }

    // conv whose residual is a downsample (1x1 conv `ds` of tensor x2 at stride st2) folded into its K
    // (ds empty: a plain conv)
    void conv_ds(const std::vector<std::string>& names, int in, int in_off, int cin, int out, int out_off, int kh,
                 int kw, int sh, int sw, int ph, int pw, int act, int res, int res_off, int out2, const std::string& aff,
                 const std::string& ds, int x2, int c2, int st2) {
        if (rc) return;
        Op op;
        op.kind = OP_CONV;
        op.in = in; op.in_off = in_off; op.cin = cin;
        op.out = out; op.out_off = out_off;
        op.res = res; op.res_off = res_off; op.out2 = out2;
        op.kh = kh; op.kw = kw; op.sh = sh; op.sw = sw; op.ph = ph; op.pw = pw; op.act = act;
        op.x2 = ds.empty() ? -1 : x2;
        op.st2 = st2;
        pack_f16 = h->dtype == FR_DTYPE_F16 || h->tensors[in].f16;
        // inside an f16 section of a bf16 plan a residual must be f16 too and the output stays f16 (the kernels' y_bf16
        // boundary store takes no residual)
        const bool res_ok = res < 0 || (h->tensors[res].f16 && h->tensors[out].f16);
        if (h->tensors[in].f16 && (!res_ok || out2 >= 0 || !ds.empty() || h->dtype != FR_DTYPE_BF16)) {
            set_error("plan: f16 section conv " + names[0] + " with a residual / second output / projection");
            rc = FR_ERR_ARG;
            return;
        }
        op.wi = make_convw(names, kh, kw, cin, act, aff, ds, c2);
        if (op.wi < 0) return;
        const auto& ti = h->tensors[in];
        const auto& to = h->tensors[out];
        const int Ho = (ti.H + 2 * ph - kh) / sh + 1, Wo = (ti.W + 2 * pw - kw) / sw + 1;
        const int cout = h->convw[op.wi].Cout;
        if (Ho != to.H || Wo != to.W || out_off + cout > to.C || in_off + cin > ti.C ||
            (res >= 0 && (h->tensors[res].H != Ho || res_off + cout > h->tensors[res].C)) ||
            (op.x2 >= 0 && (h->tensors[x2].C != c2 || (Ho - 1) * st2 >= h->tensors[x2].H ||
                            (Wo - 1) * st2 >= h->tensors[x2].W || cin % 64 != 0 || c2 % 64 != 0))) {
            set_error("plan: shape mismatch at conv " + names[0]);
            rc = FR_ERR_ARG;
            return;
        }
        h->ops.push_back(op);
    }

    // whether a residual block's downsample folds into its last conv (igemm K-concatenation): not for
    // e4m3 convs (the fp8 kernel has no projection source) and only on the 64-channel fast-K path;
    // FR_AB no_ds_fuse keeps the separate downsample conv (A/B)
    // whether conv `name` runs in e4m3 (FR_DTYPE_FP8 and the blob's plan gave it a .wscale)
    bool is_fp8(const std::string& name) { return h->dtype == FR_DTYPE_FP8 && find(name + ".wscale"); }
    bool fuse_ds(int cin, int c2, const std::string& pre) {
        static const bool off = [] { return ab_int("no_ds_fuse", 0) != 0; }();
        return !off && !is_fp8(pre + ".conv2") && !is_fp8(pre + ".downsample") && cin % 64 == 0 && c2 % 64 == 0;
    }
    void maxpool(int in, int out, int out_off, int k, int s, int p) {
        Op op;
        op.kind = OP_MAXPOOL;
        op.in = in; op.out = out; op.out_off = out_off; op.pk = k; op.ps = s; op.pp = p;
        op.cin = h->tensors[in].C;
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
        op.wi = make_convw({"head.__as_conv"}, 1, 1, K, 0, "");
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
    h->ops.push_back(Op{OP_PRE, -1, 0, 0, in});
    // Each block's pre-conv bn1 is folded into its conv1 (weights scaled per input channel, the shift in
    // a border-class bias table .b9: weights.fold_state_dict), so conv1 reads the previous block's output
    // directly and no producer writes a second (bn1) output.
    int x = b.tensor(112, 112, 64, "prelu");
    b.stem = true;
    b.conv({"conv1"}, in, 0, 8, x, 0, 3, 3, 1, 1, 1, 1, 2);
    h->ops[h->ops.size() - 2].fuse_stem = true;  // conv_stem.hip (u8 input)
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
        auto close_stage = [&](bool layer_end) {
            // tail candidates: the bf16 layer3 stage (-> layer4.0.conv1) and the layer2 split stage (-> layer3.0.conv1)
            if (st_op >= 0 && !b.rc && layer_end && !rec.fp8 &&
                ((l == 2 && rec.parts == 1 && rec.C == 256) || (l == 1 && rec.parts == 2 && rec.C == 128 && rec.H == 28))) {
                rec.out = x;
                rec.nblk = (int)rec.t_tensors.size();
                tail_rec = rec;
                tail_st_op = st_op;
            } else if (st_op >= 0) {
                rec.out = x;
                rec.nblk = (int)rec.t_tensors.size();
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
            if (st_op >= 0 && (!can || f8 != rec.fp8)) close_stage(false);
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
            const int hmid = b.tensor(Hin, Hin, P, pre + ".prelu");
            b.conv({pre + ".conv1"}, x, 0, C, hmid, 0, 3, 3, 1, 1, 1, 1, 2);
            if (tail_st_op >= 0 && !b.rc) {  // layer4.0.conv1: the layer3 stage's tail when it fits, then close it
                const int oi = (int)h->ops.size() - 1;
                const Op& op = h->ops[oi];
                const DevConvW& cw = h->convw[op.wi];
                static const bool no_tail = ab_int("no_stage_tail", 0) != 0;  // FR_AB no_stage_tail: A/B timing
                const int TC = tail_rec.C;
                if (!no_tail && h->dtype != FR_DTYPE_FP8 && !cw.w8 && op.act == 2 && cw.slope && cw.Cout == 2 * TC &&
                    cw.Npad >= 2 * TC && cw.Cin == TC && cw.Kh == 3 && cw.Kw == 3 && op.sh == 1 && op.sw == 1 && op.ph == 1 &&
                    op.pw == 1 && op.in == tail_rec.out && op.in_off == 0 && op.out_off == 0 && op.res < 0 && op.x2 < 0 &&
                    op.out2 < 0 && h->tensors[hmid].C == 2 * TC && !h->tensors[hmid].f16)
                    tail_rec.tail_op = oi;
                if (tail_rec.tail_op >= 0) tail_rec.conv_ops.push_back(oi);  // (the packer reads the blocks' 2 * nblk first)
                b.close_stage(tail_st_op, tail_rec);
                tail_st_op = -1;
            }
            int res = x;
            if (i == 0 && !fuse) {
                res = b.tensor(Ho, Ho, P, pre + ".downsample");
                b.conv({pre + ".downsample"}, x, 0, C, res, 0, 1, 1, 2, 2, 0, 0, 0);
            }
            const int y = b.tensor(Ho, Ho, P, pre);
            if (fuse)  // y = conv2(t) + downsample(x) in one K loop (no downsample tensor)
                b.conv_ds({pre + ".conv2"}, hmid, 0, P, y, 0, 3, 3, st, st, 1, 1, 0, -1, 0, -1, "", pre + ".downsample",
                          x, C, 2);
            else
                b.conv({pre + ".conv2"}, hmid, 0, P, y, 0, 3, 3, st, st, 1, 1, 0, res, 0);
            if (tr && !b.rc) {
                StageRec t;
                t.kind = STAGE_TRANS;
                t.in = x; t.out = y; t.nblk = 1; t.H = H; t.C = P;
                t.conv_ops = {(int)h->ops.size() - 2, (int)h->ops.size() - 1};
                t.t_tensors = {hmid};
                t.x_tensors = {y};
                b.close_stage(tr_op, t);
            }
            if (st_op >= 0 && !b.rc) {
                rec.conv_ops.push_back((int)h->ops.size() - 2);
                rec.conv_ops.push_back((int)h->ops.size() - 1);
                rec.t_tensors.push_back(hmid);
                rec.x_tensors.push_back(y);
            }
            x = y;
            C = P;
        }
        close_stage(true);
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
    h->ops.push_back(Op{OP_PRE, -1, 0, 0, in});
    const int c1 = b.tensor(56, 56, 64, "backbone.relu");
    // conv1 + maxpool are also emitted as one launch (conv_stem_r50.hip) beside the member ops
    const bool st = h->dtype != FR_DTYPE_FP8;
    const int st_op = st ? b.open_stage() : -1;
    b.stem = true;
    b.conv({"backbone.conv1"}, in, 0, 8, c1, 0, 7, 7, 2, 2, 3, 3, 1);
    int x = b.tensor(28, 28, 64, "backbone.maxpool");
    b.maxpool(c1, x, 0, 3, 2, 1);
    if (st && !b.rc) {
        StageRec sr;
        sr.kind = STAGE_STEM_R50;
        sr.in = in; sr.out = x; sr.H = 112; sr.C = 8; sr.nblk = 1;
        sr.conv_ops = {st_op + 1, st_op + 2};
        const Op& cv = h->ops[st_op + 1];
        const DevConvW& cw = h->convw[cv.wi];
        if (!stem_r50_supported(112, 112, cv.cin, cw.K, cw.Kpad, cw.Cout) || cw.w8 || !cw.bias || cv.act != 1 ||
            cv.sh != 2 || cv.ph != 3 || cv.res >= 0 || h->ops[st_op + 2].kind != OP_MAXPOOL) {
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
            const size_t op0 = h->ops.size();
            const int s = i == 0 ? strd[l] : 1;
            const int Ho = (H + 2 - 3) / s + 1;
            const int h1 = b.tensor(H, H, P);
            b.conv({pre + ".conv1"}, x, 0, C, h1, 0, 1, 1, 1, 1, 0, 0, 1);
            const int h2 = b.tensor(Ho, Ho, P);
            b.conv({pre + ".conv2"}, h1, 0, P, h2, 0, 3, 3, s, s, 1, 1, 1);
            int id = x;
            const bool fuse = i == 0 && b.fuse_ds(P, C, pre);
            if (i == 0 && !fuse) {
                id = b.tensor(Ho, Ho, 4 * P, pre + ".downsample");
                b.conv({pre + ".downsample"}, x, 0, C, id, 0, 1, 1, s, s, 0, 0, 0);
            }
            const int y = b.tensor(Ho, Ho, 4 * P, pre);
            if (fuse)  // y = relu(conv3(h2) + downsample(x)) in one K loop
                b.conv_ds({pre + ".conv3"}, h2, 0, P, y, 0, 1, 1, 1, 1, 0, 0, 1, -1, 0, -1, "", pre + ".downsample", x, C, s);
            else
                b.conv({pre + ".conv3"}, h2, 0, P, y, 0, 1, 1, 1, 1, 0, 0, 1, id, 0);
            if (ch_op >= 0 && l == 2 && i >= 1)
                for (size_t k = op0; k < h->ops.size(); ++k) ch.conv_ops.push_back((int)k);
            if (bn_op >= 0 && l == 0) {
                for (size_t k = op0; k < h->ops.size(); ++k) bn.conv_ops.push_back((int)k);
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
    const int in = b.tensor(160, 160, 8);
    h->ops.push_back(Op{OP_PRE, -1, 0, 0, in});
    const int a = b.tensor(79, 79, 32, m + "conv2d_1a");
    const int bb = b.tensor(77, 77, 32, m + "conv2d_2a");
    const int c = b.tensor(77, 77, 64, m + "conv2d_2b");
    const int d = b.tensor(38, 38, 64, m + "maxpool_3a");
    const int e = b.tensor(38, 38, 80, m + "conv2d_3b");
    const int f = b.tensor(36, 36, 192, m + "conv2d_4a");
    int x = b.tensor(17, 17, 256, m + "conv2d_4b");
    // bf16 plan: the high-resolution stem (input .. conv2d_4a) is stored and multiplied in f16.  Its
    // activations are ~90 % of the forward's bf16 rounding drift (profiles/r02_irv1_drift_bf16_vs_f16.txt:
    // 1.28e-2 of 1.61e-2 relative error is in place at conv2d_4b); f16 MFMAs run at the bf16 rate, and
    // conv2d_4b writes bf16 for the rest of the network.  FR_IRV1_BF16_STEM=1 keeps it bf16 (A/B).
    static const bool bf16_stem = [] {
        const char* e = getenv("FR_IRV1_BF16_STEM");
        return e && e[0] == '1';
    }();
    if (h->dtype == FR_DTYPE_BF16 && !bf16_stem)
        for (int t : {in, a, bb, c, d, e, f}) h->tensors[t].f16 = true;
    // Round 6: the f16 section also covers conv2d_4b's output, repeat_1 (Block35 x5) and mixed_6a's inner branch
    // tensors; mixed_6a's convs and max-pool write the bf16 concat (the section boundary).  With the stem alone in f16
    // the bf16 body still moved bs = 256 embeddings up to 8.9e-4 (1 - cos) from the fp32 oracle and flipped 7 % of
    // the non-planted top-1 matches; f16 MFMAs run at the bf16 rate.  FR_AB irv1_f16_mid=0: the
    // round-5 boundary at conv2d_4b (A/B).
    // FR_AB irv1_f16_mid=2 (default): through repeat_2 (Block17 x10) too, the boundary at mixed_7a's outputs
    static const int f16_mid = ab_int("irv1_f16_mid", 2);
    const bool mid16 = h->dtype == FR_DTYPE_BF16 && !bf16_stem && f16_mid >= 1;
    const bool mid16b = mid16 && f16_mid >= 2;
    if (mid16) h->tensors[x].f16 = true;
    b.stem = true;
    // conv2d_1a .. conv2d_3b also as one launch (conv_stem160.hip) beside the member ops, measured per batch size
    const int st_op = h->dtype != FR_DTYPE_FP8 ? b.open_stage() : -1;
    b.conv({m + "conv2d_1a"}, in, 0, 8, a, 0, 3, 3, 2, 2, 0, 0, 1);
    b.conv({m + "conv2d_2a"}, a, 0, 32, bb, 0, 3, 3, 1, 1, 0, 0, 1);
    b.conv({m + "conv2d_2b"}, bb, 0, 32, c, 0, 3, 3, 1, 1, 1, 1, 1);
    b.maxpool(c, d, 0, 3, 2, 0);
    b.conv({m + "conv2d_3b"}, d, 0, 64, e, 0, 1, 1, 1, 1, 0, 0, 1);
    if (st_op >= 0 && !b.rc) {
        StageRec sr;
        sr.kind = STAGE_STEM160;
        sr.in = in; sr.out = e; sr.H = 160; sr.C = 80; sr.nblk = 1;
        const int n = (int)h->ops.size();
        sr.conv_ops = {n - 5, n - 4, n - 3, n - 2, n - 1};
        const Op& o1 = h->ops[n - 5];
        const Op& o2 = h->ops[n - 4];
        const Op& o3 = h->ops[n - 3];
        const Op& o4 = h->ops[n - 1];
        const DevConvW& c1 = h->convw[o1.wi];
        const DevConvW& c2 = h->convw[o2.wi];
        const DevConvW& c3 = h->convw[o3.wi];
        const DevConvW& c4 = h->convw[o4.wi];
        bool ok = stem160_supported(160, 160, 8, c1.K, c2.K, c3.K, c4.K, c1.Cout, c2.Cout, c3.Cout, c4.Cout) &&
                  h->tensors[in].f16 == h->tensors[e].f16 && o1.act == 1 && o2.act == 1 && o3.act == 1 && o4.act == 1;
        for (const DevConvW* cw : {&c1, &c2, &c3, &c4}) ok = ok && cw->bias && !cw->bias9 && !cw->w8;
        b.close_stage(st_op, sr, ok);  // not ok: no fused stem for these weights, the member ops only
    }
    b.conv({m + "conv2d_4a"}, e, 0, 80, f, 0, 3, 3, 1, 1, 0, 0, 1);
    b.conv({m + "conv2d_4b"}, f, 0, 192, x, 0, 3, 3, 2, 2, 0, 0, 1);
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
        const int cat = b.tensor(17, 17, 160);
        if (mid16) h->tensors[cat].f16 = true;
        b.conv({p + "branch1.0", p + "branch2.0", p + "branch0"}, x, 0, 256, cat, 0, 1, 1, 1, 1, 0, 0, 1);
        b.conv({p + "branch1.1"}, cat, 0, 32, cat, 96, 3, 3, 1, 1, 1, 1, 1);
        const int t = b.tensor(17, 17, 32);
        if (mid16) h->tensors[t].f16 = true;
        b.conv({p + "branch2.1"}, cat, 32, 32, t, 0, 3, 3, 1, 1, 1, 1, 1);
        b.conv({p + "branch2.2"}, t, 0, 32, cat, 128, 3, 3, 1, 1, 1, 1, 1);
        const int y = b.tensor(17, 17, 256, m + "repeat_1." + std::to_string(i));
        if (mid16) h->tensors[y].f16 = true;
        b.conv({p + "conv2d"}, cat, 64, 96, y, 0, 1, 1, 1, 1, 0, 0, 1, x, 0);
        if (c35_op >= 0) {
            for (int k = 5; k >= 1; --k) c35.conv_ops.push_back((int)h->ops.size() - k);
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
        const int cat = b.tensor(8, 8, 896, m + "mixed_6a");
        if (mid16b) h->tensors[cat].f16 = true;
        b.conv({p + "branch0"}, x, 0, 256, cat, 0, 3, 3, 2, 2, 0, 0, 1);
        const int u = b.tensor(17, 17, 192), v = b.tensor(17, 17, 192);
        if (mid16) h->tensors[u].f16 = h->tensors[v].f16 = true;
        b.conv({p + "branch1.0"}, x, 0, 256, u, 0, 1, 1, 1, 1, 0, 0, 1);
        b.conv({p + "branch1.1"}, u, 0, 192, v, 0, 3, 3, 1, 1, 1, 1, 1);
        b.conv({p + "branch1.2"}, v, 0, 192, cat, 384, 3, 3, 2, 2, 0, 0, 1);
        b.maxpool(x, cat, 640, 3, 2, 0);
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
        const int cat = b.tensor(8, 8, 384);
        const int t = b.tensor(8, 8, 128);
        const int y = b.tensor(8, 8, 896, m + "repeat_2." + std::to_string(i));
        if (mid16b) h->tensors[cat].f16 = h->tensors[t].f16 = h->tensors[y].f16 = true;
        b.conv({p + "branch1.0", p + "branch0"}, x, 0, 896, cat, 0, 1, 1, 1, 1, 0, 0, 1);
        b.conv({p + "branch1.1"}, cat, 0, 128, t, 0, 1, 7, 1, 1, 0, 3, 1);
        b.conv({p + "branch1.2"}, t, 0, 128, cat, 256, 7, 1, 1, 1, 3, 0, 1);
        b.conv({p + "conv2d"}, cat, 128, 256, y, 0, 1, 1, 1, 1, 0, 0, 1, x, 0);
        if (ch_op >= 0)
            for (int k = 4; k >= 1; --k) ch.conv_ops.push_back((int)h->ops.size() - k);
        x = y;
    }
    if (ch_op >= 0) {
        ch.out = x;
        b.close_stage(ch_op, ch);
    }
    {  // mixed_7a
        const std::string p = m + "mixed_7a.";
        const int cat = b.tensor(3, 3, 1792, m + "mixed_7a");
        const int u = b.tensor(8, 8, 768);
        if (mid16b) h->tensors[u].f16 = true;
        b.conv({p + "branch0.0", p + "branch1.0", p + "branch2.0"}, x, 0, 896, u, 0, 1, 1, 1, 1, 0, 0, 1);
        b.conv({p + "branch0.1"}, u, 0, 256, cat, 0, 3, 3, 2, 2, 0, 0, 1);
        b.conv({p + "branch1.1"}, u, 256, 256, cat, 384, 3, 3, 2, 2, 0, 0, 1);
        const int v = b.tensor(8, 8, 256);
        if (mid16b) h->tensors[v].f16 = true;
        b.conv({p + "branch2.1"}, u, 512, 256, v, 0, 3, 3, 1, 1, 1, 1, 1);
        b.conv({p + "branch2.2"}, v, 0, 256, cat, 640, 3, 3, 2, 2, 0, 0, 1);
        b.maxpool(x, cat, 896, 3, 2, 0);
        x = cat;
    }
    // repeat_3: Block8 x5 + final block8 (noReLU) @3x3. cat layout [t1 | b0 | b1]; conv2d reads [192:576].
    for (int i = 0; i < 6; ++i) {
        const std::string p = i < 5 ? m + "repeat_3." + std::to_string(i) + "." : m + "block8.";
        const int cat = b.tensor(3, 3, 576);
        b.conv({p + "branch1.0", p + "branch0"}, x, 0, 1792, cat, 0, 1, 1, 1, 1, 0, 0, 1);
        const int t = b.tensor(3, 3, 192);
        b.conv({p + "branch1.1"}, cat, 0, 192, t, 0, 1, 3, 1, 1, 0, 1, 1);
        b.conv({p + "branch1.2"}, t, 0, 192, cat, 384, 3, 1, 1, 1, 1, 0, 1);
        const int y = b.tensor(3, 3, 1792, i < 5 ? m + "repeat_3." + std::to_string(i) : m + "block8");
        b.conv({p + "conv2d"}, cat, 192, 384, y, 0, 1, 1, 1, 1, 0, 0, i < 5 ? 1 : 0, x, 0);
        x = y;
    }
    // fr_explain: the activation map of block8.conv2d's own output.  That conv writes conv + x, so fr_explain runs
    // it once more without the residual into this scratch tensor (never the difference of two bf16 tensors)
    if (!b.rc) {
        h->ex_conv = (int)h->ops.size() - 1;
        h->ex_tensor = b.tensor(3, 3, 1792);
        h->ex_layout = 2;
    }
    const int pool = b.tensor(1, 1, 1792, m + "avgpool_1a");
    b.avgpool(x, pool);
    b.head(pool);
    b.projection();
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
                if (op.out2 >= 0) wr[oi].push_back({op.out2, 0, cw.Cout});
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
                        cv.res < 0 && cv.out2 < 0 && cv.sh == 1 && cv.ph == 1 && cv.kh == 3 && cv.kw == 3) {
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
    std::unordered_map<std::string, HostT> W;
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
    Builder b{h, W};
    if (h->arch == FR_ARCH_IRESNET100) build_iresnet100(b);
    else if (h->arch == FR_ARCH_RESNET50_ARCFACE) build_resnet50(b);
    else build_irv1(b);
    if (!b.rc) b.rc = pack_conv_weights(h);
    for (auto& op : h->ops) op.grp = op.stage;  // plan entries (stage_plan)
    // the tensors whose producers record amax: inputs of e4m3 convs that run per-conv (an fp8 stage
    // scales its own input; its member convs are its fallback when the stage does not run)
    h->need_amax.assign(h->tensors.size(), 0);
    for (const auto& op : h->ops)
        if (op.kind == OP_CONV && op.wi >= 0 && h->convw[op.wi].w8 && op.in_off == 0) h->need_amax[op.in] = 1;
    if (b.rc) {
        free_weights(h);
        h->tensors.clear();
        h->ops.clear();
        DevSerial::reg(h, false);
        return b.rc;
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

int fr_gallery_set(fr_handle* h, const float* G, int64_t N, int D, int64_t index_base, int g_on_device) {
    if (!h || (!G && N > 0) || N < 0 || D <= 0 || D % 4 != 0 || N + index_base > INT32_MAX) {
        set_error("fr_gallery_set: bad argument (D must be a multiple of 4, indices must fit int32)");
        return FR_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    FR_HIP_CHECK(hipSetDevice(h->device));
    if (h->gallery) { (void)hipFree(h->gallery); h->gallery = nullptr; }
    if (h->g_hi) { (void)hipFree(h->g_hi); h->g_hi = nullptr; }
    h->g_rows = 0;
    h->g_cap = N;
    if (N > 0) {
        void* p = nullptr;
        int rc = dev_alloc(&p, (size_t)N * D * sizeof(float));
        if (rc) return rc;
        h->gallery = (float*)p;
        FR_HIP_CHECK(hipMemcpy(p, G, (size_t)N * D * sizeof(float),
                               g_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        FR_HIP_CHECK(launch_gallery_prepare(h->gallery, N, D, nullptr));
        if (N >= h->x3_min_rows && D == 512) {  // bf16 hi/lo copy for the candidate pass (match_x3.hip)
            int rc2 = dev_alloc((void**)&h->g_hi, x3_gallery_elems(N) * sizeof(bf16_t));
            if (!rc2) FR_HIP_CHECK(hipMemset(h->g_hi, 0, x3_gallery_elems(N) * sizeof(bf16_t)));
            if (!rc2 && !h->match_fb) {
                rc2 = dev_alloc((void**)&h->match_fb, sizeof(int));
                if (!rc2) FR_HIP_CHECK(hipMemset(h->match_fb, 0, sizeof(int)));
            }
            if (rc2) return rc2;
            FR_HIP_CHECK(launch_split_x3(h->gallery, 0, N, h->g_hi, nullptr));
        }
        FR_HIP_CHECK(hipDeviceSynchronize());
    }
    h->g_rows = N;
    h->g_dim = D;
    h->g_base = index_base;
    return FR_OK;
}

// Rows [row0, row0 + n) of the gallery from G (host or device): an in-place update of existing rows and/or an
// append (row0 <= rows).  Only the written rows are prepared (norm rule) and, on the bf16x3 path, split;
// appends grow the allocation geometrically, so n single-row appends cost O(n) row copies amortised
// instead of a full re-upload each (a served gallery under add_to_db traffic).
int fr_gallery_write(fr_handle* h, const float* G, int64_t row0, int64_t n, int D, int g_on_device) {
    if (!h || !G || n <= 0 || row0 < 0 || D <= 0 || D % 4 != 0) {
        set_error("fr_gallery_write: bad argument");
        return FR_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->g_rows > 0 && D != h->g_dim) { set_error("fr_gallery_write: D differs from the gallery's"); return FR_ERR_ARG; }
    if (row0 > h->g_rows) { set_error("fr_gallery_write: row0 past the end (appends must be contiguous)"); return FR_ERR_ARG; }
    const int64_t rows = std::max(h->g_rows, row0 + n);
    if (rows + h->g_base > INT32_MAX) { set_error("fr_gallery_write: indices must fit int32"); return FR_ERR_ARG; }
    FR_HIP_CHECK(hipSetDevice(h->device));
    // once split, a gallery stays on the bf16x3 path (match_locked takes it whenever g_hi exists), so every
    // written row must be re-split even if FR_OPT_X3_MIN_ROWS was raised since
    const bool x3 = (h->g_hi != nullptr || rows >= h->x3_min_rows) && D == 512;
    if (rows > h->g_cap || !h->gallery) {  // grow: 2x, copy the old rows on the device
        const int64_t cap = std::max<int64_t>(rows, std::max<int64_t>(2 * h->g_cap, 1024));
        float* g = nullptr;
        int rc = dev_alloc((void**)&g, (size_t)cap * D * sizeof(float));
        if (rc) return rc;
        if (h->g_rows > 0)
            FR_HIP_CHECK(hipMemcpy(g, h->gallery, (size_t)h->g_rows * D * sizeof(float), hipMemcpyDeviceToDevice));
        if (h->gallery) (void)hipFree(h->gallery);
        h->gallery = g;
        if (h->g_hi) { (void)hipFree(h->g_hi); h->g_hi = nullptr; }  // re-split below at the new capacity
        h->g_cap = cap;
    }
    FR_HIP_CHECK(hipMemcpy(h->gallery + (size_t)row0 * D, G, (size_t)n * D * sizeof(float),
                           g_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    FR_HIP_CHECK(launch_gallery_prepare(h->gallery + (size_t)row0 * D, n, D, nullptr));
    if (x3) {
        int64_t s0 = row0, sn = n;
        if (!h->g_hi) {  // first time on the bf16x3 path (or re-grown): split every row
            int rc = dev_alloc((void**)&h->g_hi, x3_gallery_elems(h->g_cap) * sizeof(bf16_t));
            if (!rc) FR_HIP_CHECK(hipMemset(h->g_hi, 0, x3_gallery_elems(h->g_cap) * sizeof(bf16_t)));
            if (!rc && !h->match_fb) {
                rc = dev_alloc((void**)&h->match_fb, sizeof(int));
                if (!rc) FR_HIP_CHECK(hipMemset(h->match_fb, 0, sizeof(int)));
            }
            if (rc) return rc;
            s0 = 0;
            sn = rows;
        }
        FR_HIP_CHECK(launch_split_x3(h->gallery, s0, sn, h->g_hi, nullptr));
    }
    FR_HIP_CHECK(hipDeviceSynchronize());
    h->g_rows = rows;
    h->g_dim = D;
    return FR_OK;
}

int64_t fr_gallery_rows(const fr_handle* h) { return h ? h->g_rows : 0; }

static int ensure_cand(fr_handle* h, size_t need) {
    if (need <= h->cand_cap) return FR_OK;
    if (h->cand_s) (void)hipFree(h->cand_s);
    if (h->cand_i) (void)hipFree(h->cand_i);
    h->cand_s = nullptr;
    h->cand_i = nullptr;
    h->cand_cap = 0;
    int rc = dev_alloc((void**)&h->cand_s, need * sizeof(float));
    if (rc) return rc;
    rc = dev_alloc((void**)&h->cand_i, need * sizeof(int32_t));
    if (rc) return rc;
    h->cand_cap = need;
    return FR_OK;
}

// FR_AB no_match_rows: small batches take the MFMA match kernels too (A/B timing)
static bool match_rows_enabled() {
    static const bool on = [] { return !ab_int("no_match_rows", 0); }();
    return on;
}

static int match_locked(fr_handle* h, const float* P, int B, int k, float* scores, int32_t* idx, void* stream) {
    if (!P || !scores || !idx || B <= 0 || k <= 0 || k > FR_TOPK_LARGE_MAX) {
        set_error("fr_match_topk: bad argument (1 <= k <= " + std::to_string(FR_TOPK_LARGE_MAX) + ")");
        return FR_ERR_ARG;
    }
    if (!h->gallery || h->g_rows <= 0) { set_error("fr_match_topk: no gallery"); return FR_ERR_STATE; }
    FR_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (k > 16) {  // exact score rows in stream-ordered scratch, <= 256 MiB per probe chunk, + radix select
        if (h->g_rows > 0x7fffffff) { set_error("fr_match_topk: k > 16 needs a gallery below 2^31 rows"); return FR_ERR_ARG; }
        const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 26) / h->g_rows));
        float* S = nullptr;
        FR_HIP_CHECK(hipMallocAsync((void**)&S, (size_t)chunk * h->g_rows * sizeof(float), s));
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0);
            const hipError_t e = launch_match_topk_large(P + (size_t)b0 * h->g_dim, nb, h->gallery, h->g_rows, h->g_dim, k,
                                                         h->g_base, S, scores + (size_t)b0 * k, idx + (size_t)b0 * k, s);
            if (e != hipSuccess) {
                (void)hipFreeAsync(S, s);
                FR_HIP_CHECK(e);
            }
        }
        FR_HIP_CHECK(hipFreeAsync(S, s));
        return FR_OK;
    }
    int n_split;
    int64_t rps;
    // B <= 4 (the online bs = 1 path): one wave per 64 rows, exact f32 scores in the f32 kernels' order
    if (match_rows_enabled() && match_rows_supported(B, h->g_dim, k)) {
        int n_lists, R;
        match_rows_plan(h->g_rows, &n_lists, &R);
        int rc = ensure_cand(h, (size_t)B * n_lists * k);
        if (rc) return rc;
        FR_HIP_CHECK(launch_match_rows(P, B, h->gallery, h->g_rows, h->g_dim, k, h->g_base, h->cand_s, h->cand_i,
                                       n_lists, R, s));
        FR_HIP_CHECK(launch_topk_merge(h->cand_s, h->cand_i, B, n_lists, k, scores, idx, s));
        return FR_OK;
    }
    // bf16x3 candidates + exact f32 rescoring (match_x3.hip).  Its proof needs the k-th exact score to
    // clear the 16th candidate by 2 eps, which a k close to 16 almost never does (every probe would be
    // rescanned by one wave), so k > 8 takes the exact kernel.
    if (h->g_hi && !h->match_exact && 2 * k <= match_x3_candidates()) {
        match_x3_plan(B, h->g_rows, &n_split, &rps);
        int rc = ensure_cand(h, (size_t)B * n_split * match_x3_candidates());
        if (rc) return rc;
        FR_HIP_CHECK(launch_match_x3(P, B, h->gallery, h->g_hi, h->g_rows, h->g_dim, k, h->g_base, h->cand_s,
                                     h->cand_i, n_split, rps, scores, idx, h->match_fb, s));
        return FR_OK;
    }
    match_split_plan(B, h->g_rows, h->g_dim, k, &n_split, &rps);
    int rc = ensure_cand(h, (size_t)B * n_split * k);
    if (rc) return rc;
    FR_HIP_CHECK(launch_match_topk(P, B, h->gallery, h->g_rows, h->g_dim, k, h->g_base, h->cand_s, h->cand_i,
                                   n_split, rps, s));
    FR_HIP_CHECK(launch_topk_merge(h->cand_s, h->cand_i, B, n_split, k, scores, idx, s));
    return FR_OK;
}

int fr_match_topk(fr_handle* h, const float* P, int B, int k, float* scores, int32_t* idx, void* stream) {
    if (!h) { set_error("fr_match_topk: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    return match_locked(h, P, B, k, scores, idx, stream);
}

int fr_match_eval(fr_handle* h, const float* P, int B, const int32_t* true_idx, int k, float* scores, int32_t* idx,
                  float* true_score, int32_t* true_rank, uint64_t* hist, int nbins, float lo, float hi, void* stream) {
    const bool want_topk = k != 0;  // k = 0: scores / idx are not written (and may be NULL)
    if (!P || !true_idx || !true_score || !true_rank || B <= 0) {
        set_error("fr_match_eval: bad argument (P, true_idx, true_score, true_rank must be set, B >= 1)");
        return FR_ERR_ARG;
    }
    if (want_topk && (k <= 0 || !scores || !idx)) {
        set_error("fr_match_eval: bad argument (k >= 1 with scores and idx, or k = 0 for no top-k)");
        return FR_ERR_ARG;
    }
    if (hist && (nbins < 1 || nbins > 2048 || !(hi > lo))) {
        set_error("fr_match_eval: bad argument (1 <= nbins <= 2048 and hi > lo with a histogram)");
        return FR_ERR_ARG;
    }
    if (!h) { set_error("fr_match_eval: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->gallery || h->g_rows <= 0) { set_error("fr_match_eval: no gallery"); return FR_ERR_STATE; }
    if (h->g_rows > 0x7fffffff) { set_error("fr_match_eval: needs a gallery below 2^31 rows"); return FR_ERR_ARG; }
    if (want_topk) {  // fr_match_topk's launches, unchanged
        int rc = match_locked(h, P, B, k, scores, idx, stream);
        if (rc) return rc;
    }
    FR_HIP_CHECK(hipSetDevice(h->device));
    const float inv_w = hist ? (float)nbins / (hi - lo) : 0.f;  // rounded once, here
    FR_HIP_CHECK(launch_match_eval(P, B, h->gallery, h->g_rows, h->g_dim, h->g_base, true_idx, true_score, true_rank,
                                   (unsigned long long*)hist, nbins, lo, inv_w, (hipStream_t)stream));
    return FR_OK;
}

int fr_debug_match_eval_splits(fr_handle* h, int B) {
    if (!h || B <= 0) { set_error("fr_debug_match_eval_splits: bad argument"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->gallery || h->g_rows <= 0) { set_error("fr_debug_match_eval_splits: no gallery"); return FR_ERR_STATE; }
    int n_split;
    int64_t rps;
    match_eval_plan(B, h->g_rows, h->g_dim, &n_split, &rps);
    return n_split;
}

size_t fr_match_range_workspace(const fr_handle* h, int B) {
    if (!h || B <= 0) { set_error("fr_match_range_workspace: bad argument"); return 0; }
    fr_handle* hm = const_cast<fr_handle*>(h);
    std::lock_guard<std::mutex> lk(hm->mu);
    if (!h->gallery || h->g_rows <= 0) { set_error("fr_match_range_workspace: no gallery"); return 0; }
    const size_t n = match_range_workspace(B, h->g_rows, h->g_dim);
    if (!n) set_error("fr_match_range_workspace: needs a gallery below 2^31 rows");
    return n;
}

// The checks fr_match_range_count and fr_match_range_fill share, past their own pointer arguments.
static int range_state_check(fr_handle* h, const char* who) {
    if (!h->gallery || h->g_rows <= 0) { set_error(std::string(who) + ": no gallery"); return FR_ERR_STATE; }
    if (h->g_rows > 0x7fffffff) { set_error(std::string(who) + ": needs a gallery below 2^31 rows"); return FR_ERR_ARG; }
    return FR_OK;
}

int fr_match_range_count(fr_handle* h, const float* P, int B, float thresh, const int32_t* after, void* ws,
                         int64_t* lims, void* stream) {
    if (!P || !ws || !lims || B <= 0 || std::isnan(thresh)) {
        set_error("fr_match_range_count: bad argument (P, ws, lims must be set, B >= 1, thresh not NaN)");
        return FR_ERR_ARG;
    }
    if (!h) { set_error("fr_match_range_count: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = range_state_check(h, "fr_match_range_count")) return rc;
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(launch_match_range_count(P, B, h->gallery, h->g_rows, h->g_dim, h->g_base, thresh, after, (int32_t*)ws,
                                          lims, (hipStream_t)stream));
    return FR_OK;
}

int fr_match_range_fill(fr_handle* h, const float* P, int B, float thresh, const int32_t* after, const void* ws,
                        const int64_t* lims, float* scores, int32_t* idx, int64_t capacity, void* stream) {
    if (!P || !ws || !lims || !scores || !idx || B <= 0 || std::isnan(thresh) || capacity < 0) {
        set_error("fr_match_range_fill: bad argument (P, ws, lims, scores, idx must be set, B >= 1, thresh not NaN, "
                  "capacity >= 0)");
        return FR_ERR_ARG;
    }
    if (!h) { set_error("fr_match_range_fill: null handle"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = range_state_check(h, "fr_match_range_fill")) return rc;
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(launch_match_range_fill(P, B, h->gallery, h->g_rows, h->g_dim, h->g_base, thresh, after,
                                         (const int32_t*)ws, lims, scores, idx, capacity, (hipStream_t)stream));
    return FR_OK;
}

int fr_debug_match_range_splits(fr_handle* h, int B) {
    if (!h || B <= 0) { set_error("fr_debug_match_range_splits: bad argument"); return FR_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->gallery || h->g_rows <= 0) { set_error("fr_debug_match_range_splits: no gallery"); return FR_ERR_STATE; }
    int n_split;
    int64_t rps;
    match_range_plan(B, h->g_rows, h->g_dim, &n_split, &rps);
    return n_split;
}

int fr_gallery_read(const fr_handle* h, int64_t row0, int64_t n, float* out, int out_on_device) {
    if (row0 < 0 || n < 0 || (!out && n > 0)) {
        set_error("fr_gallery_read: bad argument (row0 >= 0, n >= 0, out must be set)");
        return FR_ERR_ARG;
    }
    if (!h) { set_error("fr_gallery_read: null handle"); return FR_ERR_ARG; }
    fr_handle* hm = const_cast<fr_handle*>(h);
    std::lock_guard<std::mutex> lk(hm->mu);
    if (row0 > h->g_rows || n > h->g_rows - row0) {
        set_error("fr_gallery_read: rows [" + std::to_string(row0) + ", " + std::to_string(row0) + " + " +
                  std::to_string(n) + ") outside a gallery of " + std::to_string(h->g_rows) + " rows");
        return FR_ERR_ARG;
    }
    if (n == 0) return FR_OK;
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(hipMemcpy(out, h->gallery + (size_t)row0 * h->g_dim, (size_t)n * h->g_dim * sizeof(float),
                           out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return FR_OK;
}

int fr_topk_merge(const float* cand_s, const int32_t* cand_i, int B, int n_lists, int k, float* scores,
                  int32_t* idx, void* stream) {
    if (!cand_s || !cand_i || !scores || !idx || B <= 0 || n_lists <= 0 || k <= 0 || k > 16) {
        set_error("fr_topk_merge: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_topk_merge(cand_s, cand_i, B, n_lists, k, scores, idx, (hipStream_t)stream));
    return FR_OK;
}

int fr_topk_merge_ranks(const void* xchg, int n_ranks, int B, int k, float* scores, int32_t* idx, void* stream) {
    if (!xchg || !scores || !idx || B <= 0 || n_ranks <= 0 || k <= 0 || k > 16) {
        set_error("fr_topk_merge_ranks: bad argument");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_topk_merge_ranks(xchg, n_ranks, B, k, scores, idx, (hipStream_t)stream));
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

int fr_debug_match_fallbacks(fr_handle* h) {
    if (!h) return FR_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->match_fb) return 0;
    int v = 0;
    FR_HIP_CHECK(hipSetDevice(h->device));
    FR_HIP_CHECK(hipDeviceSynchronize());
    FR_HIP_CHECK(hipMemcpy(&v, h->match_fb, sizeof(int), hipMemcpyDeviceToHost));
    return v;
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
