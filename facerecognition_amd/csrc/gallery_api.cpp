// C ABI of the gallery and the matcher (include/frhip.h "gallery + match"): the handle's gallery rows, and the argument
// checks and kernel choice in front of the match*.hip launches.  fr_embed_match (engine.cpp) matches through match_locked.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>

#include "engine_internal.h"

using namespace fr;

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

int fr::match_locked(fr_handle* h, const float* P, int B, int k, float* scores, int32_t* idx, void* stream) {
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

extern "C" {

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

}  // extern "C"
