// C ABI of the t-SNE ops (include/frhip.h "t-SNE"): the argument checks in front of tsne.hip's launches.  Handle-free,
// like the fr_lbph_* ops.  Every argument is checked before the first HIP call.
#include <cmath>
#include <string>

#include "engine_internal.h"

namespace fr {

static bool tsne_shape_ok(const char* fn, int N, int k) {
    if (N < 2) { set_error(std::string(fn) + ": N must be at least 2"); return false; }
    if (k < 1 || k >= N || k > 4095) { set_error(std::string(fn) + ": k must be 1..min(N - 1, 4095)"); return false; }
    if (2 * (int64_t)N * k >= (int64_t(1) << 31)) { set_error(std::string(fn) + ": 2 N k must be below 2^31"); return false; }
    return true;
}

static bool tsne_n_ok(const char* fn, int N) {
    if (N < 2 || N >= (1 << 30)) { set_error(std::string(fn) + ": N must be 2..2^30 - 1"); return false; }
    return true;
}

static bool tsne_positive(const char* fn, const char* what, float v) {
    if (!std::isfinite(v) || !(v > 0.f)) {
        set_error(std::string(fn) + ": " + what + " must be finite and positive");
        return false;
    }
    return true;
}

}  // namespace fr

using namespace fr;

extern "C" {

int fr_tsne_knn_sqdist(const float* X, int N, int D, const int32_t* idx, int k, float* d2, void* stream) {
    if (!tsne_shape_ok("fr_tsne_knn_sqdist", N, k)) return FR_ERR_ARG;
    if (D < 1) { set_error("fr_tsne_knn_sqdist: D must be at least 1"); return FR_ERR_ARG; }
    if (!X || !idx || !d2) { set_error("fr_tsne_knn_sqdist: null X, idx or d2"); return FR_ERR_ARG; }
    FR_HIP_CHECK(launch_tsne_knn_sqdist(X, N, D, idx, k, d2, (hipStream_t)stream));
    return FR_OK;
}

size_t fr_tsne_affinities_workspace(int N, int k) {
    if (!tsne_shape_ok("fr_tsne_affinities_workspace", N, k)) return 0;
    return tsne_affinities_workspace(N, k);
}

int fr_tsne_affinities(const int32_t* idx, const float* d2, int N, int k, float perplexity, int32_t* indptr,
                       int32_t* col, float* val, float* beta, void* ws, size_t ws_bytes, void* stream) {
    if (!tsne_shape_ok("fr_tsne_affinities", N, k)) return FR_ERR_ARG;
    if (!tsne_positive("fr_tsne_affinities", "perplexity", perplexity)) return FR_ERR_ARG;
    if (!idx || !d2 || !indptr || !col || !val || !beta || !ws) {
        set_error("fr_tsne_affinities: null buffer");
        return FR_ERR_ARG;
    }
    if (ws_bytes < tsne_affinities_workspace(N, k)) {
        set_error("fr_tsne_affinities: workspace smaller than fr_tsne_affinities_workspace");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_tsne_affinities(idx, d2, N, k, perplexity, indptr, col, val, beta, ws, (hipStream_t)stream));
    return FR_OK;
}

size_t fr_tsne_gradient_workspace(int N) {
    if (!tsne_n_ok("fr_tsne_gradient_workspace", N)) return 0;
    return tsne_gradient_workspace(N);
}

int fr_tsne_gradient(const int32_t* indptr, const int32_t* col, const float* val, int N, const float* Y,
                     float exaggeration, float* grad, double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!tsne_n_ok("fr_tsne_gradient", N)) return FR_ERR_ARG;
    if (!tsne_positive("fr_tsne_gradient", "exaggeration", exaggeration)) return FR_ERR_ARG;
    if (!indptr || !col || !val || !Y || !grad || !stats || !ws) {
        set_error("fr_tsne_gradient: null buffer");
        return FR_ERR_ARG;
    }
    if (ws_bytes < tsne_gradient_workspace(N)) {
        set_error("fr_tsne_gradient: workspace smaller than fr_tsne_gradient_workspace");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_tsne_steps(indptr, col, val, N, const_cast<float*>(Y), nullptr, nullptr, exaggeration, 0.f, 0.f,
                                   0, grad, stats, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_tsne_run(const int32_t* indptr, const int32_t* col, const float* val, int N, float* Y, float* update,
                float* gains, float exaggeration, float momentum, float learning_rate, int n_steps, float* grad,
                double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!tsne_n_ok("fr_tsne_run", N)) return FR_ERR_ARG;
    if (!tsne_positive("fr_tsne_run", "exaggeration", exaggeration) ||
        !tsne_positive("fr_tsne_run", "momentum", momentum) ||
        !tsne_positive("fr_tsne_run", "learning_rate", learning_rate))
        return FR_ERR_ARG;
    if (n_steps < 1 || n_steps > 100000) { set_error("fr_tsne_run: n_steps must be 1..100000"); return FR_ERR_ARG; }
    if (!indptr || !col || !val || !Y || !update || !gains || !grad || !stats || !ws) {
        set_error("fr_tsne_run: null buffer");
        return FR_ERR_ARG;
    }
    if (ws_bytes < tsne_gradient_workspace(N)) {
        set_error("fr_tsne_run: workspace smaller than fr_tsne_gradient_workspace");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_tsne_steps(indptr, col, val, N, Y, update, gains, exaggeration, momentum, learning_rate, n_steps,
                                   grad, stats, ws, (hipStream_t)stream));
    return FR_OK;
}

int fr_op_tsne_repulsion(const float* Y, int N, void* ws, size_t ws_bytes, void* stream) {
    if (!tsne_n_ok("fr_op_tsne_repulsion", N)) return FR_ERR_ARG;
    if (!Y || !ws) { set_error("fr_op_tsne_repulsion: null buffer"); return FR_ERR_ARG; }
    if (ws_bytes < tsne_gradient_workspace(N)) {
        set_error("fr_op_tsne_repulsion: workspace smaller than fr_tsne_gradient_workspace");
        return FR_ERR_ARG;
    }
    FR_HIP_CHECK(launch_tsne_repulsion(Y, N, ws, (hipStream_t)stream));
    return FR_OK;
}

}  // extern "C"
