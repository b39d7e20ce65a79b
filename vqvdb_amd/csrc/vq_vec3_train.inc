// vq_vec3_train.inc — codebook (EMA) training on the Vec3 handle (vqhip_vec3_train_*; include/vqvdb_hip_vec3_train.h,
// DESIGN.md §12).  Part of vq_runtime.hip's translation unit, after vq_vec3.inc: it drives the encoder chain and vq_k of
// the inference handle unchanged and adds the kernels of vq_vec3_train.h.

#include "../../include/vqvdb_hip_vec3_train.h"

namespace {

constexpr int64_t V3T_SEG_BUDGET = int64_t(1) << 22;   // entries of the per-(segment, code) count table
constexpr size_t V3T_ALIGN = 256;

// rows per counting-sort segment: 4096, doubled until the segment x code table stays within V3T_SEG_BUDGET entries
int v3t_seg_rows(int64_t rows, int k_codes)
{
    int64_t s = 4096;
    while ((rows + s - 1) / s * k_codes > V3T_SEG_BUDGET) s *= 2;
    return (int)s;
}

struct V3TWs {
    float* flat;       // [rows][64]           (used when the caller passes no latent buffer)
    uint16_t* idx;     // [rows]               (used when the caller passes no index buffer)
    int* list;         // [rows]               row ids sorted by code, stable
    int* seg;          // [n_seg][K]           counts, then offsets
    int* total;        // [K]
    int* start;        // [K+1]
    int* pstart;       // [K+1]
    float* part;       // [max_pieces][64]
    double* sqpart;    // [max_pieces]
    double* rl;        // [RL_BLOCKS][2]       reconstruction-loss partials
    int64_t max_pieces;
    size_t bytes;
};

// suballocation of a training workspace of `leaves` leaves (base NULL: sizes only)
V3TWs v3t_layout(unsigned char* base, int64_t leaves, int k_codes)
{
    const int64_t rows = leaves * 64;
    const int64_t seg_entries = std::min(V3T_SEG_BUDGET, (rows + 4095) / 4096 * k_codes);
    V3TWs w{};
    w.max_pieces = (rows + v3t::PIECE - 1) / v3t::PIECE + k_codes;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char* p = base ? base + off : nullptr;
        off += (bytes + V3T_ALIGN - 1) / V3T_ALIGN * V3T_ALIGN;
        return p;
    };
    w.flat = (float*)take((size_t)rows * 64 * sizeof(float));
    w.idx = (uint16_t*)take((size_t)rows * sizeof(uint16_t));
    w.list = (int*)take((size_t)rows * sizeof(int));
    w.seg = (int*)take((size_t)seg_entries * sizeof(int));
    w.total = (int*)take((size_t)k_codes * sizeof(int));
    w.start = (int*)take((size_t)(k_codes + 1) * sizeof(int));
    w.pstart = (int*)take((size_t)(k_codes + 1) * sizeof(int));
    w.part = (float*)take((size_t)w.max_pieces * 64 * sizeof(float));
    w.sqpart = (double*)take((size_t)w.max_pieces * sizeof(double));
    w.rl = (double*)take((size_t)RL_BLOCKS * 2 * sizeof(double));
    w.bytes = off;
    return w;
}

size_t v3t_ws_bytes(int64_t leaves, int k_codes) { return leaves > 0 ? v3t_layout(nullptr, leaves, k_codes).bytes : 0; }

int v3t_ensure_ws(vqhip_vec3_codec* c, int64_t m)
{
    if (m <= c->tr_leaves) return VQHIP_OK;
    if (int rc = ensure(c, c->tr_ws, v3t_ws_bytes(m, c->k_codes), [&](hipError_t) { return "vec3 training: cannot allocate the training workspace of " + std::to_string(m) + " leaves"; })) {
        if (!c->tr_ws) c->tr_leaves = 0;   // (a failed synchronise leaves the old block and its layout)
        c->chunk_fitted = false;
        return rc;
    }
    c->tr_leaves = m;
    return VQHIP_OK;
}

int v3t_require(vqhip_vec3_codec* c, const char* what)
{
    if (!c->training) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": call vqhip_vec3_train_begin first");
    return VQHIP_OK;
}

int v3t_check_batch(vqhip_vec3_codec* c, const char* what, const float* leaves, int64_t n, const float* stats)
{
    if (int rc = v3t_require(c, what)) return rc;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": n_leaves < 0");
    if (!stats) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": stats_dev is NULL");
    if (n > 0 && !leaves) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": leaves_dev is NULL");
    if (n > c->chunk)
        return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": " + std::to_string(n) + " leaves exceed the chunk of " + std::to_string(c->chunk) +
                                                 " (vqhip_vec3_chunk_leaves)");
    return VQHIP_OK;
}

// statistics of `rows` latent rows (flat [rows][64], idx [rows]) against the current codebook cb -> stats [66K+1]
int v3t_stats(vqhip_vec3_codec* c, const V3TWs& T, const float* flat, const uint16_t* idx, int64_t rows, float* stats, hipStream_t s)
{
    const int K = c->k_codes;
    int kbits = 0;
    while ((1 << kbits) < K) ++kbits;
    const int seg_rows = v3t_seg_rows(rows, K);
    const int n_seg = (int)((rows + seg_rows - 1) / seg_rows);
    HIPCHK(c, hipMemsetAsync(T.seg, 0, (size_t)n_seg * K * sizeof(int), s));
    hipLaunchKernelGGL(v3t::seg_hist_k, dim3(n_seg), dim3(64), 0, s, idx, rows, seg_rows, K, kbits, T.seg);
    hipLaunchKernelGGL(v3t::seg_scan_k, dim3((K + 255) / 256), dim3(256), 0, s, T.seg, n_seg, K, T.total);
    hipLaunchKernelGGL(v3t::code_scan_k, dim3(1), dim3(1024), 0, s, T.total, K, T.start, T.pstart);
    hipLaunchKernelGGL(v3t::seg_scatter_k, dim3(n_seg), dim3(64), 0, s, idx, rows, seg_rows, K, kbits, T.seg, T.start, T.list);
    const int64_t maxp = (rows + v3t::PIECE - 1) / v3t::PIECE + K;
    hipLaunchKernelGGL(v3t::piece_sum_k, dim3((unsigned)((maxp + 3) / 4)), dim3(256), 0, s, flat, T.list, T.start, T.pstart, c->w["cb"], K,
                       (int)maxp, T.part, T.sqpart);
    hipLaunchKernelGGL(v3t::code_reduce_k, dim3((K + 3) / 4), dim3(256), 0, s, T.part, T.sqpart, T.total, T.pstart, K, rows, stats);
    return v3_launch_check(c, "vec3 training statistics");
}

// encoder + assignment + flat latent + statistics of one batch (n <= chunk, n > 0); leaves W.z holding the latent
int v3t_forward(vqhip_vec3_codec* c, const float* leaves, int64_t n, float* stats, uint16_t* idx_out, float* latent_out, hipStream_t s,
                V3TWs& T, uint16_t** idx_used)
{
    if (int rc = v3_ensure_ws(c, n)) return rc;
    if (int rc = v3t_ensure_ws(c, n)) return rc;
    T = v3t_layout(c->tr_ws, c->tr_leaves, c->k_codes);
    uint16_t* idx = idx_out ? idx_out : T.idx;
    float* flat = latent_out ? latent_out : T.flat;
    if (int rc = v3_encode_chunk(c, leaves, n, idx, s)) return rc;
    hipLaunchKernelGGL(v3t::flat_k, dim3((unsigned)n), dim3(256), 0, s, v3_ws(c).z, flat, n);
    if (idx_used) *idx_used = idx;
    return v3t_stats(c, T, flat, idx, n * 64, stats, s);
}

int v3t_rebuild_tables(vqhip_vec3_codec* c, hipStream_t s)
{
    hipLaunchKernelGGL(v3t::tables_k, dim3((c->k_codes + 3) / 4), dim3(256), 0, s, c->w["cb"], c->k_codes, c->w["cb.f"], c->w["cb.ee"]);
    return v3_launch_check(c, "vec3 codebook tables");
}

}  // namespace

extern "C" {

int64_t vqhip_vec3_train_stats_floats(const vqhip_vec3_codec* c) { return c ? (int64_t)66 * c->k_codes + 1 : -1; }

int vqhip_vec3_train_begin(vqhip_vec3_codec* c, const float* cluster_size, const float* embed_avg)
{
    if (!c) return VQHIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const size_t K = (size_t)c->k_codes;
    auto nomem = [](hipError_t) { return std::string("vec3 train_begin: cannot allocate the EMA buffers"); };
    if (int rc = ensure(c, c->tr_cs, K, nomem)) return rc;
    if (int rc = ensure(c, c->tr_avg, K * 64, nomem)) return rc;
    if (cluster_size) HIPCHK(c, hipMemcpy(c->tr_cs, cluster_size, K * sizeof(float), hipMemcpyHostToDevice));
    else {
        const std::vector<float> ones(K, 1.0f);
        HIPCHK(c, hipMemcpy(c->tr_cs, ones.data(), K * sizeof(float), hipMemcpyHostToDevice));
    }
    if (embed_avg) HIPCHK(c, hipMemcpy(c->tr_avg, embed_avg, K * 64 * sizeof(float), hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemcpy(c->tr_avg, c->w["cb"], K * 64 * sizeof(float), hipMemcpyDeviceToDevice));
    c->training = true;
    c->chunk_fitted = false;   // the next call fits the chunk to workspace + training workspace
    return VQHIP_OK;
}

int vqhip_vec3_train_vq_stats_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, float* stats_dev, uint16_t* indices_dev,
                                     float* latent_dev, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = v3t_check_batch(c, "vec3 train_vq_stats", leaves_dev, n, stats_dev)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(stats_dev, 0, (size_t)vqhip_vec3_train_stats_floats(c) * sizeof(float), s));
        return VQHIP_OK;
    }
    V3TWs T;
    return v3t_forward(c, leaves_dev, n, stats_dev, indices_dev, latent_dev, s, T, nullptr);
}

int vqhip_vec3_train_eval_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, float* stats_dev, float* recon_sums_dev,
                                 float* recon_dev, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = v3t_check_batch(c, "vec3 train_eval", leaves_dev, n, stats_dev)) return rc;
    if (!recon_sums_dev) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 train_eval: recon_sums_dev is NULL");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(stats_dev, 0, (size_t)vqhip_vec3_train_stats_floats(c) * sizeof(float), s));
        HIPCHK(c, hipMemsetAsync(recon_sums_dev, 0, 3 * sizeof(float), s));
        return VQHIP_OK;
    }
    V3TWs T;
    uint16_t* idx = nullptr;
    if (int rc = v3t_forward(c, leaves_dev, n, stats_dev, nullptr, nullptr, s, T, &idx)) return rc;
    const V3Ws W = v3_ws(c);
    hipLaunchKernelGGL(v3t::straight_k, dim3(v3_ew_grid(n * 4096)), dim3(256), 0, s, W.z, idx, c->w["cb"], n);
    // the recon goes to the caller's buffer or to the second half of R8, which the decoder leaves alone from the stem on
    float* out = recon_dev ? recon_dev : W.b8;
    if (int rc = v3_decode_from_z(c, n, out, s)) return rc;
    hipLaunchKernelGGL(recon_loss_partials_k, dim3(RL_BLOCKS), dim3(256), 0, s, leaves_dev, out, n * 1536, T.rl);
    hipLaunchKernelGGL(recon_loss_reduce_k, dim3(1), dim3(1), 0, s, T.rl, n * 1536, recon_sums_dev);
    return v3_launch_check(c, "vec3 reconstruction loss");
}

int vqhip_vec3_train_vq_update_device(vqhip_vec3_codec* c, const float* stats_dev, float decay, float eps, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3t_require(c, "vec3 train_vq_update")) return rc;
    if (!stats_dev) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 train_vq_update: stats_dev is NULL");
    if (!(decay >= 0.0f && decay <= 1.0f)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 train_vq_update: decay must be in [0, 1]");
    if (!(eps > 0.0f)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 train_vq_update: eps must be > 0");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const float alpha = (float)(1.0 - (double)decay);
    hipLaunchKernelGGL(v3t::ema_update_k, dim3((c->k_codes + 3) / 4), dim3(256), 0, s, stats_dev, c->k_codes, decay, alpha, eps, c->tr_cs, c->tr_avg,
                       c->w["cb"]);
    if (int rc = v3_launch_check(c, "vec3 EMA update")) return rc;
    return v3t_rebuild_tables(c, s);
}

int vqhip_vec3_train_get_state(vqhip_vec3_codec* c, float* embedding, float* cluster_size, float* embed_avg)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3t_require(c, "vec3 train_get_state")) return rc;
    const size_t K = (size_t)c->k_codes;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (embedding) HIPCHK(c, hipMemcpy(embedding, c->w["cb"], K * 64 * sizeof(float), hipMemcpyDeviceToHost));
    if (cluster_size) HIPCHK(c, hipMemcpy(cluster_size, c->tr_cs, K * sizeof(float), hipMemcpyDeviceToHost));
    if (embed_avg) HIPCHK(c, hipMemcpy(embed_avg, c->tr_avg, K * 64 * sizeof(float), hipMemcpyDeviceToHost));
    return VQHIP_OK;
}

int vqhip_vec3_train_set_state(vqhip_vec3_codec* c, const float* embedding, const float* cluster_size, const float* embed_avg)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3t_require(c, "vec3 train_set_state")) return rc;
    const size_t K = (size_t)c->k_codes;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (cluster_size) HIPCHK(c, hipMemcpy(c->tr_cs, cluster_size, K * sizeof(float), hipMemcpyHostToDevice));
    if (embed_avg) HIPCHK(c, hipMemcpy(c->tr_avg, embed_avg, K * 64 * sizeof(float), hipMemcpyHostToDevice));
    if (embedding) {
        HIPCHK(c, hipMemcpy(c->w["cb"], embedding, K * 64 * sizeof(float), hipMemcpyHostToDevice));
        if (int rc = v3t_rebuild_tables(c, c->stream)) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VQHIP_OK;
}

}  // extern "C"
