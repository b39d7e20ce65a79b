// vq_bounded.inc — runtime of the scalar handle's error-bounded calls (vqhip_roundtrip_device, _select_outliers_device,
// _compress_bounded, _decompress_bounded; include/vqvdb_hip_bounded.h, DESIGN.md §16).  Part of vq_runtime.hip's translation
// unit, after vq_vec3_bounded.inc: it drives encode_chunk and decode_chunk unchanged, measures the chunk with leaf_err_k and
// selects with the Vec3 handle's compaction kernels.  The file pair lives beside vqhip_compress_file / _decompress_file in
// vq_file.inc, which hangs bd_stage below behind every chunk of the host pipeline.

#include "vq_bounded.h"

namespace {

int bd_launch_check(vqhip_codec* c, const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, VQHIP_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return VQHIP_OK;
}

// the error text of a failed ensure() of `count` elements
auto bd_nomem(const char* what, int64_t count)
{
    return [=](hipError_t) { return std::string("bounded: cannot allocate ") + what + " (" + std::to_string(count) + " elements)"; };
}

// the chunk's leaf errors from the caller's leaves and its reconstruction
int bd_leaf_err(vqhip_codec* c, const float* d_leaves, const float* d_recon, int64_t m, float* d_err, hipStream_t s)
{
    const unsigned grid = (unsigned)((m + vqe::ERR_WAVES - 1) / vqe::ERR_WAVES);
    Launcher L{c, s, m};
    L.run("bounded_leaf_err", [&] { hipLaunchKernelGGL(vqe::leaf_err_k, dim3(grid), dim3(64 * vqe::ERR_WAVES), 0, s, d_leaves, d_recon, d_err, m); });
    return L.rc;
}

// one chunk: encode_chunk, decode_chunk on its indices, leaf_err_k.  idx / recon NULL: the handle's own buffers.
int bd_roundtrip_chunk(vqhip_codec* c, const float* d_leaves, int64_t m, uint8_t* d_idx, float* d_recon, float* d_err, hipStream_t s)
{
    if (!d_idx) {
        const int64_t count = std::max(m, std::min<int64_t>(c->chunk, 65536)) * 64;
        if (int rc = ensure(c, c->bd_idx, count, bd_nomem("the index chunk", count))) return rc;
        d_idx = c->bd_idx;
    }
    if (!d_recon) {
        const int64_t count = std::max(m, std::min<int64_t>(c->chunk, 65536)) * 512;
        if (int rc = ensure(c, c->bd_recon, count, bd_nomem("the reconstruction chunk", count))) return rc;
        d_recon = c->bd_recon;
    }
    if (int rc = encode_chunk(c, d_leaves, m, d_idx, s)) return rc;
    if (int rc = decode_chunk(c, d_idx, m, d_recon, s)) return rc;
    return bd_leaf_err(c, d_leaves, d_recon, m, d_err, s);
}

int bd_select(vqhip_codec* c, const float* d_err, int64_t n, float tol, int64_t* d_ids, int64_t* d_count, hipStream_t s)
{
    const int64_t nb = (n + v3e::SEL_BLOCK - 1) / v3e::SEL_BLOCK;
    if (int rc = ensure(c, c->bd_scan, std::max<int64_t>(nb, 64), bd_nomem("the selection's scan buffer", std::max<int64_t>(nb, 64)))) return rc;
    hipLaunchKernelGGL(v3e::select_k<false>, dim3((unsigned)nb), dim3(v3e::SEL_BLOCK), 0, s, d_err, n, tol, c->bd_scan, d_ids);
    hipLaunchKernelGGL(v3e::select_scan_k, dim3(1), dim3(1024), 0, s, c->bd_scan, nb, d_count);
    hipLaunchKernelGGL(v3e::select_k<true>, dim3((unsigned)nb), dim3(v3e::SEL_BLOCK), 0, s, d_err, n, tol, c->bd_scan, d_ids);
    return bd_launch_check(c, "bounded select_outliers");
}

// leaf errors of the host calls: a device buffer and a pinned landing zone per I/O slot, m leaves each
int bd_ensure_pipe(vqhip_codec* c, int64_t m)
{
    for (int i = 0; i < 2; ++i) {
        if (int rc = ensure(c, c->bd_err[i], (size_t)m * VQHIP_ERR_FLOATS, "the leaf-error slot")) return rc;
        if (int rc = ensure(c, c->bd_pin_err[i], (size_t)m * VQHIP_ERR_FLOATS, "the pinned leaf-error slot")) return rc;
    }
    return VQHIP_OK;
}

// a bounded file compress, behind the encode of every chunk: decode it and measure it on the compute stream; its leaf errors follow
// its indices to c->bd_pin_err[slot], where the pipeline's consumer reads them
PipeStage bd_stage(vqhip_codec* c)
{
    return {[c](int64_t step) { return bd_ensure_pipe(c, step); },
            [c](int64_t, int64_t m, int slot, hipStream_t s) {
                if (int rc = ensure(c, c->bd_recon, m * 512, bd_nomem("the reconstruction chunk", m * 512))) return rc;
                if (int rc = decode_chunk(c, c->dev_idx[slot], m, c->bd_recon, s)) return rc;
                return bd_leaf_err(c, c->dev_leaves[slot], c->bd_recon, m, c->bd_err[slot], s);
            },
            [c](int64_t m, int slot, hipStream_t s) {
                return hipMemcpyAsync(c->bd_pin_err[slot], c->bd_err[slot], (size_t)m * VQHIP_ERR_FLOATS * sizeof(float), hipMemcpyDeviceToHost, s);
            }};
}

int bd_prepare(vqhip_codec* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->chunk_fitted) fit_chunk_to_free_memory(c), c->chunk_fitted = true;
    return ensure_tables(c);
}

}  // namespace

extern "C" {

int vqhip_roundtrip_device(vqhip_codec* c, const float* d_leaves, int64_t n, uint8_t* d_idx, float* d_recon, float* d_err, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "roundtrip: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_err) return fail(c, VQHIP_ERR_INVALID, "roundtrip: null pointer (leaves_dev and leaf_err_dev are required)");
    if (int rc = bd_prepare(c)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    for (int64_t o = 0; o < n; o += c->chunk)
        if (int rc = bd_roundtrip_chunk(c, d_leaves + o * 512, std::min(c->chunk, n - o), d_idx ? d_idx + o * 64 : nullptr,
                                        d_recon ? d_recon + o * 512 : nullptr, d_err + o * VQHIP_ERR_FLOATS, s))
            return rc;
    return VQHIP_OK;
}

int vqhip_select_outliers_device(vqhip_codec* c, const float* d_err, int64_t n, float tol, int64_t* d_ids, int64_t* d_count, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "select_outliers: n_leaves < 0");
    if (!d_count) return fail(c, VQHIP_ERR_INVALID, "select_outliers: count_dev is NULL");
    if (n > 0 && (!d_err || !d_ids)) return fail(c, VQHIP_ERR_INVALID, "select_outliers: null pointer");
    if (n > (int64_t(1) << 31) * v3e::SEL_BLOCK / 2) return fail(c, VQHIP_ERR_INVALID, "select_outliers: n_leaves exceeds 2^40");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
        return VQHIP_OK;
    }
    return bd_select(c, d_err, n, tol, d_ids, d_count, s);
}

int vqhip_compress_bounded(vqhip_codec* c, const float* leaves, int64_t n, float tol, uint8_t* indices, float* leaf_err, int64_t* outlier_ids,
                           int64_t* n_outliers)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "compress_bounded: n_leaves < 0");
    if (!n_outliers) return fail(c, VQHIP_ERR_INVALID, "compress_bounded: n_outliers is NULL");
    *n_outliers = 0;
    if (n == 0) return VQHIP_OK;
    if (!leaves || !indices || !outlier_ids) return fail(c, VQHIP_ERR_INVALID, "compress_bounded: null pointer");
    if (int rc = bd_prepare(c)) return rc;
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = ensure_io(c, m)) return rc;
        if (int rc = bd_ensure_pipe(c, m)) return rc;
        if (int rc = ensure(c, c->bd_ids, m + 1, bd_nomem("the outlier ids", m + 1))) return rc;
        int64_t* d_count = c->bd_ids + m;
        HIPCHK(c, hipMemcpyAsync(c->dev_leaves[0], leaves + o * 512, (size_t)m * 2048, hipMemcpyHostToDevice, c->stream));
        int rc = bd_roundtrip_chunk(c, c->dev_leaves[0], m, c->dev_idx[0], nullptr, c->bd_err[0], c->stream);
        if (!rc) rc = bd_select(c, c->bd_err[0], m, tol, c->bd_ids, d_count, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copy above may still read the caller's leaves
            return rc;
        }
        HIPCHK(c, hipMemcpyAsync(indices + o * 64, c->dev_idx[0], (size_t)m * 64, hipMemcpyDeviceToHost, c->stream));
        if (leaf_err)
            HIPCHK(c, hipMemcpyAsync(leaf_err + o * VQHIP_ERR_FLOATS, c->bd_err[0], (size_t)m * VQHIP_ERR_FLOATS * sizeof(float), hipMemcpyDeviceToHost,
                                     c->stream));
        int64_t count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (count < 0 || count > m) return fail(c, VQHIP_ERR_DEVICE, "compress_bounded: selection count out of range");
        if (count > 0) {
            HIPCHK(c, hipMemcpy(outlier_ids + total, c->bd_ids, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < count; ++i) outlier_ids[total + i] += o;
            total += count;
        }
    }
    *n_outliers = total;
    return VQHIP_OK;
}

int vqhip_decompress_bounded(vqhip_codec* c, const uint8_t* indices, int64_t n, const int64_t* outlier_ids, int64_t n_outliers,
                             const float* outlier_leaves, float* leaves)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0 || n_outliers < 0) return fail(c, VQHIP_ERR_INVALID, "decompress_bounded: n_leaves < 0 or n_outliers < 0");
    if (n_outliers > n) return fail(c, VQHIP_ERR_INVALID, "decompress_bounded: more outliers than leaves");
    if (n == 0) return VQHIP_OK;
    if (!indices || !leaves || (n_outliers > 0 && (!outlier_ids || !outlier_leaves))) return fail(c, VQHIP_ERR_INVALID, "decompress_bounded: null pointer");
    for (int64_t i = 0; i < n_outliers; ++i) {
        if (outlier_ids[i] < 0 || outlier_ids[i] >= n)
            return fail(c, VQHIP_ERR_INVALID, "decompress_bounded: outlier id " + std::to_string(outlier_ids[i]) + " is not in [0, " + std::to_string(n) + ")");
        if (i > 0 && outlier_ids[i] <= outlier_ids[i - 1]) return fail(c, VQHIP_ERR_INVALID, "decompress_bounded: outlier ids are not ascending");
    }
    if (int rc = run_host_pipeline(c, false, indices, leaves, n)) return rc;
    host_parallel_for(n_outliers, [=](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) std::memcpy(leaves + outlier_ids[i] * 512, outlier_leaves + i * 512, 2048);
    });
    return VQHIP_OK;
}

}  // extern "C"
