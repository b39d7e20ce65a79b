// vq_vec3_bounded.inc — runtime of the Vec3 handle's error-bounded round trip (vqhip_vec3_roundtrip_device,
// _select_outliers_device, _compress_bounded; include/vqvdb_hip_vec3_bounded.h, DESIGN.md §15).  Part of vq_runtime.hip's
// translation unit, after vq_vec3_bf16.inc: it drives the encode chunk and the decoder body of the handle's precision mode
// unchanged and ends the decoder with final_err_k instead of final_k.

#include "vq_vec3_bounded.h"
#include "../../include/vqvdb_hip_vec3_bounded.h"

namespace {

// one chunk: encoder + search, gather + decoder up to up_conv, tail with the leaf errors.  idx NULL: the indices go to the
// second half of R8, which nothing touches between the encoder's ResidualBlock(64) and the next encode.  The tail reads W.u
// (first half of R8) and the caller's leaves and writes only out (when given) and err: no workspace region of its own.
int v3e_roundtrip_chunk(vqhip_vec3_codec* c, const float* leaves, int64_t m, uint16_t* idx, float* out, float* err, hipStream_t s)
{
    if (int rc = v3_ensure_ws(c, m)) return rc;
    if (!idx) idx = reinterpret_cast<uint16_t*>(v3_ws(c).b8);
    if (int rc = v3_encode_mode(c, leaves, m, idx, s)) return rc;
    if (c->precision) {
        if (int rc = v3b_decode_body(c, idx, m, s)) return rc;
    } else {
        hipLaunchKernelGGL(v3::gather_k, dim3(v3_ew_grid(m * 4096)), dim3(256), 0, s, idx, c->w["cb"], c->k_codes, v3_ws(c).z, m);
        if (int rc = v3_decode_body(c, m, s)) return rc;
    }
    hipLaunchKernelGGL(v3e::final_err_k, dim3((unsigned)m), dim3(512), V3_LDS_FINAL, s, v3_ws(c).u, c->w["d.final.w"], c->w["d.final.b"], leaves,
                       out, err, m);
    return v3_launch_check(c, "vec3 decoder.final with leaf errors");
}

int v3e_ensure_scan(vqhip_vec3_codec* c, int64_t nb)
{
    nb = std::max<int64_t>(nb, V3_MAX_CHUNK / v3e::SEL_BLOCK);
    return ensure(c, c->bd_scan, (size_t)nb, [&](hipError_t) { return "vec3 select_outliers: cannot allocate the scan buffer of " + std::to_string(nb) + " blocks"; });
}

int v3e_select(vqhip_vec3_codec* c, const float* err, int64_t n, float tol, int64_t* ids, int64_t* count, hipStream_t s)
{
    const int64_t nb = (n + v3e::SEL_BLOCK - 1) / v3e::SEL_BLOCK;
    if (int rc = v3e_ensure_scan(c, nb)) return rc;
    hipLaunchKernelGGL(v3e::select_k<false>, dim3((unsigned)nb), dim3(v3e::SEL_BLOCK), 0, s, err, n, tol, c->bd_scan, ids);
    hipLaunchKernelGGL(v3e::select_scan_k, dim3(1), dim3(1024), 0, s, c->bd_scan, nb, count);
    hipLaunchKernelGGL(v3e::select_k<true>, dim3((unsigned)nb), dim3(v3e::SEL_BLOCK), 0, s, err, n, tol, c->bd_scan, ids);
    return v3_launch_check(c, "vec3 select_outliers");
}

// host entry point: leaf errors, outlier ids and their count of one chunk (ids [m] and the count behind them)
int v3e_ensure_host(vqhip_vec3_codec* c, int64_t m)
{
    auto nomem = [&](hipError_t) { return "vec3 compress_bounded: cannot allocate the error buffers of " + std::to_string(m) + " leaves"; };
    if (int rc = ensure(c, c->bd_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS, nomem)) return rc;
    return ensure(c, c->bd_ids, (size_t)m + 1, nomem);
}

}  // namespace

extern "C" {

int vqhip_vec3_roundtrip_device(vqhip_vec3_codec* c, const float* d_leaves, int64_t n, uint16_t* d_idx, float* d_recon, float* d_err, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 roundtrip: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_err) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 roundtrip: null pointer (leaves_dev and leaf_err_dev are required)");
    if (int rc = v3_prepare(c)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    for (int64_t o = 0; o < n; o += c->chunk)
        if (int rc = v3e_roundtrip_chunk(c, d_leaves + o * 1536, std::min(c->chunk, n - o), d_idx ? d_idx + o * 64 : nullptr,
                                         d_recon ? d_recon + o * 1536 : nullptr, d_err + o * VQHIP_VEC3_ERR_FLOATS, s))
            return rc;
    return VQHIP_OK;
}

int vqhip_vec3_select_outliers_device(vqhip_vec3_codec* c, const float* d_err, int64_t n, float tol, int64_t* d_ids, int64_t* d_count, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 select_outliers: n_leaves < 0");
    if (!d_count) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 select_outliers: count_dev is NULL");
    if (n > 0 && (!d_err || !d_ids)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 select_outliers: null pointer");
    if (n > (int64_t(1) << 31) * v3e::SEL_BLOCK / 2)
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 select_outliers: n_leaves exceeds 2^40");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
        return VQHIP_OK;
    }
    return v3e_select(c, d_err, n, tol, d_ids, d_count, s);
}

int vqhip_vec3_compress_bounded(vqhip_vec3_codec* c, const float* leaves, int64_t n, float tol, uint16_t* indices, float* leaf_err,
                                int64_t* outlier_ids, int64_t* n_outliers)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 compress_bounded: n_leaves < 0");
    if (!n_outliers) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 compress_bounded: n_outliers is NULL");
    *n_outliers = 0;
    if (n == 0) return VQHIP_OK;
    if (!leaves || !indices || !outlier_ids) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 compress_bounded: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3_ensure_io(c, m)) return rc;
        if (int rc = v3e_ensure_host(c, m)) return rc;
        int64_t* d_count = c->bd_ids + m;
        HIPCHK(c, hipMemcpyAsync(c->io_leaves, leaves + o * 1536, (size_t)m * 1536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (int rc = v3e_roundtrip_chunk(c, c->io_leaves, m, c->io_idx, nullptr, c->bd_err, c->stream)) return rc;
        if (int rc = v3e_select(c, c->bd_err, m, tol, c->bd_ids, d_count, c->stream)) return rc;
        HIPCHK(c, hipMemcpyAsync(indices + o * 64, c->io_idx, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
        if (leaf_err)
            HIPCHK(c, hipMemcpyAsync(leaf_err + o * VQHIP_VEC3_ERR_FLOATS, c->bd_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS * sizeof(float),
                                     hipMemcpyDeviceToHost, c->stream));
        int64_t count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (count < 0 || count > m) return v3_fail(c, VQHIP_ERR_DEVICE, "vec3 compress_bounded: selection count out of range");
        if (count > 0) {
            HIPCHK(c, hipMemcpy(outlier_ids + total, c->bd_ids, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < count; ++i) outlier_ids[total + i] += o;
            total += count;
        }
    }
    *n_outliers = total;
    return VQHIP_OK;
}

}  // extern "C"
