// vq_vec3_residual.inc — runtime of the Vec3 handle's quantised residuals (vqhip_vec3_residual_encode_device, _apply_device,
// vqhip_vec3_residual_compress, _residual_decompress; include/vqvdb_hip_vec3_residual.h, DESIGN.md §18).  Part of
// vq_runtime.hip's translation unit, after vq_residual.inc: the round trip and its leaf errors are vq_vec3_bounded.inc's,
// unchanged; the four kernels of vq_residual.h (C = 3) follow them.

#include "../../include/vqvdb_hip_vec3_residual.h"
#include "vq_residual.h"

static_assert(VQHIP_VEC3_RES_KEPT == vqr::Format<3>::KEPT && VQHIP_VEC3_RES_RAW == vqr::Format<3>::RAW, "the header's codes are the kernels'");

namespace {

// class, scan, pack of n leaves: d_off[n] ends as the payload's size
int v3r_encode(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, float tol, uint16_t* d_code,
               int64_t* d_off, uint8_t* d_payload, int64_t capacity, hipStream_t s)
{
    hipLaunchKernelGGL(vqr::resid_class_k<3>, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, d_err, n, tol, d_code, d_off);
    hipLaunchKernelGGL(vqr::resid_scan_k, dim3(1), dim3(1024), 0, s, d_off, n);
    hipLaunchKernelGGL(vqr::resid_pack_k<3>, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, n, tol, d_code, d_off, d_payload, capacity);
    return v3_launch_check(c, "vec3 residual_encode");
}

int v3r_apply(vqhip_vec3_codec* c, float* d_leaves, int64_t n, float tol, const uint16_t* d_code, const int64_t* d_off, const uint8_t* d_payload,
              hipStream_t s)
{
    hipLaunchKernelGGL(vqr::resid_apply_k<3>, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, n, tol, d_code, d_off, d_payload);
    return v3_launch_check(c, "vec3 residual_apply");
}

// host pair: reconstruction, leaf errors, codes, offsets and payload of one chunk
int v3r_ensure_host(vqhip_vec3_codec* c, int64_t m)
{
    auto nomem = [&](hipError_t) { return "vec3 residual: cannot allocate the record buffers of " + std::to_string(m) + " leaves"; };
    if (int rc = ensure(c, c->rs_recon, (size_t)m * 1536, nomem)) return rc;
    if (int rc = ensure(c, c->rs_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS, nomem)) return rc;
    if (int rc = ensure(c, c->rs_code, (size_t)m, nomem)) return rc;
    if (int rc = ensure(c, c->rs_off, (size_t)m + 1, nomem)) return rc;
    return ensure(c, c->rs_payload, (size_t)m * 6144, nomem);
}

// the tail of a chunk that v3r_encode has classed and packed: its codes, then its payload (once the size is known) go to the
// caller's arrays and *total grows by the payload's bytes
int v3r_fetch_chunk(vqhip_vec3_codec* c, const char* what, int64_t o, int64_t m, uint16_t* leaf_code, uint8_t* payload, int64_t* total)
{
    HIPCHK(c, hipMemcpyAsync(leaf_code + o, c->rs_code, (size_t)m * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    int64_t bytes = 0;
    HIPCHK(c, hipMemcpyAsync(&bytes, c->rs_off + m, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bytes < 0 || bytes > m * 6144) return v3_fail(c, VQHIP_ERR_DEVICE, std::string(what) + ": payload size out of range");
    if (bytes > 0) HIPCHK(c, hipMemcpy(payload + *total, c->rs_payload, (size_t)bytes, hipMemcpyDeviceToHost));
    *total += bytes;
    return VQHIP_OK;
}

}  // namespace

extern "C" {

int vqhip_vec3_residual_encode_device(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, float tol,
                                      uint16_t* d_code, int64_t* d_off, uint8_t* d_payload, int64_t capacity, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 residual_encode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (capacity < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 residual_encode: payload_capacity < 0");
    if (!d_leaves || !d_recon || !d_err || !d_code || !d_off || (!d_payload && capacity > 0))
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 residual_encode: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 residual_encode: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3r_encode(c, d_leaves, d_recon, d_err, n, tol, d_code, d_off, d_payload, capacity, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_residual_apply_device(vqhip_vec3_codec* c, float* d_leaves, int64_t n, float tol, const uint16_t* d_code, const int64_t* d_off,
                                     const uint8_t* d_payload, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 residual_apply: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_code || !d_off) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 residual_apply: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 residual_apply: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3r_apply(c, d_leaves, n, tol, d_code, d_off, d_payload, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_residual_compress(vqhip_vec3_codec* c, const float* leaves, int64_t n, float tol, uint16_t* indices, float* leaf_err,
                                 uint16_t* leaf_code, uint8_t* payload, int64_t* payload_bytes)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 compress_residual: n_leaves < 0");
    if (!payload_bytes) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 compress_residual: payload_bytes is NULL");
    *payload_bytes = 0;
    if (n == 0) return VQHIP_OK;
    if (!leaves || !indices || !leaf_code || !payload) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 compress_residual: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3_ensure_io(c, m)) return rc;
        if (int rc = v3r_ensure_host(c, m)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->io_leaves, leaves + o * 1536, (size_t)m * 1536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        int rc = v3e_roundtrip_chunk(c, c->io_leaves, m, c->io_idx, c->rs_recon, c->rs_err, c->stream);
        if (!rc) rc = v3r_encode(c, c->io_leaves, c->rs_recon, c->rs_err, m, tol, c->rs_code, c->rs_off, c->rs_payload, m * 6144, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copy above may still read the caller's leaves
            return rc;
        }
        HIPCHK(c, hipMemcpyAsync(indices + o * 64, c->io_idx, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
        if (leaf_err)
            HIPCHK(c, hipMemcpyAsync(leaf_err + o * VQHIP_VEC3_ERR_FLOATS, c->rs_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS * sizeof(float),
                                     hipMemcpyDeviceToHost, c->stream));
        if ((rc = v3r_fetch_chunk(c, "vec3 compress_residual", o, m, leaf_code, payload, &total))) return rc;
    }
    *payload_bytes = total;
    return VQHIP_OK;
}

int vqhip_vec3_residual_decompress(vqhip_vec3_codec* c, const uint16_t* indices, int64_t n, float tol, const uint16_t* leaf_code,
                                   const uint8_t* payload, int64_t payload_bytes, float* leaves)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0 || payload_bytes < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_residual: n_leaves < 0 or payload_bytes < 0");
    if (n == 0) return VQHIP_OK;
    if (!indices || !leaves || !leaf_code || (payload_bytes > 0 && !payload))
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_residual: null pointer");
    int64_t need = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!vqr::code_ok<3>(leaf_code[i])) {
            char hex[8];
            std::snprintf(hex, sizeof hex, "0x%04X", (unsigned)leaf_code[i]);
            return v3_fail(c, VQHIP_ERR_INVALID, std::string("vec3 decompress_residual: code ") + hex + " of leaf " + std::to_string(i) +
                                                     " is neither 0xFFFE, 0xFFFF nor three widths of 0..16");
        }
        need += vqr::record_size<3>(leaf_code[i]);
    }
    if (need != payload_bytes)
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_residual: the codes need " + std::to_string(need) + " payload bytes, the caller gives " +
                                                 std::to_string(payload_bytes));
    if (int rc = v3_prepare(c)) return rc;
    std::vector<int64_t> off;
    int64_t at = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3_ensure_io(c, m)) return rc;
        if (int rc = v3r_ensure_host(c, m)) return rc;
        off.resize((size_t)m + 1);
        off[0] = 0;
        for (int64_t i = 0; i < m; ++i) off[i + 1] = off[i] + vqr::record_size<3>(leaf_code[o + i]);
        HIPCHK(c, hipMemcpy(c->io_idx, indices + o * 64, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->rs_code, leaf_code + o, (size_t)m * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->rs_off, off.data(), (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        if (off[m] > 0) HIPCHK(c, hipMemcpy(c->rs_payload, payload + at, (size_t)off[m], hipMemcpyHostToDevice));
        at += off[m];
        if (int rc = v3_decode_mode(c, c->io_idx, m, c->io_leaves, c->stream)) return rc;
        if (int rc = v3r_apply(c, c->io_leaves, m, tol, c->rs_code, c->rs_off, c->rs_payload, c->stream)) return rc;
        HIPCHK(c, hipMemcpyAsync(leaves + o * 1536, c->io_leaves, (size_t)m * 1536 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VQHIP_OK;
}

}  // extern "C"
