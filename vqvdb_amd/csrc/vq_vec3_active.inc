// vq_vec3_active.inc — runtime of the Vec3 handle's compact residual records (vqhip_vec3_active_record_bytes, _encode_device,
// _apply_device, _sweep_device, _compress, _decompress, _sweep; include/vqvdb_hip_vec3_active.h, DESIGN.md §25).  Part of
// vq_runtime.hip's translation unit, after vq_vec3_mask.inc: the round trip of the handle's precision mode, the masked error, the
// scan, the chunk buffers, the chunk tail (v3r_fetch_chunk reads the chunk's size from offsets[m], so it serves these records as
// they are) and the ladder checks are the other files', unchanged; the kernels of vq_active.h class, pack, apply and sweep.

#include "../../include/vqvdb_hip_vec3_active.h"
#include "vq_active.h"

namespace {

int v3a_encode(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err, int64_t n, float tol,
               uint16_t* d_code, int64_t* d_off, uint8_t* d_payload, int64_t capacity, hipStream_t s)
{
    hipLaunchKernelGGL(vqa::active_class_k, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, d_err, n, tol, d_code, d_off,
                       mk_words(d_mask));
    hipLaunchKernelGGL(vqr::resid_scan_k, dim3(1), dim3(1024), 0, s, d_off, n);
    hipLaunchKernelGGL(vqa::active_pack_k, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, n, tol, d_code, d_off, d_payload,
                       capacity, mk_words(d_mask));
    return v3_launch_check(c, "vec3 active_encode");
}

// background: host pointer to three floats or NULL; they travel in the kernel's arguments
int v3a_apply(vqhip_vec3_codec* c, float* d_leaves, const uint64_t* d_mask, int64_t n, float tol, const uint16_t* d_code, const int64_t* d_off,
              const uint8_t* d_payload, const float* background, hipStream_t s)
{
    const float b0 = background ? background[0] : 0.0f, b1 = background ? background[1] : 0.0f, b2 = background ? background[2] : 0.0f;
    hipLaunchKernelGGL(vqa::active_apply_k, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, n, tol, d_code, d_off, d_payload,
                       mk_words(d_mask), background ? 1 : 0, b0, b1, b2);
    return v3_launch_check(c, "vec3 active_apply");
}

int v3a_sweep(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err, int64_t n,
              const vqrate::Tols& T, int64_t* d_bytes, hipStream_t s)
{
    const unsigned grid = (unsigned)std::min<int64_t>((n + vqrate::RATE_WAVES - 1) / vqrate::RATE_WAVES, vqrate::RATE_MAX_GRID);
    hipLaunchKernelGGL(vqa::active_sweep_k, dim3(grid), dim3(64 * vqrate::RATE_WAVES), 0, s, d_leaves, d_recon, d_err, n, T,
                       reinterpret_cast<unsigned long long*>(d_bytes), mk_words(d_mask));
    return v3_launch_check(c, "vec3 active_sweep");
}

inline int v3a_popcount(const uint64_t* words)
{
    int a = 0;
    for (int j = 0; j < 8; ++j) a += __builtin_popcountll(words[j]);
    return a;
}

// one chunk of vqhip_vec3_active_compress (m <= c->chunk, after v3_prepare), host arrays of that chunk: the round trip, the masked
// error, the compact encode; its records go to payload + *total, which grows by their bytes
int v3a_compress_chunk(vqhip_vec3_codec* c, const char* what, const float* leaves, const uint64_t* masks, int64_t m, float tol, uint16_t* indices,
                       float* leaf_err, uint16_t* leaf_code, uint8_t* payload, int64_t* total)
{
    int rc = v3m_roundtrip_host(c, leaves, masks, 0, m);
    if (!rc) rc = v3a_encode(c, c->io_leaves, c->rs_recon, c->mk_mask, c->rs_err, m, tol, c->rs_code, c->rs_off, c->rs_payload, m * 6144, c->stream);
    if (rc) {
        hipStreamSynchronize(c->stream);   // the copies above may still read the caller's arrays
        return rc;
    }
    HIPCHK(c, hipMemcpyAsync(indices, c->io_idx, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    if (leaf_err)
        HIPCHK(c, hipMemcpyAsync(leaf_err, c->rs_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return v3r_fetch_chunk(c, what, 0, m, leaf_code, payload, total);   // sized by offsets[m]
}

// one chunk of vqhip_vec3_active_decompress (m <= c->chunk, after v3_prepare), host arrays of that chunk whose codes and sizes have
// been checked; payload addresses the chunk's first record and *bytes receives the bytes of its records
int v3a_decompress_chunk(vqhip_vec3_codec* c, const uint16_t* indices, const uint64_t* masks, int64_t m, float tol, const uint16_t* leaf_code,
                         const uint8_t* payload, const float* background, float* leaves, std::vector<int64_t>& off, int64_t* bytes)
{
    if (int rc = v3_ensure_io(c, m)) return rc;
    if (int rc = v3m_ensure_host(c, m)) return rc;
    off.resize((size_t)m + 1);
    off[0] = 0;
    for (int64_t i = 0; i < m; ++i) off[i + 1] = off[i] + vqa::record_bytes(leaf_code[i], v3a_popcount(masks + i * 8));
    HIPCHK(c, hipMemcpy(c->io_idx, indices, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->mk_mask, masks, (size_t)m * 64, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->rs_code, leaf_code, (size_t)m * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->rs_off, off.data(), (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (off[m] > 0) HIPCHK(c, hipMemcpy(c->rs_payload, payload, (size_t)off[m], hipMemcpyHostToDevice));
    *bytes = off[m];
    if (int rc = v3_decode_mode(c, c->io_idx, m, c->io_leaves, c->stream)) return rc;
    if (int rc = v3a_apply(c, c->io_leaves, c->mk_mask, m, tol, c->rs_code, c->rs_off, c->rs_payload, background, c->stream)) return rc;
    HIPCHK(c, hipMemcpyAsync(leaves, c->io_leaves, (size_t)m * 1536 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

}  // namespace

extern "C" {

int64_t vqhip_vec3_active_record_bytes(int code, int active)
{
    if (!vqr::code_ok<3>(code) || active < 0 || active > 512) return -1;
    return vqa::record_bytes(code, active);
}

int vqhip_vec3_active_encode_device(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err,
                                    int64_t n, float tol, uint16_t* d_code, int64_t* d_off, uint8_t* d_payload, int64_t capacity, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_encode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (capacity < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_encode: payload_capacity < 0");
    if (!d_leaves || !d_recon || !d_mask || !d_err || !d_code || !d_off || (!d_payload && capacity > 0))
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_encode: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_encode: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3a_encode(c, d_leaves, d_recon, d_mask, d_err, n, tol, d_code, d_off, d_payload, capacity, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_active_apply_device(vqhip_vec3_codec* c, float* d_leaves, const uint64_t* d_mask, int64_t n, float tol, const uint16_t* d_code,
                                   const int64_t* d_off, const uint8_t* d_payload, const float* background, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_apply: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_mask || !d_code || !d_off) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_apply: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_apply: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3a_apply(c, d_leaves, d_mask, n, tol, d_code, d_off, d_payload, background, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_active_sweep_device(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err,
                                   int64_t n, const float* tols, int n_tols, int64_t* d_bytes, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_sweep: n_leaves < 0");
    if (int rc = rate_check_count(c, "vec3 active_sweep", n_tols)) return rc;
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_recon || !d_mask || !d_err || !tols || !d_bytes) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_sweep: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_sweep: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3a_sweep(c, d_leaves, d_recon, d_mask, d_err, n, rate_tols(tols, n_tols), d_bytes, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_active_compress(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t n, float tol, uint16_t* indices,
                               float* leaf_err, uint16_t* leaf_code, uint8_t* payload, int64_t* payload_bytes)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_compress: n_leaves < 0");
    if (!payload_bytes) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_compress: payload_bytes is NULL");
    *payload_bytes = 0;
    if (n == 0) return VQHIP_OK;
    if (!leaves || !masks || !indices || !leaf_code || !payload) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_compress: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3a_compress_chunk(c, "vec3 active_compress", leaves + o * 1536, masks + o * 8, m, tol, indices + o * 64,
                                        leaf_err ? leaf_err + o * VQHIP_VEC3_ERR_FLOATS : nullptr, leaf_code + o, payload, &total))
            return rc;
    }
    *payload_bytes = total;
    return VQHIP_OK;
}

int vqhip_vec3_active_decompress(vqhip_vec3_codec* c, const uint16_t* indices, const uint64_t* masks, int64_t n, float tol, const uint16_t* leaf_code,
                                 const uint8_t* payload, int64_t payload_bytes, const float* background, float* leaves)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0 || payload_bytes < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_decompress: n_leaves < 0 or payload_bytes < 0");
    if (n == 0) return VQHIP_OK;
    if (!indices || !masks || !leaves || !leaf_code || (payload_bytes > 0 && !payload))
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_decompress: null pointer");
    int64_t need = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!vqr::code_ok<3>(leaf_code[i])) {
            char hex[8];
            std::snprintf(hex, sizeof hex, "0x%04X", (unsigned)leaf_code[i]);
            return v3_fail(c, VQHIP_ERR_INVALID, std::string("vec3 active_decompress: code ") + hex + " of leaf " + std::to_string(i) +
                                                     " is neither 0xFFFE, 0xFFFF nor three widths of 0..16");
        }
        need += vqa::record_bytes(leaf_code[i], v3a_popcount(masks + i * 8));
    }
    if (need != payload_bytes)
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_decompress: the codes and masks need " + std::to_string(need) +
                                                 " payload bytes, the caller gives " + std::to_string(payload_bytes));
    if (int rc = v3_prepare(c)) return rc;
    std::vector<int64_t> off;
    int64_t at = 0, bytes = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3a_decompress_chunk(c, indices + o * 64, masks + o * 8, m, tol, leaf_code + o, payload + at, background, leaves + o * 1536, off,
                                          &bytes))
            return rc;
        at += bytes;
    }
    return VQHIP_OK;
}

int vqhip_vec3_active_sweep(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t n, const float* tols, int n_tols, int64_t* bytes)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_sweep: n_leaves < 0");
    if (int rc = rate_check_tols(c, "vec3 active_sweep", tols, n_tols)) return rc;
    if (!bytes) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_sweep: bytes is NULL");
    std::memset(bytes, 0, (size_t)n_tols * sizeof(int64_t));
    if (n == 0) return VQHIP_OK;
    if (!leaves || !masks) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 active_sweep: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = ensure(c, c->ac_bytes, (size_t)VQHIP_VEC3_RATE_MAX_TOLS, "the compact size sums")) return rc;
    HIPCHK(c, hipMemsetAsync(c->ac_bytes, 0, (size_t)VQHIP_VEC3_RATE_MAX_TOLS * sizeof(int64_t), c->stream));
    const vqrate::Tols T = rate_tols(tols, n_tols);
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        int rc = v3m_roundtrip_host(c, leaves, masks, o, m);
        if (!rc) rc = v3a_sweep(c, c->io_leaves, c->rs_recon, c->mk_mask, c->rs_err, m, T, c->ac_bytes, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copies above may still read the caller's arrays
            return rc;
        }
    }
    HIPCHK(c, hipMemcpyAsync(bytes, c->ac_bytes, (size_t)n_tols * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

}  // extern "C"
