// vq_vec3_mask.inc — runtime of the Vec3 handle's active-voxel masks (vqhip_vec3_mask_leaf_err_device, _residual_encode_device,
// _sweep_device, _compress_residual, _sweep; include/vqvdb_hip_vec3_mask.h, DESIGN.md §21).  Part of vq_runtime.hip's translation
// unit, after vq_vec3_rate.inc: the round trip of the handle's precision mode, the scan, the chunk tail and the ladder checks are the
// other files', unchanged; leaf_err_masked_k of vq_mask.h measures a chunk as a pass of its own behind the round trip and the
// MASKED instantiations of vq_residual.h and vq_rate.h (C = 3) class, pack and sweep it.

#include "../../include/vqvdb_hip_vec3_mask.h"
#include "vq_mask.h"

static_assert(VQHIP_VEC3_MASK_WORDS == 8, "a leaf of 512 voxels has eight mask words");

namespace {

inline const unsigned long long* mk_words(const uint64_t* p) { return reinterpret_cast<const unsigned long long*>(p); }   // the kernels' word

int v3m_leaf_err(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, int64_t m, float* d_err, hipStream_t s)
{
    hipLaunchKernelGGL(vqm::leaf_err_masked_k, dim3((unsigned)m), dim3(512), 0, s, d_leaves, d_recon, mk_words(d_mask), d_err, m);
    return v3_launch_check(c, "vec3 mask_leaf_err");
}

int v3m_encode(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err, int64_t n, float tol,
               uint16_t* d_code, int64_t* d_off, uint8_t* d_payload, int64_t capacity, hipStream_t s)
{
    hipLaunchKernelGGL((vqr::resid_class_k<3, true>), dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, d_err, n, tol, d_code, d_off,
                       mk_words(d_mask));
    hipLaunchKernelGGL(vqr::resid_scan_k, dim3(1), dim3(1024), 0, s, d_off, n);
    hipLaunchKernelGGL((vqr::resid_pack_k<3, true>), dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, n, tol, d_code, d_off,
                       d_payload, capacity, mk_words(d_mask));
    return v3_launch_check(c, "vec3 mask_residual_encode");
}

int v3m_sweep(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err, int64_t n,
              const vqrate::Tols& T, int64_t* d_hist, hipStream_t s)
{
    const unsigned grid = (unsigned)std::min<int64_t>((n + vqrate::RATE_WAVES - 1) / vqrate::RATE_WAVES, vqrate::RATE_MAX_GRID);
    hipLaunchKernelGGL((vqrate::sweep_k<3, true>), dim3(grid), dim3(64 * vqrate::RATE_WAVES), 0, s, d_leaves, d_recon, d_err, n, T,
                       reinterpret_cast<unsigned long long*>(d_hist), mk_words(d_mask));
    return v3_launch_check(c, "vec3 mask_sweep");
}

// host calls: one chunk's masks beside the buffers of v3r_ensure_host
int v3m_ensure_host(vqhip_vec3_codec* c, int64_t m)
{
    if (int rc = v3r_ensure_host(c, m)) return rc;
    return ensure(c, c->mk_mask, (size_t)m * 8, [&](hipError_t) { return "vec3 mask: cannot allocate the masks of " + std::to_string(m) + " leaves"; });
}

// one chunk of the host calls, leaves and masks from the caller's arrays: the round trip with a stored reconstruction, then the
// masked error over it in c->rs_err
int v3m_roundtrip_host(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t o, int64_t m)
{
    if (int rc = v3_ensure_io(c, m)) return rc;
    if (int rc = v3m_ensure_host(c, m)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->io_leaves, leaves + o * 1536, (size_t)m * 1536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->mk_mask, masks + o * 8, (size_t)m * 64, hipMemcpyHostToDevice, c->stream));
    if (int rc = v3e_roundtrip_chunk(c, c->io_leaves, m, c->io_idx, c->rs_recon, c->rs_err, c->stream)) return rc;
    return v3m_leaf_err(c, c->io_leaves, c->rs_recon, c->mk_mask, m, c->rs_err, c->stream);
}

}  // namespace

extern "C" {

int vqhip_vec3_mask_leaf_err_device(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, int64_t n, float* d_err,
                                    void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_leaf_err: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_recon || !d_mask || !d_err) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_leaf_err: null pointer");
    if (n > 0x7FFFFFFFll) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_leaf_err: n_leaves exceeds 2^31 - 1");
    HIPCHK(c, hipSetDevice(c->device));
    return v3m_leaf_err(c, d_leaves, d_recon, d_mask, n, d_err, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_mask_residual_encode_device(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err,
                                           int64_t n, float tol, uint16_t* d_code, int64_t* d_off, uint8_t* d_payload, int64_t capacity, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_residual_encode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (capacity < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_residual_encode: payload_capacity < 0");
    if (!d_leaves || !d_recon || !d_mask || !d_err || !d_code || !d_off || (!d_payload && capacity > 0))
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_residual_encode: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_residual_encode: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3m_encode(c, d_leaves, d_recon, d_mask, d_err, n, tol, d_code, d_off, d_payload, capacity, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_mask_sweep_device(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const uint64_t* d_mask, const float* d_err, int64_t n,
                                 const float* tols, int n_tols, int64_t* d_hist, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_sweep: n_leaves < 0");
    if (int rc = rate_check_count(c, "vec3 mask_sweep", n_tols)) return rc;
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_recon || !d_mask || !d_err || !tols || !d_hist) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_sweep: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_sweep: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3m_sweep(c, d_leaves, d_recon, d_mask, d_err, n, rate_tols(tols, n_tols), d_hist, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_mask_compress_residual(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t n, float tol, uint16_t* indices,
                                      float* leaf_err, uint16_t* leaf_code, uint8_t* payload, int64_t* payload_bytes)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_compress_residual: n_leaves < 0");
    if (!payload_bytes) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_compress_residual: payload_bytes is NULL");
    *payload_bytes = 0;
    if (n == 0) return VQHIP_OK;
    if (!leaves || !masks || !indices || !leaf_code || !payload) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_compress_residual: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        int rc = v3m_roundtrip_host(c, leaves, masks, o, m);
        if (!rc) rc = v3m_encode(c, c->io_leaves, c->rs_recon, c->mk_mask, c->rs_err, m, tol, c->rs_code, c->rs_off, c->rs_payload, m * 6144, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copies above may still read the caller's arrays
            return rc;
        }
        HIPCHK(c, hipMemcpyAsync(indices + o * 64, c->io_idx, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
        if (leaf_err)
            HIPCHK(c, hipMemcpyAsync(leaf_err + o * VQHIP_VEC3_ERR_FLOATS, c->rs_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS * sizeof(float),
                                     hipMemcpyDeviceToHost, c->stream));
        if ((rc = v3r_fetch_chunk(c, "vec3 mask_compress_residual", o, m, leaf_code, payload, &total))) return rc;
    }
    *payload_bytes = total;
    return VQHIP_OK;
}

int vqhip_vec3_mask_sweep(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t n, const float* tols, int n_tols, int64_t* hist)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_sweep: n_leaves < 0");
    if (int rc = rate_check_tols(c, "vec3 mask_sweep", tols, n_tols)) return rc;
    if (!hist) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_sweep: hist is NULL");
    std::memset(hist, 0, (size_t)n_tols * V3RATE_ROW_BYTES);
    if (n == 0) return VQHIP_OK;
    if (!leaves || !masks) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 mask_sweep: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = v3rate_begin(c)) return rc;
    const vqrate::Tols T = rate_tols(tols, n_tols);
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        int rc = v3m_roundtrip_host(c, leaves, masks, o, m);
        if (!rc) rc = v3m_sweep(c, c->io_leaves, c->rs_recon, c->mk_mask, c->rs_err, m, T, c->rate_hist, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copies above may still read the caller's arrays
            return rc;
        }
    }
    return v3rate_end(c, n_tols, hist);
}

}  // extern "C"
