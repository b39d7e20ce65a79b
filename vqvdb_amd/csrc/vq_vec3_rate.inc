// vq_vec3_rate.inc — runtime of the Vec3 handle's size sweep (vqhip_vec3_rate_payload_bytes, _sweep_device, _sweep, _compress,
// _pick; include/vqvdb_hip_vec3_rate.h, DESIGN.md §20).  Part of vq_runtime.hip's translation unit, after vq_vec3_residual.inc
// and vq_rate.inc: the round trip is vq_vec3_bounded.inc's, the encode of the records and the chunk tail vq_vec3_residual.inc's,
// the ladder checks, rate_payload and rate_pick vq_rate.inc's; sweep_k<3> of vq_rate.h follows the round trip of every chunk and
// adds to one histogram that stays on the device until the call's end.

#include "../../include/vqvdb_hip_vec3_rate.h"
#include "vq_rate.h"

static_assert(VQHIP_VEC3_RATE_MAX_TOLS == vqrate::RATE_MAX_TOLS && VQHIP_VEC3_RATE_CLASSES == vqrate::CLASSES<3>, "the header's table is the kernel's");

namespace {

constexpr size_t V3RATE_ROW_BYTES = (size_t)VQHIP_VEC3_RATE_CLASSES * sizeof(int64_t);
constexpr size_t V3RATE_HIST_BYTES = (size_t)VQHIP_VEC3_RATE_MAX_TOLS * V3RATE_ROW_BYTES;

// the histogram of n leaves added to d_hist
int v3rate_sweep(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, const vqrate::Tols& T, int64_t* d_hist,
                 hipStream_t s)
{
    const unsigned grid = (unsigned)std::min<int64_t>((n + vqrate::RATE_WAVES - 1) / vqrate::RATE_WAVES, vqrate::RATE_MAX_GRID);
    hipLaunchKernelGGL(vqrate::sweep_k<3>, dim3(grid), dim3(64 * vqrate::RATE_WAVES), 0, s, d_leaves, d_recon, d_err, n, T,
                       reinterpret_cast<unsigned long long*>(d_hist));
    return v3_launch_check(c, "vec3 rate_sweep");
}

// the handle's histogram, cleared on its stream
int v3rate_begin(vqhip_vec3_codec* c)
{
    if (int rc = ensure(c, c->rate_hist, V3RATE_HIST_BYTES / sizeof(int64_t), "the size-sweep histogram")) return rc;
    HIPCHK(c, hipMemsetAsync(c->rate_hist, 0, V3RATE_HIST_BYTES, c->stream));
    return VQHIP_OK;
}

// ... and read back behind everything the stream holds
int v3rate_end(vqhip_vec3_codec* c, int n_tols, int64_t* hist)
{
    HIPCHK(c, hipMemcpyAsync(hist, c->rate_hist, (size_t)n_tols * V3RATE_ROW_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

// pass 1 of both host calls: per chunk the round trip with a stored reconstruction, then the sweep; indices and leaf_err (both
// or neither) receive every chunk's indices and errors.  hist [n_tols][51] is overwritten.  n > 0.
int v3rate_sweep_host(vqhip_vec3_codec* c, const float* leaves, int64_t n, const float* tols, int n_tols, int64_t* hist, uint16_t* indices,
                      float* leaf_err)
{
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = v3rate_begin(c)) return rc;
    const vqrate::Tols T = rate_tols(tols, n_tols);
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3_ensure_io(c, m)) return rc;
        if (int rc = v3r_ensure_host(c, m)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->io_leaves, leaves + o * 1536, (size_t)m * 1536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        int rc = v3e_roundtrip_chunk(c, c->io_leaves, m, c->io_idx, c->rs_recon, c->rs_err, c->stream);
        if (!rc) rc = v3rate_sweep(c, c->io_leaves, c->rs_recon, c->rs_err, m, T, c->rate_hist, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copy above may still read the caller's leaves
            return rc;
        }
        if (indices) {
            HIPCHK(c, hipMemcpyAsync(indices + o * 64, c->io_idx, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(leaf_err + o * VQHIP_VEC3_ERR_FLOATS, c->rs_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS * sizeof(float),
                                     hipMemcpyDeviceToHost, c->stream));
        }
    }
    return v3rate_end(c, n_tols, hist);
}

}  // namespace

extern "C" {

int64_t vqhip_vec3_rate_payload_bytes(const int64_t* hist_row)
{
    return hist_row ? rate_payload<3>(hist_row) : -1;
}

int vqhip_vec3_rate_pick(const int64_t* hist, const float* tols, int n_tols, int64_t payload_budget)
{
    if (!hist || !tols || n_tols < 1 || n_tols > VQHIP_VEC3_RATE_MAX_TOLS || payload_budget < 0) return -1;
    return rate_pick<3>(hist, tols, n_tols, payload_budget, rate_payload<3>, nullptr);
}

int vqhip_vec3_rate_sweep_device(vqhip_vec3_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, const float* tols,
                                 int n_tols, int64_t* d_hist, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_sweep: n_leaves < 0");
    if (int rc = rate_check_count(c, "vec3 rate_sweep", n_tols)) return rc;
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_recon || !d_err || !tols || !d_hist) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_sweep: null pointer");
    if (n > (int64_t(1) << 32)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_sweep: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return v3rate_sweep(c, d_leaves, d_recon, d_err, n, rate_tols(tols, n_tols), d_hist, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_vec3_rate_sweep(vqhip_vec3_codec* c, const float* leaves, int64_t n, const float* tols, int n_tols, int64_t* hist)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_sweep: n_leaves < 0");
    if (int rc = rate_check_tols(c, "vec3 rate_sweep", tols, n_tols)) return rc;
    if (!hist) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_sweep: hist is NULL");
    std::memset(hist, 0, (size_t)n_tols * V3RATE_ROW_BYTES);
    if (n == 0) return VQHIP_OK;
    if (!leaves) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_sweep: null pointer");
    return v3rate_sweep_host(c, leaves, n, tols, n_tols, hist, nullptr, nullptr);
}

int vqhip_vec3_rate_compress(vqhip_vec3_codec* c, const float* leaves, int64_t n, const float* tols, int n_tols, int64_t payload_budget, float* tol_used,
                             int64_t* hist, uint16_t* indices, float* leaf_err, uint16_t* leaf_code, uint8_t* payload, int64_t* payload_bytes)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_compress: n_leaves < 0");
    if (!tol_used || !payload_bytes) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_compress: tol_used or payload_bytes is NULL");
    *payload_bytes = 0;
    if (payload_budget < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_compress: payload_budget < 0");
    if (int rc = rate_check_tols(c, "vec3 rate_compress", tols, n_tols)) return rc;
    int64_t table[VQHIP_VEC3_RATE_MAX_TOLS * VQHIP_VEC3_RATE_CLASSES];
    std::memset(table, 0, (size_t)n_tols * V3RATE_ROW_BYTES);
    if (n == 0) {   // every rung needs 0 bytes: the smallest that is not NaN, if there is one
        if (hist) std::memcpy(hist, table, (size_t)n_tols * V3RATE_ROW_BYTES);
        const int best = rate_pick<3>(table, tols, n_tols, payload_budget, rate_payload<3>, nullptr);
        if (best >= 0) *tol_used = tols[best];
        return VQHIP_OK;
    }
    if (!leaves || !indices || !leaf_code || !payload) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_compress: null pointer");
    std::unique_ptr<float[]> own;
    if (!leaf_err) {
        own.reset(new (std::nothrow) float[(size_t)n * VQHIP_VEC3_ERR_FLOATS]);
        if (!own) return v3_fail(c, VQHIP_ERR_NOMEM, "vec3 rate_compress: cannot allocate the leaf errors of " + std::to_string(n) + " leaves");
        leaf_err = own.get();
    }
    if (int rc = v3rate_sweep_host(c, leaves, n, tols, n_tols, table, indices, leaf_err)) return rc;
    if (hist) std::memcpy(hist, table, (size_t)n_tols * V3RATE_ROW_BYTES);
    int64_t smallest = -1;
    const int best = rate_pick<3>(table, tols, n_tols, payload_budget, rate_payload<3>, &smallest);
    if (best < 0) {
        if (smallest < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_compress: every rung is NaN, none can be chosen");
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 rate_compress: the smallest payload of the " + std::to_string(n_tols) + " rungs has " +
                                                 std::to_string(smallest) + " bytes, the budget is " + std::to_string(payload_budget) + " bytes");
    }
    const float tol = tols[best];
    *tol_used = tol;
    // pass 2: the model's encoder is not run again; pass 1's indices decode to the x^ its round trip stored, to the bit
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3_ensure_io(c, m)) return rc;
        if (int rc = v3r_ensure_host(c, m)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->io_leaves, leaves + o * 1536, (size_t)m * 1536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->io_idx, indices + o * 64, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->rs_err, leaf_err + o * VQHIP_VEC3_ERR_FLOATS, (size_t)m * VQHIP_VEC3_ERR_FLOATS * sizeof(float),
                                 hipMemcpyHostToDevice, c->stream));
        int rc = v3_decode_mode(c, c->io_idx, m, c->rs_recon, c->stream);
        if (!rc) rc = v3r_encode(c, c->io_leaves, c->rs_recon, c->rs_err, m, tol, c->rs_code, c->rs_off, c->rs_payload, m * 6144, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copies above may still read the caller's arrays
            return rc;
        }
        if ((rc = v3r_fetch_chunk(c, "vec3 rate_compress", o, m, leaf_code, payload, &total))) return rc;
    }
    if (total != rate_payload<3>(table + (size_t)best * VQHIP_VEC3_RATE_CLASSES))
        return v3_fail(c, VQHIP_ERR_DEVICE, "vec3 rate_compress: the payload has " + std::to_string(total) + " bytes, the histogram predicted " +
                                                std::to_string(rate_payload<3>(table + (size_t)best * VQHIP_VEC3_RATE_CLASSES)));
    *payload_bytes = total;
    return VQHIP_OK;
}

}  // extern "C"
