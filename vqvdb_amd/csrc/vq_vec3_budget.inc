// vq_vec3_budget.inc — the Vec3 handle's compress into a byte budget on compact records (vqhip_vec3_budget_pick, _file_bytes,
// _compress, _file_sweep, _file_compress; include/vqvdb_hip_vec3_budget.h, DESIGN.md §27).  Part of vq_runtime.hip's translation
// unit, after vq_vec3_file.inc.  No kernel of its own and none edited: pass 1 is the sequence of vqhip_vec3_active_sweep
// (v3m_roundtrip_host, v3a_sweep), pass 2 is v3_decode_mode and v3a_encode on the selected leaves of a chunk with the chunk tail
// v3r_fetch_chunk, the writer is vq_vec3_file.inc's v3f_compress with pass 2 as its batch function, and the pick and the file size
// are vq_vec3_budget_format.h's.

#include "../../include/vqvdb_hip_vec3_budget.h"
#include "vq_vec3_budget_format.h"

static_assert(vqv3b::MAX_TOLS == VQHIP_VEC3_RATE_MAX_TOLS, "the host arithmetic takes the sweep's ladders");

namespace {

// host arrays of pass 2, kept from chunk to chunk
struct V3bScratch {
    std::vector<int64_t> sel;   // the selected leaves of the chunk, in leaf order
    std::vector<uint16_t> idx, code;
    std::vector<uint64_t> mask;
    std::vector<float> err;
};

// Pass 2 of one chunk (m <= c->chunk, after v3_prepare) from what pass 1 brought to the host: indices [m][64] and the masked errors
// err [m][2].  The leaves are `leaves` [m][512][3] or, where that is NULL, the m buffers of leaf_ptrs.  A leaf is selected exactly
// when !(err[0] <= tol), the rule of active_class_k; only those are gathered, uploaded, decoded and encoded, in leaf order, so their
// records follow one another as in the encode of the whole chunk.  leaf_code [m] receives VQHIP_VEC3_RES_KEPT for the others, the
// records go to payload + *total, which grows by their bytes.  *copy_s (may be NULL) grows by the time of the leaf gather.
int v3b_encode_selected(vqhip_vec3_codec* c, const char* what, const float* leaves, const float* const* leaf_ptrs, const uint64_t* masks,
                        const uint16_t* indices, const float* err, int64_t m, float tol, uint16_t* leaf_code, uint8_t* payload, int64_t* total,
                        V3bScratch& S, double* copy_s)
{
    S.sel.clear();
    for (int64_t i = 0; i < m; ++i) {
        leaf_code[i] = (uint16_t)VQHIP_VEC3_RES_KEPT;
        if (!(err[i * VQHIP_VEC3_ERR_FLOATS] <= tol)) S.sel.push_back(i);
    }
    const int64_t s = (int64_t)S.sel.size();
    if (s == 0) return VQHIP_OK;   // no GPU work
    if (int rc = v3_ensure_io(c, s)) return rc;
    if (int rc = v3m_ensure_host(c, s)) return rc;
    const float* src = leaves;
    const uint16_t* h_idx = indices;
    const uint64_t* h_mask = masks;
    const float* h_err = err;
    if (!leaves || s < m) {
        if (int rc = v3f_ensure_stage(c, s)) return rc;
        const double t = now_s();
        float* stage = c->fl_stage;
        const int64_t* sel = S.sel.data();
        host_parallel_for(s, [=](int64_t a, int64_t b) {
            for (int64_t j = a; j < b; ++j) std::memcpy(stage + j * 1536, leaves ? leaves + sel[j] * 1536 : leaf_ptrs[sel[j]], 6144);
        }, V3F_COPY_GRAIN);
        if (copy_s) *copy_s += now_s() - t;
        src = stage;
    }
    if (s < m) {
        S.idx.resize((size_t)s * 64), S.mask.resize((size_t)s * 8), S.err.resize((size_t)s * VQHIP_VEC3_ERR_FLOATS);
        for (int64_t j = 0; j < s; ++j) {
            const int64_t i = S.sel[j];
            std::memcpy(&S.idx[j * 64], indices + i * 64, 128);
            std::memcpy(&S.mask[j * 8], masks + i * 8, 64);
            std::memcpy(&S.err[j * VQHIP_VEC3_ERR_FLOATS], err + i * VQHIP_VEC3_ERR_FLOATS, VQHIP_VEC3_ERR_FLOATS * sizeof(float));
        }
        h_idx = S.idx.data(), h_mask = S.mask.data(), h_err = S.err.data();
    }
    S.code.resize((size_t)s);
    HIPCHK(c, hipMemcpyAsync(c->io_leaves, src, (size_t)s * 1536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->io_idx, h_idx, (size_t)s * 64 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->mk_mask, h_mask, (size_t)s * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rs_err, h_err, (size_t)s * VQHIP_VEC3_ERR_FLOATS * sizeof(float), hipMemcpyHostToDevice, c->stream));
    int rc = v3_decode_mode(c, c->io_idx, s, c->rs_recon, c->stream);
    if (!rc) rc = v3a_encode(c, c->io_leaves, c->rs_recon, c->mk_mask, c->rs_err, s, tol, c->rs_code, c->rs_off, c->rs_payload, s * 6144, c->stream);
    if (rc) {
        hipStreamSynchronize(c->stream);   // the copies above may still read the host arrays
        return rc;
    }
    if ((rc = v3r_fetch_chunk(c, what, 0, s, S.code.data(), payload, total))) return rc;   // synchronises
    for (int64_t j = 0; j < s; ++j) leaf_code[S.sel[j]] = S.code[j];
    return VQHIP_OK;
}

// the handle's compact size sums, cleared on its stream / read back behind everything the stream holds
int v3b_begin(vqhip_vec3_codec* c)
{
    if (int rc = ensure(c, c->ac_bytes, (size_t)VQHIP_VEC3_RATE_MAX_TOLS, "the compact size sums")) return rc;
    HIPCHK(c, hipMemsetAsync(c->ac_bytes, 0, (size_t)VQHIP_VEC3_RATE_MAX_TOLS * sizeof(int64_t), c->stream));
    return VQHIP_OK;
}
int v3b_end(vqhip_vec3_codec* c, int n_tols, int64_t* bytes)
{
    HIPCHK(c, hipMemcpyAsync(bytes, c->ac_bytes, (size_t)n_tols * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

// Pass 1 of one chunk: vqhip_vec3_active_sweep's sequence, which adds to c->ac_bytes; indices and leaf_err (both or neither) receive
// the chunk's indices and masked errors.  Nothing is synchronised.
int v3b_sweep_chunk(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t m, const vqrate::Tols& T, uint16_t* indices,
                    float* leaf_err)
{
    int rc = v3m_roundtrip_host(c, leaves, masks, 0, m);
    if (!rc) rc = v3a_sweep(c, c->io_leaves, c->rs_recon, c->mk_mask, c->rs_err, m, T, c->ac_bytes, c->stream);
    if (rc) {
        hipStreamSynchronize(c->stream);   // the copies above may still read the host arrays
        return rc;
    }
    if (indices) {
        HIPCHK(c, hipMemcpyAsync(indices, c->io_idx, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(leaf_err, c->rs_err, (size_t)m * VQHIP_VEC3_ERR_FLOATS * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    return VQHIP_OK;
}

// Pass 1 over the grids of a file call: bytes [n_grids][n_tols] receives every grid's compact payload at every rung; indices and
// leaf_err (both or neither; the grids' leaves one after another) every leaf's indices and masked error.  Batches are gathered into
// the pinned stage, so each one is finished before the next gather overwrites it.
int v3b_file_pass1(vqhip_vec3_codec* c, const char* what, const vqhip_vec3_grid_source* grids, int n_grids, const float* tols, int n_tols,
                   int64_t batch_leaves, int64_t* bytes, uint16_t* indices, float* leaf_err, vqhip_stream_stats& st)
{
    if (int rc = v3_prepare(c)) return rc;
    const vqrate::Tols T = rate_tols(tols, n_tols);
    int64_t base = 0;   // leaves of the grids before this one
    for (int g = 0; g < n_grids; ++g) {
        const vqhip_vec3_grid_source& G = grids[g];
        const int64_t n = G.n_leaves, step = v3f_step(c, batch_leaves);
        std::memset(bytes + (size_t)g * n_tols, 0, (size_t)n_tols * sizeof(int64_t));
        if (n == 0) continue;
        if (int rc = v3b_begin(c)) return rc;
        for (int64_t o = 0; o < n; o += step) {
            const int64_t m = std::min(step, n - o);
            if (int rc = v3f_check_ptrs(c, what, G.leaf_ptrs + o, m)) return rc;
            if (int rc = v3f_ensure_stage(c, m)) return rc;
            const double t = now_s();
            v3f_gather(c->fl_stage, G.leaf_ptrs + o, m);
            st.copy_s += now_s() - t;
            if (int rc = v3b_sweep_chunk(c, c->fl_stage, G.masks + o * 8, m, T, indices ? indices + (base + o) * 64 : nullptr,
                                         leaf_err ? leaf_err + (base + o) * VQHIP_VEC3_ERR_FLOATS : nullptr))
                return rc;
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (int rc = v3b_end(c, n_tols, bytes + (size_t)g * n_tols)) return rc;
        base += n;
    }
    return VQHIP_OK;
}

// pass 2 as a batch function of v3f_compress: the batch's indices are pass 1's, its codes and records those of its selected leaves
struct V3bFileBatch {
    vqhip_vec3_codec* c;
    const char* what;
    float tol;
    const uint16_t* indices;          // pass 1's, the grids' leaves one after another
    const float* leaf_err;
    const std::vector<int64_t>& base; // [n_grids]: leaves of the grids before each one
    V3bScratch& S;
    vqhip_stream_stats& st;
    int operator()(int g, const vqhip_vec3_grid_source& G, int64_t o, int64_t m, uint16_t* idx, uint16_t* code, uint8_t* payload, int64_t* bytes) const
    {
        const int64_t at = base[(size_t)g] + o;
        std::memcpy(idx, indices + at * 64, (size_t)m * 128);
        return v3b_encode_selected(c, what, nullptr, G.leaf_ptrs + o, G.masks + o * 8, idx, leaf_err + at * VQHIP_VEC3_ERR_FLOATS, m, tol, code, payload,
                                   bytes, S, &st.copy_s);
    }
};

}  // namespace

extern "C" {

int vqhip_vec3_budget_pick(const int64_t* bytes, const float* tols, int n_tols, int64_t budget)
{
    return vqv3b::active_rate_pick(bytes, tols, n_tols, budget);
}

int64_t vqhip_vec3_budget_file_bytes(const vqhip_vec3_grid_source* grids, int n_grids, int kind, const int64_t* payload_bytes)
{
    return vqv3b::file_bytes(grids, n_grids, kind, payload_bytes);
}

int vqhip_vec3_budget_compress(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t n, const float* tols, int n_tols,
                               int64_t payload_budget, float* tol_used, int64_t* bytes, uint16_t* indices, float* leaf_err, uint16_t* leaf_code,
                               uint8_t* payload, int64_t* payload_bytes)
{
    const char* what = "vec3 rate_compress_active";
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": n_leaves < 0");
    if (!tol_used || !payload_bytes) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": tol_used or payload_bytes is NULL");
    *payload_bytes = 0;
    if (payload_budget < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": payload_budget < 0");
    if (int rc = rate_check_tols(c, what, tols, n_tols)) return rc;
    int64_t sizes[VQHIP_VEC3_RATE_MAX_TOLS];
    std::memset(sizes, 0, sizeof sizes);
    if (n == 0) {   // every rung needs 0 bytes: the smallest that is not NaN, if there is one
        if (bytes) std::memcpy(bytes, sizes, (size_t)n_tols * sizeof(int64_t));
        const int best = vqv3b::active_rate_pick(sizes, tols, n_tols, payload_budget);
        if (best >= 0) *tol_used = tols[best];
        return VQHIP_OK;
    }
    if (!leaves || !masks || !indices || !leaf_code || !payload) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": null pointer");
    std::unique_ptr<float[]> own;
    if (!leaf_err) {
        own.reset(new (std::nothrow) float[(size_t)n * VQHIP_VEC3_ERR_FLOATS]);
        if (!own) return v3_fail(c, VQHIP_ERR_NOMEM, std::string(what) + ": cannot allocate the leaf errors of " + std::to_string(n) + " leaves");
        leaf_err = own.get();
    }
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = v3b_begin(c)) return rc;
    const vqrate::Tols T = rate_tols(tols, n_tols);
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3b_sweep_chunk(c, leaves + o * 1536, masks + o * 8, m, T, indices + o * 64, leaf_err + o * VQHIP_VEC3_ERR_FLOATS)) return rc;
    }
    if (int rc = v3b_end(c, n_tols, sizes)) return rc;
    if (bytes) std::memcpy(bytes, sizes, (size_t)n_tols * sizeof(int64_t));
    int64_t smallest = -1;
    const int best = vqv3b::active_rate_pick(sizes, tols, n_tols, payload_budget, &smallest);
    if (best < 0) {
        if (smallest < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": every rung is NaN, none can be chosen");
        return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": the smallest payload of the " + std::to_string(n_tols) + " rungs has " +
                                                 std::to_string(smallest) + " bytes, the budget is " + std::to_string(payload_budget) + " bytes");
    }
    const float tol = tols[best];
    *tol_used = tol;
    V3bScratch S;
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3b_encode_selected(c, what, leaves + o * 1536, nullptr, masks + o * 8, indices + o * 64, leaf_err + o * VQHIP_VEC3_ERR_FLOATS, m,
                                         tol, leaf_code + o, payload, &total, S, nullptr))
            return rc;
    }
    if (total != sizes[best])
        return v3_fail(c, VQHIP_ERR_DEVICE, std::string(what) + ": the payload has " + std::to_string(total) + " bytes, the sweep predicted " +
                                                std::to_string(sizes[best]));
    *payload_bytes = total;
    return VQHIP_OK;
}

int vqhip_vec3_budget_file_sweep(vqhip_vec3_codec* c, const vqhip_vec3_grid_source* grids, int n_grids, const float* tols, int n_tols,
                                 int64_t batch_leaves, int64_t* bytes)
{
    const char* what = "vec3 rate_sweep_file";
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_check_grids(c, what, false, nullptr, grids, n_grids, vqv3f::KIND_ACTIVE)) return rc;
    if (int rc = rate_check_tols(c, what, tols, n_tols)) return rc;
    if (!bytes) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": bytes is NULL");
    vqhip_stream_stats st;
    std::memset(&st, 0, sizeof st);
    return v3b_file_pass1(c, what, grids, n_grids, tols, n_tols, batch_leaves, bytes, nullptr, nullptr, st);
}

int vqhip_vec3_budget_file_compress(vqhip_vec3_codec* c, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, const float* tols,
                                    int n_tols, int64_t file_budget, int64_t batch_leaves, vqhip_stream_stats* stats, float* tol_used,
                                    int64_t* payload_bytes, int64_t* file_bytes)
{
    const char* what = "vec3 compress_file_budget";
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_check_grids(c, what, true, path, grids, n_grids, vqv3f::KIND_ACTIVE)) return rc;
    if (!tol_used || !file_bytes) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": tol_used or file_bytes is NULL");
    if (file_budget < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": file_budget < 0");
    if (int rc = rate_check_tols(c, what, tols, n_tols)) return rc;
    const double t_start = now_s();
    vqhip_stream_stats st;
    std::memset(&st, 0, sizeof st);
    std::vector<int64_t> base((size_t)n_grids);
    int64_t leaves = 0;
    for (int g = 0; g < n_grids; ++g) base[(size_t)g] = leaves, leaves += grids[g].n_leaves;   // at most 255 * 2^32
    // pass 1's indices and masked errors of every leaf, 136 B each, not initialised
    std::unique_ptr<uint16_t[]> idx(new (std::nothrow) uint16_t[(size_t)std::max<int64_t>(leaves, 1) * 64]);
    std::unique_ptr<float[]> err(new (std::nothrow) float[(size_t)std::max<int64_t>(leaves, 1) * VQHIP_VEC3_ERR_FLOATS]);
    if (!idx || !err)
        return v3_fail(c, VQHIP_ERR_NOMEM, std::string(what) + ": cannot allocate the indices and errors of " + std::to_string(leaves) + " leaves");
    std::vector<int64_t> sizes((size_t)n_grids * n_tols);
    if (int rc = v3b_file_pass1(c, what, grids, n_grids, tols, n_tols, batch_leaves, sizes.data(), idx.get(), err.get(), st)) return rc;
    // the pick is on the file's size at every rung
    int64_t file_at[VQHIP_VEC3_RATE_MAX_TOLS];
    std::vector<int64_t> per_grid((size_t)n_grids);
    for (int t = 0; t < n_tols; ++t) {
        for (int g = 0; g < n_grids; ++g) per_grid[(size_t)g] = sizes[(size_t)g * n_tols + t];
        file_at[t] = vqv3b::file_bytes(grids, n_grids, vqv3f::KIND_ACTIVE, per_grid.data());
        if (file_at[t] < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": the size of the file at rung " + std::to_string(t) + " has no 64-bit value");
    }
    int64_t smallest = -1;
    const int best = vqv3b::active_rate_pick(file_at, tols, n_tols, file_budget, &smallest);
    if (best < 0) {
        if (smallest < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": every rung is NaN, none can be chosen");
        return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": the smallest file of the " + std::to_string(n_tols) + " rungs has " +
                                                 std::to_string(smallest) + " bytes, the budget is " + std::to_string(file_budget) + " bytes");
    }
    const float tol = tols[best];
    V3bScratch S;
    std::vector<int64_t> written((size_t)n_grids);
    if (int rc = v3f_write_file(c, what, path, grids, n_grids, vqv3f::KIND_ACTIVE, tol, batch_leaves, st, written.data(),
                                V3bFileBatch{c, what, tol, idx.get(), err.get(), base, S, st}))
        return rc;
    for (int g = 0; g < n_grids; ++g)
        if (written[(size_t)g] != sizes[(size_t)g * n_tols + best]) {
            std::remove(path);
            return v3_fail(c, VQHIP_ERR_DEVICE, std::string(what) + ": the payload of grid " + std::to_string(g) + " has " + std::to_string(written[(size_t)g]) +
                                                    " bytes, the sweep predicted " + std::to_string(sizes[(size_t)g * n_tols + best]));
        }
    *tol_used = tol;
    *file_bytes = file_at[best];
    if (payload_bytes) std::memcpy(payload_bytes, written.data(), (size_t)n_grids * sizeof(int64_t));
    st.wall_s = now_s() - t_start;
    if (stats) *stats = st;
    return VQHIP_OK;
}

}  // extern "C"
