// vq_vec3_file.inc — the Vec3 handle's leaf-pointer and file calls (vqhip_vec3_encode_leaves, _decode_leaves, _file_compress,
// _file_compress_active, _file_decompress, _file_info; include/vqvdb_hip_vec3_file.h, DESIGN.md §26).  Part of vq_runtime.hip's
// translation unit, after vq_vec3_active.inc.  No kernel of its own: a batch is gathered into pinned staging and handed to the chunk
// functions of the in-memory calls (v3_encode_host_chunk, v3_decode_host_chunk, v3a_compress_chunk, v3a_decompress_chunk), and the
// container is vq_vec3_file_format.h's.  Chunked and serial: gather, GPU work and file I/O of a batch follow one another.  The writer
// (v3f_compress) takes the function that fills a batch's indices, codes and records as a parameter: V3fModelBatch here, pass 2 of the
// byte-budget call in vq_vec3_budget.inc.

#include "../../include/vqvdb_hip_vec3_file.h"
#include "vq_vec3_file_format.h"

static_assert(vqv3f::CODE_KEPT == vqr::Format<3>::KEPT && vqv3f::CODE_RAW == vqr::Format<3>::RAW, "the container's codes are the kernels'");
static_assert(VQHIP_VEC3_FILE_VERSION == vqv3f::VERSION && VQHIP_VEC3_FILE_HEADER_BYTES == vqv3f::FILE_HEADER_BYTES &&
                  VQHIP_VEC3_FILE_KIND_INDICES == vqv3f::KIND_INDICES && VQHIP_VEC3_FILE_KIND_ACTIVE == vqv3f::KIND_ACTIVE,
              "the header's constants are the container's");

namespace {

constexpr int64_t V3F_COPY_GRAIN = 512;   // leaves of 6 KiB per copy thread before another one pays

// per-leaf buffers into a contiguous (pinned) block / a block into per-leaf buffers, on the library's copy threads
void v3f_gather(float* stage, const float* const* lp, int64_t m)
{
    host_parallel_for(m, [=](int64_t a, int64_t b) {
        for (int64_t l = a; l < b; ++l) std::memcpy(stage + l * 1536, lp[l], 6144);
    }, V3F_COPY_GRAIN);
}
void v3f_scatter(float* const* dst, const float* src, int64_t m)
{
    host_parallel_for(m, [=](int64_t a, int64_t b) {
        for (int64_t l = a; l < b; ++l) std::memcpy(dst[l], src + l * 1536, 6144);
    }, V3F_COPY_GRAIN);
}

int v3f_check_ptrs(vqhip_vec3_codec* c, const char* what, const float* const* lp, int64_t n)
{
    for (int64_t l = 0; l < n; ++l)
        if (!lp[l]) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": leaf pointer " + std::to_string(l) + " is NULL");
    return VQHIP_OK;
}

int v3f_ensure_stage(vqhip_vec3_codec* c, int64_t m) { return ensure(c, c->fl_stage, (size_t)m * 1536, "the pinned leaf stage"); }

// leaves per batch of a file call: the caller's wish, never above the handle's chunk (after v3_prepare has fitted it)
int64_t v3f_step(const vqhip_vec3_codec* c, int64_t batch_leaves) { return batch_leaves > 0 ? std::min(batch_leaves, c->chunk) : c->chunk; }

const char* v3f_mode_name(int mode) { return mode == VQHIP_VEC3_PRECISION_BF16 ? "bf16" : "fp32"; }

// a batch of the compress by the model: the leaves o .. o + m of grid G gathered into the pinned stage, then the chunk function of
// the in-memory call of that kind.  The batch functions of v3f_compress fill idx [m][64] and, kind 1, code [m] and the batch's records
// from payload on, *bytes their size; the time of their gathers goes to st.copy_s.
struct V3fModelBatch {
    vqhip_vec3_codec* c;
    const char* what;
    int kind;
    float tol;
    vqhip_stream_stats& st;
    int operator()(int, const vqhip_vec3_grid_source& G, int64_t o, int64_t m, uint16_t* idx, uint16_t* code, uint8_t* payload, int64_t* bytes) const
    {
        if (int rc = v3f_check_ptrs(c, what, G.leaf_ptrs + o, m)) return rc;
        if (int rc = v3f_ensure_stage(c, m)) return rc;
        const double t = now_s();
        v3f_gather(c->fl_stage, G.leaf_ptrs + o, m);
        st.copy_s += now_s() - t;
        if (kind) return v3a_compress_chunk(c, what, c->fl_stage, G.masks + o * 8, m, tol, idx, nullptr, code, payload, bytes);
        return v3_encode_host_chunk(c, c->fl_stage, m, idx);
    }
};

// kind 0 (tol unused) or kind 1 of the compress, every batch's indices, codes and records from `batch`; the partial output is the
// caller's to remove when this fails.  vqhip_stream_stats has one field for file I/O, read_s ("file read/write"): here it collects
// the time of the writes, copy_s that of the gathers.
template <typename Batch>
int v3f_compress(vqhip_vec3_codec* c, const char* what, vqv3f::File& f, const vqhip_vec3_grid_source* grids, int n_grids, int kind, float tol,
                 int64_t batch_leaves, vqhip_stream_stats& st, int64_t* payload_bytes, const Batch& batch)
{
    const std::string wfail = std::string(what) + ": failed to write to the .vqv3 file";
    if (int rc = v3_prepare(c)) return rc;
    vqv3f::Header h;
    h.n_grids = n_grids, h.num_codes = (uint32_t)c->k_codes, h.kind = kind, h.mode = kind ? c->precision : 0, h.tol = kind ? tol : 0.0f;
    unsigned char hb[vqv3f::FILE_HEADER_BYTES];
    vqv3f::emit_header(h, hb);
    if (!f.write_at(0, hb, sizeof hb)) return v3_fail(c, VQHIP_ERR_INVALID, wfail);
    std::vector<unsigned char> meta;
    std::vector<uint16_t> idx, code;
    std::unique_ptr<uint8_t[]> payload;   // room for a batch's largest payload, not initialised: only the bytes of its records are ever touched
    int64_t payload_leaves = 0;
    uint64_t at = vqv3f::FILE_HEADER_BYTES;
    for (int g = 0; g < n_grids; ++g) {
        const vqhip_vec3_grid_source& G = grids[g];
        vqv3f::Grid M;
        M.name = G.name;
        if (G.transform) std::memcpy(M.transform, G.transform, 64);
        M.total = (uint32_t)G.n_leaves;
        M.has_background = G.background ? 1 : 0;
        if (G.background) std::memcpy(M.background, G.background, 12);
        vqv3f::layout(M, kind, at);
        vqv3f::emit_grid_meta(M, meta);
        double t = now_s();
        if (!f.write_at(at, meta.data(), meta.size())) return v3_fail(c, VQHIP_ERR_INVALID, wfail);
        st.read_s += now_s() - t;
        ++st.grids;
        const int64_t n = G.n_leaves, step = v3f_step(c, batch_leaves);
        int64_t total = 0;   // the grid's payload bytes so far
        for (int64_t o = 0; o < n; o += step) {
            const int64_t m = std::min(step, n - o);
            idx.resize((size_t)m * 64);
            int64_t bytes = 0;
            if (kind) {
                code.resize((size_t)m);
                if (m > payload_leaves) {
                    payload.reset(new (std::nothrow) uint8_t[(size_t)m * 6144]);
                    payload_leaves = payload ? m : 0;
                    if (!payload) return v3_fail(c, VQHIP_ERR_NOMEM, std::string(what) + ": cannot allocate the payload buffer of " + std::to_string(m) + " leaves");
                }
            }
            if (int rc = batch(g, G, o, m, idx.data(), code.data(), payload.get(), &bytes)) return rc;
            t = now_s();
            bool ok = f.write_at(M.origins_at + 12 * (uint64_t)o, G.origins + 3 * o, 12 * (uint64_t)m) &&
                      f.write_at(M.indices_at + 128 * (uint64_t)o, idx.data(), 128 * (uint64_t)m);
            if (ok && kind)
                ok = f.write_at(M.masks_at + 64 * (uint64_t)o, G.masks + o * 8, 64 * (uint64_t)m) &&
                     f.write_at(M.codes_at + 2 * (uint64_t)o, code.data(), 2 * (uint64_t)m) &&
                     f.write_at(M.payload_at + (uint64_t)total, payload.get(), (uint64_t)bytes);
            st.read_s += now_s() - t;
            if (!ok) return v3_fail(c, VQHIP_ERR_INVALID, wfail);
            total += bytes;
        }
        M.payload_bytes = (uint64_t)total;
        if (total && !f.write_at(M.payload_field_at, &M.payload_bytes, 8)) return v3_fail(c, VQHIP_ERR_INVALID, wfail);   // patched when the grid ends
        if (payload_bytes) payload_bytes[g] = total;
        st.leaves += n;
        at = M.payload_at + M.payload_bytes;
    }
    return VQHIP_OK;
}

// what a compress refuses of its path and grid list before anything is opened or launched (path NULL: a call without an output)
int v3f_check_grids(vqhip_vec3_codec* c, const std::string& what, bool need_path, const char* path, const vqhip_vec3_grid_source* grids, int n_grids,
                    int kind)
{
    if ((need_path && !path) || !grids) return v3_fail(c, VQHIP_ERR_INVALID, what + ": null path or grid list");
    if (n_grids < 1 || n_grids > 255) return v3_fail(c, VQHIP_ERR_INVALID, what + ": a .vqv3 file holds 1..255 grids");
    for (int g = 0; g < n_grids; ++g) {
        const vqhip_vec3_grid_source& G = grids[g];
        if (!G.name || G.n_leaves < 0 || G.n_leaves > 0xFFFFFFFFll || (G.n_leaves > 0 && (!G.leaf_ptrs || !G.origins)))
            return v3_fail(c, VQHIP_ERR_INVALID, what + ": grid " + std::to_string(g) + " has no name, no leaves/origins or more than 2^32-1 leaves");
        if (kind && G.n_leaves > 0 && !G.masks) return v3_fail(c, VQHIP_ERR_INVALID, what + ": grid " + std::to_string(g) + " has no masks");
    }
    return VQHIP_OK;
}

// the output opened, written by v3f_compress, closed, and removed if any of that failed
template <typename Batch>
int v3f_write_file(vqhip_vec3_codec* c, const char* what, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, int kind, float tol,
                   int64_t batch_leaves, vqhip_stream_stats& st, int64_t* payload_bytes, const Batch& batch)
{
    vqv3f::File f;
    if (!f.open_write(path)) return v3_fail(c, VQHIP_ERR_INVALID, std::string("Cannot open output file: ") + path);
    int rc = v3f_compress(c, what, f, grids, n_grids, kind, tol, batch_leaves, st, payload_bytes, batch);
    if (!f.close() && !rc) rc = v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": error closing the output file");
    if (rc) std::remove(path);   // no partial output
    return rc;
}

int v3f_compress_file(vqhip_vec3_codec* c, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, int kind, float tol,
                      int64_t batch_leaves, vqhip_stream_stats* stats, int64_t* payload_bytes)
{
    const char* what = kind ? "vec3 compress_file_active" : "vec3 compress_file";
    if (int rc = v3f_check_grids(c, what, true, path, grids, n_grids, kind)) return rc;
    const double t_start = now_s();
    vqhip_stream_stats st;
    std::memset(&st, 0, sizeof st);
    if (int rc = v3f_write_file(c, what, path, grids, n_grids, kind, tol, batch_leaves, st, payload_bytes, V3fModelBatch{c, what, kind, tol, st}))
        return rc;
    st.wall_s = now_s() - t_start;
    if (stats) *stats = st;
    return VQHIP_OK;
}

}  // namespace

extern "C" {

int vqhip_vec3_encode_leaves(vqhip_vec3_codec* c, const float* const* leaf_ptrs, int64_t n, uint16_t* indices)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 encode_leaves: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!leaf_ptrs || !indices) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 encode_leaves: null pointer");
    if (int rc = v3f_check_ptrs(c, "vec3 encode_leaves", leaf_ptrs, n)) return rc;
    if (int rc = v3_prepare(c)) return rc;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3f_ensure_stage(c, m)) return rc;
        v3f_gather(c->fl_stage, leaf_ptrs + o, m);
        if (int rc = v3_encode_host_chunk(c, c->fl_stage, m, indices + o * 64)) return rc;
    }
    return VQHIP_OK;
}

int vqhip_vec3_decode_leaves(vqhip_vec3_codec* c, const uint16_t* indices, int64_t n, float* const* leaf_ptrs)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decode_leaves: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!leaf_ptrs || !indices) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decode_leaves: null pointer");
    if (int rc = v3f_check_ptrs(c, "vec3 decode_leaves", leaf_ptrs, n)) return rc;
    if (int rc = v3_check_indices(c, indices, n, 0)) return rc;
    if (int rc = v3_prepare(c)) return rc;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = v3f_ensure_stage(c, m)) return rc;
        if (int rc = v3_decode_host_chunk(c, indices + o * 64, m, c->fl_stage)) return rc;
        v3f_scatter(leaf_ptrs + o, c->fl_stage, m);
    }
    return VQHIP_OK;
}

int vqhip_vec3_file_compress(vqhip_vec3_codec* c, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, int64_t batch_leaves,
                             vqhip_stream_stats* stats)
{
    if (!c) return VQHIP_ERR_INVALID;
    return v3f_compress_file(c, path, grids, n_grids, vqv3f::KIND_INDICES, 0.0f, batch_leaves, stats, nullptr);
}

int vqhip_vec3_file_compress_active(vqhip_vec3_codec* c, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, float tol,
                                    int64_t batch_leaves, vqhip_stream_stats* stats, int64_t* payload_bytes)
{
    if (!c) return VQHIP_ERR_INVALID;
    return v3f_compress_file(c, path, grids, n_grids, vqv3f::KIND_ACTIVE, tol, batch_leaves, stats, payload_bytes);
}

int vqhip_vec3_file_decompress(vqhip_vec3_codec* c, const char* path, int64_t batch_leaves, vqhip_vec3_grid_begin_fn grid_begin,
                               vqhip_vec3_leaf_alloc_fn leaf_alloc, void* user, vqhip_stream_stats* stats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !leaf_alloc) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_file: null path or leaf allocator");
    const double t_start = now_s();
    vqhip_stream_stats st;
    std::memset(&st, 0, sizeof st);
    vqv3f::File f;
    if (!f.open_read(path)) return v3_fail(c, VQHIP_ERR_INVALID, std::string("Cannot open input file: ") + path);
    vqv3f::Header h;
    std::vector<vqv3f::Grid> grids;
    std::string err;
    if (!vqv3f::read_index(f, h, grids, err)) return v3_fail(c, VQHIP_ERR_INVALID, err);
    if ((int64_t)h.num_codes != c->k_codes)
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_file: the file was written with " + std::to_string(h.num_codes) + " codes, this model has " +
                                                 std::to_string(c->k_codes));
    const bool active = h.kind == vqv3f::KIND_ACTIVE;
    if (active && h.mode != c->precision)
        return v3_fail(c, VQHIP_ERR_INVALID, std::string("vec3 decompress_file: the file's records belong to the ") + v3f_mode_name(h.mode) +
                                                 " decoder, the handle is in " + v3f_mode_name(c->precision) + " mode (switch it with vqhip_vec3_set_precision)");
    if (int rc = v3_prepare(c)) return rc;
    std::vector<int32_t> origins;
    std::vector<uint16_t> idx, code;
    std::vector<uint64_t> mask;
    std::vector<uint8_t> payload;
    std::vector<int64_t> off;
    std::vector<float*> ptrs;
    for (int g = 0; g < h.n_grids; ++g) {
        const vqv3f::Grid& G = grids[g];
        double t = now_s();
        if (!vqv3f::check_grid(f, h, G, err)) return v3_fail(c, VQHIP_ERR_INVALID, err);   // before grid_begin, leaf_alloc and any GPU work
        st.read_s += now_s() - t;
        vqhip_vec3_grid_info gi;
        std::memset(&gi, 0, sizeof gi);
        gi.name = G.name.c_str();
        std::memcpy(gi.transform, G.transform, 64);
        gi.num_codes = h.num_codes, gi.total_blocks = G.total, gi.grid_index = g, gi.kind = h.kind, gi.mode = h.mode, gi.tol = h.tol;
        gi.has_background = G.has_background;
        std::memcpy(gi.background, G.background, 12);
        if (grid_begin && grid_begin(user, &gi) != 0) return v3_fail(c, VQHIP_ERR_INVALID, "grid_begin callback failed for grid '" + G.name + "'");
        ++st.grids;
        const int64_t n = G.total, step = v3f_step(c, batch_leaves);
        uint64_t pay_at = G.payload_at;
        for (int64_t o = 0; o < n; o += step) {
            const int64_t m = std::min(step, n - o);
            t = now_s();
            origins.resize((size_t)m * 3);
            idx.resize((size_t)m * 64);
            bool ok = f.read_at(G.origins_at + 12 * (uint64_t)o, origins.data(), 12 * (uint64_t)m) &&
                      f.read_at(G.indices_at + 128 * (uint64_t)o, idx.data(), 128 * (uint64_t)m);
            uint64_t bytes = 0;
            if (ok && active) {
                mask.resize((size_t)m * 8);
                code.resize((size_t)m);
                ok = f.read_at(G.masks_at + 64 * (uint64_t)o, mask.data(), 64 * (uint64_t)m) && f.read_at(G.codes_at + 2 * (uint64_t)o, code.data(), 2 * (uint64_t)m);
                // the file may have changed since check_grid: the batch's codes and sizes are checked again where they are used
                for (int64_t i = 0; ok && i < m; ++i) {
                    if (!vqv3f::code_ok(code[i])) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_file: the file changed while it was read");
                    bytes += vqv3f::record_bytes(code[i], vqv3f::popcount512(&mask[i * 8]));
                }
                if (ok && (pay_at + bytes > G.end_at)) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_file: the file changed while it was read");
                payload.resize((size_t)bytes);
                if (ok && bytes) ok = f.read_at(pay_at, payload.data(), bytes);
            }
            st.read_s += now_s() - t;
            if (!ok) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decompress_file: cannot read the sections of grid '" + G.name + "'");
            if (int rc = v3_check_indices(c, idx.data(), m, o)) return rc;
            ptrs.assign((size_t)m, nullptr);
            t = now_s();
            const int arc = leaf_alloc(user, g, origins.data(), active ? mask.data() : nullptr, m, ptrs.data());
            st.alloc_s += now_s() - t;
            if (arc != 0) return v3_fail(c, VQHIP_ERR_INVALID, "leaf_alloc callback failed (" + std::to_string(arc) + ")");
            for (int64_t l = 0; l < m; ++l)
                if (!ptrs[l]) return v3_fail(c, VQHIP_ERR_INVALID, "leaf_alloc callback left a null leaf pointer");
            if (int rc = v3f_ensure_stage(c, m)) return rc;
            if (active) {
                int64_t used = 0;
                if (int rc = v3a_decompress_chunk(c, idx.data(), mask.data(), m, h.tol, code.data(), payload.data(), G.has_background ? G.background : nullptr,
                                                  c->fl_stage, off, &used))
                    return rc;
                pay_at += bytes;
            } else if (int rc = v3_decode_host_chunk(c, idx.data(), m, c->fl_stage)) {
                return rc;
            }
            t = now_s();
            v3f_scatter(ptrs.data(), c->fl_stage, m);
            st.copy_s += now_s() - t;
        }
        st.leaves += n;
    }
    st.wall_s = now_s() - t_start;
    if (stats) *stats = st;
    return VQHIP_OK;
}

int vqhip_vec3_file_info(const char* path, int* n_grids, uint32_t* num_codes, int* kind, int* mode, float* tol, int64_t* total_blocks,
                         int64_t* payload_bytes)
{
    if (!path) return v3_fail(nullptr, VQHIP_ERR_INVALID, "vec3 file_info: null path");
    vqv3f::File f;
    if (!f.open_read(path)) return v3_fail(nullptr, VQHIP_ERR_INVALID, std::string("Cannot open input file: ") + path);
    vqv3f::Header h;
    std::vector<vqv3f::Grid> grids;
    std::string err;
    if (!vqv3f::read_index(f, h, grids, err)) return v3_fail(nullptr, VQHIP_ERR_INVALID, err);
    int64_t blocks = 0, bytes = 0;
    for (const vqv3f::Grid& G : grids) blocks += G.total, bytes += (int64_t)G.payload_bytes;
    if (n_grids) *n_grids = h.n_grids;
    if (num_codes) *num_codes = h.num_codes;
    if (kind) *kind = h.kind;
    if (mode) *mode = h.mode;
    if (tol) *tol = h.tol;
    if (total_blocks) *total_blocks = blocks;
    if (payload_bytes) *payload_bytes = bytes;
    return VQHIP_OK;
}

}  // extern "C"
