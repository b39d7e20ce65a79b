// vq_file.inc — the scalar handle's file calls: vqhip_compress_file / _decompress_file (include/vqvdb_hip.h) and the pairs that
// add a .vqres sidecar, _bounded (v1, vqvdb_hip_bounded.h, DESIGN.md §16) and _residual (v2, vqvdb_hip_residual.h, §17).  Part
// of vq_runtime.hip's translation unit, after vq_residual.inc: every call runs run_pipeline with a reader or writer around it,
// and the pairs pass it the stage that vq_bounded.inc or vq_residual.inc builds.

namespace {

// ---------------- .vqvdb v3 container (SURVEY.md App. B; reference src/Utils/VQVDB_Reader.{hpp,cpp}) ----------------
// file : "VQVDB" | u8 version=3 | u8 numGrids | u32 numEmbeddings | u8 latentDimCount
// grid : u32 nameLength | name | f32 transform[16] | u16 latentShape[latentDimCount] | u32 totalBlocks
//        totalBlocks x { i32 origin[3] | u8 indices[64] }   (76 B per leaf)
constexpr size_t REC_BYTES = 76;

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct FileCloser {
    FILE* f;
    ~FileCloser()
    {
        if (f) std::fclose(f);
    }
};

// One decoded-side batch travelling from the reader thread to the pipeline: indices de-framed from the records,
// origins, and the leaf addresses the caller's allocator returned for them.
struct StreamBatch {
    std::vector<uint8_t> idx;
    std::vector<int32_t> origins;
    std::vector<float*> ptrs;
    std::vector<unsigned char> raw;
};

// ---- .vqvdb stream entry points: file read || GPU decode || leaf insert (SURVEY.md §8 f-1) ----
// Replaces the body of VQVAECodec::decompress (VQVAECodec.cpp:137-208): per grid, a reader thread reads and de-frames
// batch k+1..k+2 and asks the caller's allocator for their leaf buffers while the GPU decodes batch k and the calling
// thread scatters batch k-1 straight from pinned memory into those buffers.
//
// residual_path, res_version 1 (vqhip_decompress_file_bounded; NULL, 0 without a sidecar): a .vqres sidecar (vqvdb_hip_bounded.h)
// read in step with the batches; after a batch's scatter the leaves it names are overwritten with its floats.  res_version 2
// (vqhip_decompress_file_residual): a .vqres v2 sidecar (vqvdb_hip_residual.h); rs_decode_stage reads the records of a decoded
// chunk forward, uploads and applies them on the GPU before the chunk leaves it.
int decompress_file_impl(vqhip_codec* c, const char* path, const char* residual_path, int res_version, int64_t batch_leaves,
                         vqhip_grid_begin_fn grid_begin, vqhip_leaf_alloc_fn leaf_alloc, void* user, vqhip_stream_stats* stats)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(c, VQHIP_ERR_INVALID, std::string("Cannot open input file: ") + path);
    FileCloser closer{f};
    const double t_start = now_s();
    vqhip_stream_stats st;
    std::memset(&st, 0, sizeof st);
    unsigned char h[12];
    if (std::fread(h, 1, 12, f) != 12) return fail(c, VQHIP_ERR_INVALID, "Failed to read file header.");
    if (std::memcmp(h, "VQVDB", 5) != 0) return fail(c, VQHIP_ERR_INVALID, "Invalid file magic; not a .vqvdb file.");
    if (h[5] != 3) return fail(c, VQHIP_ERR_INVALID, "Unsupported .vqvdb version " + std::to_string((int)h[5]) + " (expected 3).");
    const int n_grids = h[6], dim_count = h[11];
    uint32_t num_emb;
    std::memcpy(&num_emb, h + 7, 4);
    if (dim_count != 3) return fail(c, VQHIP_ERR_INVALID, "latent rank " + std::to_string(dim_count) + " in file; this codec decodes [4,4,4] latents");
    FILE* fr = nullptr;
    if (residual_path) {
        if (!(fr = std::fopen(residual_path, "rb"))) return fail(c, VQHIP_ERR_INVALID, std::string("Cannot open residual file: ") + residual_path);
    }
    FileCloser rcloser{fr};
    float res_tol = 0.0f;
    if (fr) {
        unsigned char rh[11];
        if (std::fread(rh, 1, 11, fr) != 11) return fail(c, VQHIP_ERR_INVALID, "Failed to read residual file header.");
        if (std::memcmp(rh, "VQRES", 5) != 0) return fail(c, VQHIP_ERR_INVALID, "Invalid residual file magic; not a .vqres file.");
        if (rh[5] != res_version)
            return fail(c, VQHIP_ERR_INVALID, "Unsupported .vqres version " + std::to_string((int)rh[5]) + " (expected " + std::to_string(res_version) + ").");
        std::memcpy(&res_tol, rh + 7, 4);
        if (rh[6] != n_grids)
            return fail(c, VQHIP_ERR_INVALID, "residual file holds " + std::to_string((int)rh[6]) + " grids, the .vqvdb file " + std::to_string(n_grids));
    }

    for (int g = 0; g < n_grids; ++g) {
        vqhip_grid_info gi;
        std::memset(&gi, 0, sizeof gi);
        uint32_t name_len = 0, total = 0;
        uint16_t shp[3];
        std::string name;
        if (std::fread(&name_len, 4, 1, f) != 1 || name_len > (1u << 20)) return fail(c, VQHIP_ERR_INVALID, "Failed to read grid name length.");
        name.resize(name_len);
        if (name_len && std::fread(&name[0], 1, name_len, f) != name_len) return fail(c, VQHIP_ERR_INVALID, "Failed to read grid name.");
        if (std::fread(gi.transform, 4, 16, f) != 16) return fail(c, VQHIP_ERR_INVALID, "Failed to read transform.");
        if (std::fread(shp, 2, 3, f) != 3) return fail(c, VQHIP_ERR_INVALID, "Failed to read latent shape.");
        if (std::fread(&total, 4, 1, f) != 1) return fail(c, VQHIP_ERR_INVALID, "File appears truncated, failed to read total block count.");
        if (shp[0] != 4 || shp[1] != 4 || shp[2] != 4)
            return fail(c, VQHIP_ERR_INVALID, "grid '" + name + "' has latent shape [" + std::to_string(shp[0]) + "," + std::to_string(shp[1]) + "," +
                                                  std::to_string(shp[2]) + "]; this codec decodes [4,4,4]");
        gi.name = name.c_str();
        gi.grid_index = g;
        for (int i = 0; i < 3; ++i) gi.latent_shape[i] = shp[i];
        gi.num_embeddings = num_emb;
        gi.total_blocks = total;
        if (grid_begin && grid_begin(user, &gi) != 0) return fail(c, VQHIP_ERR_INVALID, "grid_begin callback failed for grid '" + name + "'");
        ++st.grids;
        const int64_t n = total;
        const bool v2 = fr && res_version == 2;
        ResidualWalk walk{c, fr, v2, name, n};   // this grid's sidecar entries
        if (fr) {
            uint32_t n_out = 0;
            if (std::fread(&n_out, 4, 1, fr) != 1) return fail(c, VQHIP_ERR_INVALID, "Residual file truncated: no outlier count for grid '" + name + "'.");
            if ((int64_t)n_out > n)
                return fail(c, VQHIP_ERR_INVALID, "residual file: grid '" + name + "' lists " + std::to_string(n_out) + " leaves, the grid has " + std::to_string(n));
            walk.left = n_out;
        }
        const PipeStage stage = v2 ? rs_decode_stage(c, res_tol, &walk) : PipeStage{};
        if (n == 0) continue;
        const int64_t step = std::min(batch_leaves > 0 ? std::min(batch_leaves, c->chunk) : c->chunk, n);
        const int64_t nb = (n + step - 1) / step;

        constexpr int Q = 3;
        StreamBatch slot[Q];
        std::mutex mu;
        std::condition_variable cv;
        int64_t produced = 0, consumed = 0;
        bool failed = false, stop = false;
        std::string herr;
        double read_s = 0, alloc_s = 0, wait_s = 0, copy_s = 0;
        std::thread reader([&] {
            auto bail = [&](const std::string& m) {
                std::lock_guard<std::mutex> lk(mu);
                herr = m;
                failed = true;
                cv.notify_all();
            };
            for (int64_t k = 0; k < nb; ++k) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return stop || k - consumed < Q; });
                    if (stop) return;
                }
                const int64_t m = std::min(step, n - k * step);
                StreamBatch& B = slot[k % Q];
                double t = now_s();
                B.raw.resize((size_t)m * REC_BYTES);
                if (std::fread(B.raw.data(), REC_BYTES, (size_t)m, f) != (size_t)m) return bail("File truncated: incomplete block data.");
                B.idx.resize((size_t)m * 64);
                B.origins.resize((size_t)m * 3);
                B.ptrs.assign((size_t)m, nullptr);
                const unsigned char* p = B.raw.data();
                for (int64_t l = 0; l < m; ++l, p += REC_BYTES) {
                    std::memcpy(&B.origins[3 * l], p, 12);
                    std::memcpy(&B.idx[64 * l], p + 12, 64);
                }
                read_s += now_s() - t;
                t = now_s();
                const int rc = leaf_alloc(user, g, B.origins.data(), m, B.ptrs.data());
                alloc_s += now_s() - t;
                if (rc != 0) return bail("leaf_alloc callback failed (" + std::to_string(rc) + ")");
                for (int64_t l = 0; l < m; ++l)
                    if (!B.ptrs[l]) return bail("leaf_alloc callback left a null leaf pointer");
                std::lock_guard<std::mutex> lk(mu);
                produced = k + 1;
                cv.notify_all();
            }
        });
        const int rc = run_pipeline(
            c, false, n, step, false,
            [&](int64_t o, int64_t, void*) -> const void* {
                const int64_t k = o / step;
                const double t = now_s();
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return failed || produced > k; });
                wait_s += now_s() - t;
                if (produced <= k) {
                    c->err = herr;
                    return nullptr;
                }
                return slot[k % Q].idx.data() + (o - k * step) * 64;   // run_pipeline may cut a batch into pieces (host_split)
            },
            [&](const PipeChunk& ch) -> int {
                const int64_t k = ch.o / step;
                float* const* ptrs = slot[k % Q].ptrs.data() + (ch.o - k * step);
                const double t = now_s();
                scatter_leaves(ptrs, static_cast<const float*>(ch.result), ch.m);
                // v1: the chunk's raw leaves straight from the sidecar into the caller's buffers
                const int rrc = fr && !v2 ? walk.read_chunk(ch.o, ch.m, [&](int64_t l, int) { return ptrs[l]; }) : VQHIP_OK;
                copy_s += now_s() - t;
                if (ch.o + ch.m < std::min(n, (k + 1) * step)) return rrc;   // a piece of the batch: its slot is still in use
                std::lock_guard<std::mutex> lk(mu);
                consumed = k + 1;
                cv.notify_all();
                return rrc;
            },
            &stage,
            // the plain decompress follows the handle's decode mode; a sidecar's records are corrections of the fp32 reconstruction
            residual_path ? VQHIP_PRECISION_FP32 : c->decode_precision);
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        reader.join();
        if (rc) return rc;
        st.leaves += n;
        st.read_s += read_s, st.alloc_s += alloc_s, st.io_wait_s += wait_s, st.copy_s += copy_s;
    }
    st.wall_s = now_s() - t_start;
    if (stats) *stats = st;
    return VQHIP_OK;
}

// The .vqres file a compress writes beside the .vqvdb, as far as both versions share it: per grid a count, a placeholder until the
// grid is done, then the entries of the leaves that are not kept; the kept leaves' errors go into the call's statistics.
struct SidecarOut {
    FILE* fr;
    bool failed = false;
    long count_pos = 0;
    uint32_t grid_out = 0;             // entries of the grid being written
    vqhip_bounded_stats bst{};
    std::vector<unsigned char> rec;    // v2: a chunk's framed entries

    void put(const void* p, size_t n)
    {
        if (std::fwrite(p, 1, n, fr) != n) failed = true;
    }
    void kept(const float* e)   // the leaf's {max |d|, sum d^2}
    {
        bst.max_err_kept = std::max(bst.max_err_kept, e[0]);
        bst.sum_sq_kept += e[1];
    }
    bool begin_grid()
    {
        grid_out = 0;
        count_pos = std::ftell(fr);
        put(&grid_out, 4);
        return !failed && count_pos >= 0;
    }
    bool end_grid()
    {
        if (std::fseek(fr, count_pos, SEEK_SET) != 0) failed = true;
        put(&grid_out, 4);
        if (std::fseek(fr, 0, SEEK_END) != 0) failed = true;
        bst.outliers += grid_out;
        return !failed;
    }
};

// .vqres v1: the chunk's leaves with !(max error <= tol), raw from the caller's buffers.  e: the chunk's {max |d|, sum d^2} per leaf
void write_sidecar_v1(SidecarOut& out, const PipeChunk& ch, const float* e, const float* const* leaf_ptrs, float tol)
{
    for (int64_t l = 0; l < ch.m; ++l) {
        if (e[2 * l] <= tol) {
            out.kept(e + 2 * l);
            continue;
        }
        const uint32_t ri = (uint32_t)(ch.o + l);
        out.put(&ri, 4);
        out.put(leaf_ptrs[ch.o + l], 2048);
        ++out.grid_out;
    }
}

// .vqres v2: the chunk's classes lie in the slot's pinned block and its payload is fetched now; every leaf that is not kept gets
// {index, class, record}
int write_sidecar_v2(vqhip_codec* c, SidecarOut& out, const PipeChunk& ch, const float* e, vqhip_residual_stats& rst)
{
    const unsigned char* pay = nullptr;
    int64_t pay_bytes = 0, at = 0;
    if (int rc = rs_fetch_payload(c, ch, &pay, &pay_bytes)) return rc;
    const unsigned char* cls = rs_pin_class(c, ch.slot);
    out.rec.clear();
    for (int64_t l = 0; l < ch.m; ++l) {
        if (cls[l] == VQHIP_RES_KEPT) {
            out.kept(e + 2 * l);
            continue;
        }
        if (cls[l] > 16 && cls[l] != VQHIP_RES_RAW) return fail(c, VQHIP_ERR_DEVICE, "compress_file_residual: class out of range");
        const int64_t sz = vqr::record_size<1>(cls[l]);
        if (at + sz > pay_bytes) return fail(c, VQHIP_ERR_DEVICE, "compress_file_residual: records exceed the payload");
        const uint32_t ri = (uint32_t)(ch.o + l);
        const size_t w = out.rec.size();
        out.rec.resize(w + 5 + (size_t)sz);
        std::memcpy(&out.rec[w], &ri, 4);
        out.rec[w + 4] = cls[l];
        std::memcpy(&out.rec[w + 5], pay + at, (size_t)sz);
        at += sz;
        ++out.grid_out;
        ++(cls[l] == VQHIP_RES_RAW ? rst.raw : rst.quantised);
    }
    if (at != pay_bytes) return fail(c, VQHIP_ERR_DEVICE, "compress_file_residual: records do not fill the payload");
    rst.payload_bytes += pay_bytes;
    if (!out.rec.empty()) out.put(out.rec.data(), out.rec.size());
    return VQHIP_OK;
}

// Replaces the body of VQVAECodec::compress (VQVAECodec.cpp:78-134): gather the leaf buffers into pinned memory,
// encode on the GPU, frame {origin, 64 indices} records and append them to the file while the next batch encodes.
//
// residual_path, res_version 1 (vqhip_compress_file_bounded; NULL, 0 without a sidecar): bd_stage also decodes and measures every
// chunk; the leaves with !(max error <= tol) go raw, from the caller's leaf buffers, into a .vqres sidecar (vqvdb_hip_bounded.h).
// The .vqvdb bytes are the same either way.  res_version 2 (vqhip_compress_file_residual): rs_encode_stage also classes and packs
// the measured chunk and the sidecar holds each selected leaf's record, quantised or raw (.vqres v2, vqvdb_hip_residual.h).
int compress_file_impl(vqhip_codec* c, const char* path, const char* residual_path, int res_version, const vqhip_grid_source* grids, int n_grids,
                       int64_t batch_leaves, float tol, vqhip_stream_stats* stats, vqhip_bounded_stats* bstats, vqhip_residual_stats* rstats)
{
    if (n_grids < 1 || n_grids > 255) return fail(c, VQHIP_ERR_INVALID, "compress_file: a .vqvdb file holds 1..255 grids");
    for (int g = 0; g < n_grids; ++g) {
        const vqhip_grid_source& G = grids[g];
        if (!G.name || G.n_leaves < 0 || G.n_leaves > 0xFFFFFFFFll || (G.n_leaves > 0 && (!G.leaf_ptrs || !G.origins)))
            return fail(c, VQHIP_ERR_INVALID, "compress_file: grid " + std::to_string(g) + " has no name, no leaves/origins or more than 2^32-1 leaves");
    }
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(c, VQHIP_ERR_INVALID, std::string("Cannot open output file: ") + path);
    FileCloser closer{f};
    FILE* fr = nullptr;
    if (residual_path) {
        if (!(fr = std::fopen(residual_path, "wb"))) return fail(c, VQHIP_ERR_INVALID, std::string("Cannot open residual file: ") + residual_path);
    }
    FileCloser rcloser{fr};
    const bool v2 = fr && res_version == 2;
    const PipeStage stage = v2 ? rs_encode_stage(c, tol) : fr ? bd_stage(c) : PipeStage{};
    SidecarOut side{fr};
    vqhip_residual_stats rst;
    std::memset(&rst, 0, sizeof rst);
    const double t_start = now_s();
    vqhip_stream_stats st;
    std::memset(&st, 0, sizeof st);
    bool wfail = false;
    auto put = [&](const void* p, size_t n) {
        if (n && std::fwrite(p, 1, n, f) != n) wfail = true;
    };
    if (fr) {
        unsigned char rh[11];
        std::memcpy(rh, "VQRES", 5);
        rh[5] = (unsigned char)res_version;
        rh[6] = (unsigned char)n_grids;
        std::memcpy(rh + 7, &tol, 4);
        side.put(rh, 11);
    }
    unsigned char h[12];
    std::memcpy(h, "VQVDB", 5);
    h[5] = 3;
    h[6] = (unsigned char)n_grids;
    const uint32_t num_emb = 256;
    std::memcpy(h + 7, &num_emb, 4);
    h[11] = 3;
    put(h, 12);
    std::vector<unsigned char> rec;
    for (int g = 0; g < n_grids; ++g) {
        const vqhip_grid_source& G = grids[g];
        static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const uint32_t name_len = (uint32_t)std::strlen(G.name), total = (uint32_t)G.n_leaves;
        const uint16_t shp[3] = {4, 4, 4};
        put(&name_len, 4);
        put(G.name, name_len);
        put(G.transform ? G.transform : ident, 64);
        put(shp, 6);
        put(&total, 4);
        ++st.grids;
        if (wfail) return fail(c, VQHIP_ERR_INVALID, "Failed to write to .vqvdb file.");
        if (fr && !side.begin_grid()) return fail(c, VQHIP_ERR_INVALID, "Failed to write to residual file.");
        if (G.n_leaves == 0) continue;
        double copy_s = 0, write_s = 0;
        const int rc = run_pipeline(
            c, true, G.n_leaves, batch_leaves, true,
            [&](int64_t o, int64_t m, void* stage) -> const void* {
                const double t = now_s();
                gather_leaves(static_cast<float*>(stage), G.leaf_ptrs + o, m);
                copy_s += now_s() - t;
                return stage;
            },
            [&](const PipeChunk& ch) -> int {
                const double t = now_s();
                rec.resize((size_t)ch.m * REC_BYTES);
                const uint8_t* idx = static_cast<const uint8_t*>(ch.result);
                unsigned char* p = rec.data();
                for (int64_t l = 0; l < ch.m; ++l, p += REC_BYTES) {
                    std::memcpy(p, G.origins + 3 * (ch.o + l), 12);
                    std::memcpy(p + 12, idx + 64 * l, 64);
                }
                put(rec.data(), rec.size());
                if (v2) {
                    if (int src = write_sidecar_v2(c, side, ch, c->bd_pin_err[ch.slot], rst)) return src;
                } else if (fr) {
                    write_sidecar_v1(side, ch, c->bd_pin_err[ch.slot], G.leaf_ptrs, tol);
                }
                write_s += now_s() - t;
                if (side.failed) return fail(c, VQHIP_ERR_INVALID, "Failed to write to residual file.");
                return wfail ? fail(c, VQHIP_ERR_INVALID, "Failed to write to .vqvdb file.") : VQHIP_OK;
            },
            &stage, VQHIP_PRECISION_FP32,
            // the plain compress follows the handle's encode mode; a sidecar's records belong to the fp32 encode's indices
            fr ? VQHIP_PRECISION_FP32 : c->encode_precision);
        if (rc) return rc;
        if (fr && !side.end_grid()) return fail(c, VQHIP_ERR_INVALID, "Failed to write to residual file.");
        st.leaves += G.n_leaves;
        st.copy_s += copy_s, st.read_s += write_s;
    }
    closer.f = nullptr;
    if (std::fclose(f) != 0) return fail(c, VQHIP_ERR_INVALID, "Error closing the output file.");
    if (fr) {
        rcloser.f = nullptr;
        if (std::fclose(fr) != 0) return fail(c, VQHIP_ERR_INVALID, "Error closing the residual file.");
    }
    st.wall_s = now_s() - t_start;
    side.bst.leaves = st.leaves;
    if (stats) *stats = st;
    if (bstats) *bstats = side.bst;
    if (rstats) *rstats = rst;
    return VQHIP_OK;
}

}  // namespace

extern "C" {

int vqhip_decompress_file(vqhip_codec* c, const char* path, int64_t batch_leaves, vqhip_grid_begin_fn grid_begin, vqhip_leaf_alloc_fn leaf_alloc,
                          void* user, vqhip_stream_stats* stats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !leaf_alloc) return fail(c, VQHIP_ERR_INVALID, "decompress_file: null path or leaf allocator");
    return decompress_file_impl(c, path, nullptr, 0, batch_leaves, grid_begin, leaf_alloc, user, stats);
}

int vqhip_decompress_file_bounded(vqhip_codec* c, const char* path, const char* residual_path, int64_t batch_leaves, vqhip_grid_begin_fn grid_begin,
                                  vqhip_leaf_alloc_fn leaf_alloc, void* user, vqhip_stream_stats* stats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !residual_path || !leaf_alloc) return fail(c, VQHIP_ERR_INVALID, "decompress_file_bounded: null path, residual path or leaf allocator");
    return decompress_file_impl(c, path, residual_path, 1, batch_leaves, grid_begin, leaf_alloc, user, stats);
}

int vqhip_compress_file(vqhip_codec* c, const char* path, const vqhip_grid_source* grids, int n_grids, int64_t batch_leaves, vqhip_stream_stats* stats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !grids) return fail(c, VQHIP_ERR_INVALID, "compress_file: null path or grid list");
    return compress_file_impl(c, path, nullptr, 0, grids, n_grids, batch_leaves, 0.0f, stats, nullptr, nullptr);
}

int vqhip_compress_file_bounded(vqhip_codec* c, const char* path, const char* residual_path, const vqhip_grid_source* grids, int n_grids,
                                int64_t batch_leaves, float tol, vqhip_stream_stats* stats, vqhip_bounded_stats* bstats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !residual_path || !grids) return fail(c, VQHIP_ERR_INVALID, "compress_file_bounded: null path, residual path or grid list");
    return compress_file_impl(c, path, residual_path, 1, grids, n_grids, batch_leaves, tol, stats, bstats, nullptr);
}

int vqhip_compress_file_residual(vqhip_codec* c, const char* path, const char* residual_path, const vqhip_grid_source* grids, int n_grids,
                                 int64_t batch_leaves, float tol, vqhip_stream_stats* stats, vqhip_bounded_stats* bstats, vqhip_residual_stats* rstats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !residual_path || !grids) return fail(c, VQHIP_ERR_INVALID, "compress_file_residual: null path, residual path or grid list");
    return compress_file_impl(c, path, residual_path, 2, grids, n_grids, batch_leaves, tol, stats, bstats, rstats);
}

int vqhip_decompress_file_residual(vqhip_codec* c, const char* path, const char* residual_path, int64_t batch_leaves, vqhip_grid_begin_fn grid_begin,
                                   vqhip_leaf_alloc_fn leaf_alloc, void* user, vqhip_stream_stats* stats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !residual_path || !leaf_alloc) return fail(c, VQHIP_ERR_INVALID, "decompress_file_residual: null path, residual path or leaf allocator");
    return decompress_file_impl(c, path, residual_path, 2, batch_leaves, grid_begin, leaf_alloc, user, stats);
}

}  // extern "C"
