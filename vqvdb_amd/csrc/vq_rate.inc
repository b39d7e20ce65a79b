// vq_rate.inc — runtime of the scalar handle's size sweep (vqhip_rate_sweep_device, _sweep, _sweep_file, _compress_file and the
// two size helpers; include/vqvdb_hip_rate.h, DESIGN.md §19).  Part of vq_runtime.hip's translation unit, after vq_file.inc: the
// round trip is vq_bounded.inc's, the file pipeline and compress_file_impl are vq_file.inc's, all unchanged; sweep_k<1> of vq_rate.h
// follows the round trip of every chunk and adds to one histogram that stays on the device until the call's end.  The helpers that
// do not depend on the handle (rate_tols, rate_check_count, rate_check_tols, rate_payload, rate_pick) also serve vq_vec3_rate.inc.

#include "../../include/vqvdb_hip_rate.h"
#include "vq_rate.h"

static_assert(VQHIP_RATE_MAX_TOLS == vqrate::RATE_MAX_TOLS && VQHIP_RATE_CLASSES == vqrate::CLASSES<1>, "the header's table is the kernel's");

namespace {

constexpr size_t RATE_HIST_BYTES = (size_t)VQHIP_RATE_MAX_TOLS * VQHIP_RATE_CLASSES * sizeof(int64_t);

// the payload of a compress whose histogram row this is: C channels per voxel
template <int C>
inline int64_t rate_payload(const int64_t* row)
{
    int64_t s = 2048 * C * row[vqrate::COL_RAW<C>];
    for (int b = 0; b < vqrate::COL_RAW<C>; ++b) s += 64 * (int64_t)b * row[b];
    return s;
}

inline int64_t rate_selected(const int64_t* row)
{
    int64_t s = 0;
    for (int b = 0; b <= vqrate::COL_RAW<1>; ++b) s += row[b];
    return s;
}

inline int64_t rate_sidecar(const int64_t* row, int n_grids)
{
    return 11 + 4 * (int64_t)n_grids + 5 * rate_selected(row) + rate_payload<1>(row);
}

// the smallest rung by value whose row of hist [n_tols][16 C + 3] has a size within the budget; no order of the rungs and no
// monotone sizes are assumed, NaN never compares as smaller.  *smallest: the smallest size of the rungs that are not NaN, -1 if
// there is none
template <int C, typename Size>
int rate_pick(const int64_t* hist, const float* tols, int n_tols, int64_t budget, Size size_of_row, int64_t* smallest)
{
    int best = -1;
    int64_t least = -1;
    for (int t = 0; t < n_tols; ++t) {
        if (tols[t] != tols[t]) continue;
        const int64_t bytes = size_of_row(hist + (size_t)t * vqrate::CLASSES<C>);
        if (least < 0 || bytes < least) least = bytes;
        if (bytes <= budget && (best < 0 || tols[t] < tols[best])) best = t;
    }
    if (smallest) *smallest = least;
    return best;
}

inline int fail(vqhip_vec3_codec* c, int code, const std::string& msg) { return v3_fail(c, code, msg); }

template <typename Handle>
int rate_check_count(Handle* c, const char* what, int n_tols)
{
    if (n_tols < 1 || n_tols > vqrate::RATE_MAX_TOLS)
        return fail(c, VQHIP_ERR_INVALID, std::string(what) + ": n_tols " + std::to_string(n_tols) + " is not in 1.." + std::to_string(vqrate::RATE_MAX_TOLS));
    return VQHIP_OK;
}

template <typename Handle>
int rate_check_tols(Handle* c, const char* what, const float* tols, int n_tols)
{
    if (int rc = rate_check_count(c, what, n_tols)) return rc;
    return tols ? VQHIP_OK : fail(c, VQHIP_ERR_INVALID, std::string(what) + ": tols is NULL");
}

vqrate::Tols rate_tols(const float* tols, int n_tols)
{
    vqrate::Tols T;
    std::memset(&T, 0, sizeof T);
    T.count = n_tols;
    std::memcpy(T.t, tols, (size_t)n_tols * sizeof(float));
    return T;
}

// the histogram of n leaves added to d_hist
int rate_sweep(vqhip_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, const vqrate::Tols& T, int64_t* d_hist,
               hipStream_t s)
{
    const unsigned grid = (unsigned)std::min<int64_t>((n + vqrate::RATE_WAVES - 1) / vqrate::RATE_WAVES, vqrate::RATE_MAX_GRID);
    Launcher L{c, s, n};
    L.run("rate_sweep", [&] {
        hipLaunchKernelGGL(vqrate::sweep_k<1>, dim3(grid), dim3(64 * vqrate::RATE_WAVES), 0, s, d_leaves, d_recon, d_err, n, T,
                           reinterpret_cast<unsigned long long*>(d_hist));
    });
    return L.rc;
}

// the handle's histogram, cleared on the compute stream
int rate_begin(vqhip_codec* c)
{
    if (int rc = ensure(c, c->rate_hist, RATE_HIST_BYTES / sizeof(int64_t), "the size-sweep histogram")) return rc;
    HIPCHK(c, hipMemsetAsync(c->rate_hist, 0, RATE_HIST_BYTES, c->stream));
    return VQHIP_OK;
}

// ... and read back behind everything the compute stream holds
int rate_end(vqhip_codec* c, int n_tols, int64_t* hist)
{
    HIPCHK(c, hipMemcpyAsync(hist, c->rate_hist, (size_t)n_tols * VQHIP_RATE_CLASSES * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

// a sweep over a file compress's grids: the bounded stage decodes and measures every chunk, the sweep follows on the chunk's stream;
// nothing of the stage travels back per chunk
PipeStage rate_stage(vqhip_codec* c, const vqrate::Tols& T)
{
    const PipeStage bd = bd_stage(c);
    return {bd.ensure,
            [=](int64_t o, int64_t m, int slot, hipStream_t s) {
                const int rc = bd.device(o, m, slot, s);
                return rc ? rc : rate_sweep(c, c->dev_leaves[slot], c->bd_recon, c->bd_err[slot], m, T, c->rate_hist, s);
            },
            nullptr};
}

// vqhip_compress_file's pipeline with rate_stage behind every chunk and a consumer that writes nothing: no file is opened
int sweep_file_impl(vqhip_codec* c, const vqhip_grid_source* grids, int n_grids, int64_t batch_leaves, const float* tols, int n_tols, int64_t* hist,
                    vqhip_stream_stats* stats)
{
    if (n_grids < 1 || n_grids > 255) return fail(c, VQHIP_ERR_INVALID, "rate_sweep_file: a .vqvdb file holds 1..255 grids");
    for (int g = 0; g < n_grids; ++g) {
        const vqhip_grid_source& G = grids[g];
        if (!G.name || G.n_leaves < 0 || G.n_leaves > 0xFFFFFFFFll || (G.n_leaves > 0 && (!G.leaf_ptrs || !G.origins)))
            return fail(c, VQHIP_ERR_INVALID, "rate_sweep_file: grid " + std::to_string(g) + " has no name, no leaves/origins or more than 2^32-1 leaves");
    }
    if (int rc = bd_prepare(c)) return rc;
    if (int rc = rate_begin(c)) return rc;
    const vqrate::Tols T = rate_tols(tols, n_tols);
    const PipeStage stage = rate_stage(c, T);
    const double t_start = now_s();
    vqhip_stream_stats st;
    std::memset(&st, 0, sizeof st);
    for (int g = 0; g < n_grids; ++g) {
        const vqhip_grid_source& G = grids[g];
        ++st.grids;
        if (G.n_leaves == 0) continue;
        double copy_s = 0;
        const int rc = run_pipeline(
            c, true, G.n_leaves, batch_leaves, true,
            [&](int64_t o, int64_t m, void* stage_buf) -> const void* {
                const double t = now_s();
                gather_leaves(static_cast<float*>(stage_buf), G.leaf_ptrs + o, m);
                copy_s += now_s() - t;
                return stage_buf;
            },
            [](const PipeChunk&) -> int { return VQHIP_OK; }, &stage);
        if (rc) return rc;
        st.leaves += G.n_leaves;
        st.copy_s += copy_s;
    }
    if (int rc = rate_end(c, n_tols, hist)) return rc;
    st.wall_s = now_s() - t_start;
    if (stats) *stats = st;
    return VQHIP_OK;
}

}  // namespace

extern "C" {

int64_t vqhip_rate_payload_bytes(const int64_t* hist_row)
{
    return hist_row ? rate_payload<1>(hist_row) : -1;
}

int64_t vqhip_rate_sidecar_bytes(const int64_t* hist_row, int n_grids)
{
    return hist_row ? rate_sidecar(hist_row, n_grids) : -1;
}

int vqhip_rate_sweep_device(vqhip_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, const float* tols, int n_tols,
                            int64_t* d_hist, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "rate_sweep: n_leaves < 0");
    if (int rc = rate_check_count(c, "rate_sweep", n_tols)) return rc;
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_recon || !d_err || !tols || !d_hist) return fail(c, VQHIP_ERR_INVALID, "rate_sweep: null pointer");
    if (n > (int64_t(1) << 32)) return fail(c, VQHIP_ERR_INVALID, "rate_sweep: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return rate_sweep(c, d_leaves, d_recon, d_err, n, rate_tols(tols, n_tols), d_hist, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_rate_sweep(vqhip_codec* c, const float* leaves, int64_t n, const float* tols, int n_tols, int64_t* hist)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "rate_sweep: n_leaves < 0");
    if (int rc = rate_check_tols(c, "rate_sweep", tols, n_tols)) return rc;
    if (!hist) return fail(c, VQHIP_ERR_INVALID, "rate_sweep: hist is NULL");
    std::memset(hist, 0, (size_t)n_tols * VQHIP_RATE_CLASSES * sizeof(int64_t));
    if (n == 0) return VQHIP_OK;
    if (!leaves) return fail(c, VQHIP_ERR_INVALID, "rate_sweep: null pointer");
    if (int rc = bd_prepare(c)) return rc;
    if (int rc = rate_begin(c)) return rc;
    const vqrate::Tols T = rate_tols(tols, n_tols);
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = ensure_io(c, m)) return rc;
        if (int rc = bd_ensure_pipe(c, m)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->dev_leaves[0], leaves + o * 512, (size_t)m * 2048, hipMemcpyHostToDevice, c->stream));
        int rc = bd_roundtrip_chunk(c, c->dev_leaves[0], m, c->dev_idx[0], nullptr, c->bd_err[0], c->stream);
        if (!rc) rc = rate_sweep(c, c->dev_leaves[0], c->bd_recon, c->bd_err[0], m, T, c->rate_hist, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copy above may still read the caller's leaves
            return rc;
        }
    }
    return rate_end(c, n_tols, hist);
}

int vqhip_rate_sweep_file(vqhip_codec* c, const vqhip_grid_source* grids, int n_grids, int64_t batch_leaves, const float* tols, int n_tols, int64_t* hist,
                          vqhip_stream_stats* stats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!grids || !hist) return fail(c, VQHIP_ERR_INVALID, "rate_sweep_file: null grid list or histogram");
    if (int rc = rate_check_tols(c, "rate_sweep_file", tols, n_tols)) return rc;
    return sweep_file_impl(c, grids, n_grids, batch_leaves, tols, n_tols, hist, stats);
}

int vqhip_rate_compress_file(vqhip_codec* c, const char* path, const char* residual_path, const vqhip_grid_source* grids, int n_grids, int64_t batch_leaves,
                             const float* tols, int n_tols, int64_t sidecar_budget, float* tol_used, int64_t* hist, vqhip_stream_stats* stats,
                             vqhip_bounded_stats* bstats, vqhip_residual_stats* rstats)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!path || !residual_path || !grids || !tol_used) return fail(c, VQHIP_ERR_INVALID, "rate_compress_file: null path, residual path, grid list or tol_used");
    if (sidecar_budget < 0) return fail(c, VQHIP_ERR_INVALID, "rate_compress_file: sidecar_budget < 0");
    if (int rc = rate_check_tols(c, "rate_compress_file", tols, n_tols)) return rc;
    int64_t table[VQHIP_RATE_MAX_TOLS * VQHIP_RATE_CLASSES];
    if (int rc = sweep_file_impl(c, grids, n_grids, batch_leaves, tols, n_tols, table, nullptr)) return rc;
    if (hist) std::memcpy(hist, table, (size_t)n_tols * VQHIP_RATE_CLASSES * sizeof(int64_t));
    int64_t smallest = -1;
    const int best = rate_pick<1>(table, tols, n_tols, sidecar_budget, [&](const int64_t* row) { return rate_sidecar(row, n_grids); }, &smallest);
    if (best < 0) {
        if (smallest < 0) return fail(c, VQHIP_ERR_INVALID, "rate_compress_file: every rung is NaN, none can be chosen");
        return fail(c, VQHIP_ERR_INVALID, "rate_compress_file: the smallest sidecar of the " + std::to_string(n_tols) + " rungs has " +
                                              std::to_string(smallest) + " bytes, the budget is " + std::to_string(sidecar_budget) + " bytes");
    }
    *tol_used = tols[best];
    return compress_file_impl(c, path, residual_path, 2, grids, n_grids, batch_leaves, tols[best], stats, bstats, rstats);
}

}  // extern "C"
