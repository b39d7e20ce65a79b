// vq_residual.inc — runtime of the scalar handle's quantised residuals (vqhip_residual_encode_device, _apply_device,
// _compress_residual, _decompress_residual and the file pair; include/vqvdb_hip_residual.h, DESIGN.md §17).  Part of
// vq_runtime.hip's translation unit, after vq_bounded.inc: the round trip and its leaf errors are that file's, unchanged; the
// four kernels of vq_residual.h (C = 1) follow them.  The file pair runs compress_file_impl / decompress_file_impl of vq_file.inc,
// which hang rs_encode_stage / rs_decode_stage below behind every chunk of the host pipeline.

#include "../../include/vqvdb_hip_residual.h"
#include "vq_residual.h"

static_assert(VQHIP_RES_KEPT == vqr::Format<1>::KEPT && VQHIP_RES_RAW == vqr::Format<1>::RAW, "the header's classes are the kernels'");

namespace {

inline unsigned rs_grid(int64_t n)
{
    return (unsigned)((n + vqr::RES_WAVES - 1) / vqr::RES_WAVES);
}

// class, scan, pack of n leaves: d_off[n] ends as the payload's size
int rs_encode(vqhip_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, float tol, uint8_t* d_class, int64_t* d_off,
              uint8_t* d_payload, int64_t capacity, hipStream_t s)
{
    Launcher L{c, s, n};
    L.run("residual_class", [&] {
        hipLaunchKernelGGL(vqr::resid_class_k<1>, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, d_err, n, tol, d_class, d_off);
    });
    L.run("residual_scan", [&] { hipLaunchKernelGGL(vqr::resid_scan_k, dim3(1), dim3(1024), 0, s, d_off, n); });
    L.run("residual_pack", [&] {
        hipLaunchKernelGGL(vqr::resid_pack_k<1>, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, d_recon, n, tol, d_class, d_off, d_payload,
                           capacity);
    });
    return L.rc;
}

int rs_apply(vqhip_codec* c, float* d_leaves, int64_t n, float tol, const uint8_t* d_class, const int64_t* d_off, const uint8_t* d_payload, hipStream_t s)
{
    Launcher L{c, s, n};
    L.run("residual_apply", [&] {
        hipLaunchKernelGGL(vqr::resid_apply_k<1>, dim3(rs_grid(n)), dim3(64 * vqr::RES_WAVES), 0, s, d_leaves, n, tol, d_class, d_off, d_payload);
    });
    return L.rc;
}

// per I/O slot the classes, offsets and payload of m leaves on the device; `pinned`: also a pinned block per slot that holds
// {int64 total | m + 1 offsets | m * 2048 payload bytes | m classes} (the file pair's landing zone and upload staging)
int rs_ensure(vqhip_codec* c, int64_t m, bool pinned)
{
    for (int i = 0; i < 2; ++i) {
        if (int rc = ensure(c, c->rs_class[i], (size_t)m, "the residual classes")) return rc;
        if (int rc = ensure(c, c->rs_off[i], (size_t)m + 1, "the residual offsets")) return rc;
        if (int rc = ensure(c, c->rs_payload[i], (size_t)m * 2048, "the residual payload")) return rc;
    }
    if (pinned && c->rs_pin_leaves < m) {
        for (int i = 0; i < 2; ++i)
            if (int rc = ensure(c, c->rs_pin[i], (size_t)m * (8 + 2048 + 1) + 16, "the pinned residual block")) {
                if (!c->rs_pin[i]) c->rs_pin_leaves = 0;   // (a failed synchronise leaves the old blocks and their layout)
                return rc;
            }
        c->rs_pin_leaves = m;
    }
    return VQHIP_OK;
}

int64_t* rs_pin_off(vqhip_codec* c, int slot) { return reinterpret_cast<int64_t*>(c->rs_pin[slot].get()) + 1; }
unsigned char* rs_pin_payload(vqhip_codec* c, int slot) { return c->rs_pin[slot] + (size_t)(c->rs_pin_leaves + 2) * 8; }
unsigned char* rs_pin_class(vqhip_codec* c, int slot) { return rs_pin_payload(c, slot) + (size_t)c->rs_pin_leaves * 2048; }

// a residual file compress: the bounded stage, then the measured chunk is classed, placed and packed into the slot's payload
// buffer; its total and classes travel to the pinned block behind the leaf errors, and the consumer fetches the payload
PipeStage rs_encode_stage(vqhip_codec* c, float tol)
{
    const PipeStage bd = bd_stage(c);
    return {[=](int64_t step) {
                const int rc = bd.ensure(step);
                return rc ? rc : rs_ensure(c, step, true);
            },
            [=](int64_t o, int64_t m, int slot, hipStream_t s) {
                const int rc = bd.device(o, m, slot, s);
                return rc ? rc : rs_encode(c, c->dev_leaves[slot], c->bd_recon, c->bd_err[slot], m, tol, c->rs_class[slot], c->rs_off[slot],
                                           c->rs_payload[slot], m * 2048, s);
            },
            [=](int64_t m, int slot, hipStream_t s) {
                hipError_t e = bd.copy_out(m, slot, s);
                if (e == hipSuccess) e = hipMemcpyAsync(c->rs_pin[slot], c->rs_off[slot] + m, sizeof(int64_t), hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipMemcpyAsync(rs_pin_class(c, slot), c->rs_class[slot], (size_t)m, hipMemcpyDeviceToHost, s);
                return e;
            }};
}

// the consumer of a residual file compress: the chunk's payload, now that its total is known.  The slot's device buffer is
// not written again before the consumer returns, and the chunk's idle stream carries the copy.
int rs_fetch_payload(vqhip_codec* c, const PipeChunk& ch, const unsigned char** payload, int64_t* total)
{
    std::memcpy(total, c->rs_pin[ch.slot], sizeof(int64_t));
    if (*total < 0 || *total > ch.m * 2048) return fail(c, VQHIP_ERR_DEVICE, "compress_file_residual: payload size out of range");
    *payload = rs_pin_payload(c, ch.slot);
    if (*total == 0) return VQHIP_OK;
    HIPCHK(c, hipMemcpyAsync(rs_pin_payload(c, ch.slot), c->rs_payload[ch.slot], (size_t)*total, hipMemcpyDeviceToHost, ch.idle));
    HIPCHK(c, hipStreamSynchronize(ch.idle));
    return VQHIP_OK;
}

// a residual file decompress: the slot's pinned block holds the chunk's classes and, in leaf order, its records; place them,
// upload all three and apply them to the decoded chunk on stream s.  The block is not written again before that work is done.
int rs_upload_apply(vqhip_codec* c, int64_t m, float tol, int slot, hipStream_t s)
{
    const unsigned char* cls = rs_pin_class(c, slot);
    int64_t* off = rs_pin_off(c, slot);
    off[0] = 0;
    for (int64_t i = 0; i < m; ++i) off[i + 1] = off[i] + vqr::record_size<1>(cls[i]);
    const int64_t total = off[m];
    HIPCHK(c, hipMemcpyAsync(c->rs_class[slot], rs_pin_class(c, slot), (size_t)m, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->rs_off[slot], rs_pin_off(c, slot), (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (total > 0) HIPCHK(c, hipMemcpyAsync(c->rs_payload[slot], rs_pin_payload(c, slot), (size_t)total, hipMemcpyHostToDevice, s));
    return rs_apply(c, c->dev_leaves[slot], m, tol, c->rs_class[slot], c->rs_off[slot], c->rs_payload[slot], s);
}

// Forward reader of one grid's entries in a .vqres sidecar: {u32 index | v2: u8 class | record}, indices ascending within the
// grid of n leaves (v1, vqvdb_hip_bounded.h: every record a raw leaf; v2: vqvdb_hip_residual.h).  The file pair's decompress
// walks it in step with the chunks: an entry whose header is read but whose leaf lies in a later chunk stays pending.
struct ResidualWalk {
    vqhip_codec* c;
    FILE* fr;
    bool v2;
    const std::string& name;
    int64_t n;
    int64_t left = 0, pending = -1, prev = -1;   // entries still to take, the index read ahead (-1: none), the last one taken
    int cls = VQHIP_RES_RAW;                     // the class read with `pending`

    // every entry of chunk [o, o + m), in order: dst(leaf within the chunk, class) is where its record goes
    template <typename Dst>
    int read_chunk(int64_t o, int64_t m, Dst&& dst)
    {
        while (left > 0) {
            if (pending < 0) {
                unsigned char eh[5];
                const size_t hb = v2 ? 5 : 4;
                uint32_t ri = 0;
                if (std::fread(eh, 1, hb, fr) != hb) return fail(c, VQHIP_ERR_INVALID, "Residual file truncated: incomplete leaf entry.");
                std::memcpy(&ri, eh, 4);
                if ((int64_t)ri >= n)
                    return fail(c, VQHIP_ERR_INVALID, "residual file: record index " + std::to_string(ri) + " in grid '" + name + "' of " + std::to_string(n) + " leaves");
                if ((int64_t)ri <= prev)
                    return fail(c, VQHIP_ERR_INVALID, "residual file: record index " + std::to_string(ri) + " in grid '" + name + "' is not ascending");
                if (v2 && eh[4] > 16 && eh[4] != VQHIP_RES_RAW)
                    return fail(c, VQHIP_ERR_INVALID, "residual file: class " + std::to_string((int)eh[4]) + " of record " + std::to_string(ri) + " in grid '" + name +
                                                          "' is not 0..16 or 255");
                pending = ri;
                if (v2) cls = eh[4];
            }
            if (pending >= o + m) break;   // a later chunk's leaf (earlier ones went with their chunk: pending >= o)
            const size_t sz = (size_t)vqr::record_size<1>(cls);
            void* to = dst(pending - o, cls);   // also for a class of no bytes
            if (sz && std::fread(to, 1, sz, fr) != sz) return fail(c, VQHIP_ERR_INVALID, "Residual file truncated: incomplete leaf entry.");
            prev = pending, pending = -1, --left;
        }
        return VQHIP_OK;
    }
};

// a residual file decompress (.vqres v2), behind the decode of the slot's chunk on stream s: the chunk's records are read forward
// into the slot's pinned block, uploaded and applied before the chunk leaves the GPU.  *walk outlives the pipeline run.
PipeStage rs_decode_stage(vqhip_codec* c, float tol, ResidualWalk* walk)
{
    return {[c](int64_t step) { return rs_ensure(c, step, true); },
            [c, tol, walk](int64_t o, int64_t m, int slot, hipStream_t s) {
                unsigned char* cls = rs_pin_class(c, slot);
                unsigned char* pay = rs_pin_payload(c, slot);
                bool any = false;
                const int rc = walk->read_chunk(o, m, [&](int64_t l, int k) {
                    if (!any) std::memset(cls, VQHIP_RES_KEPT, (size_t)m), any = true;
                    cls[l] = (unsigned char)k;
                    unsigned char* at = pay;
                    pay += vqr::record_size<1>(k);
                    return at;
                });
                return rc || !any ? rc : rs_upload_apply(c, m, tol, slot, s);
            },
            nullptr};
}

}  // namespace

extern "C" {

int vqhip_residual_encode_device(vqhip_codec* c, const float* d_leaves, const float* d_recon, const float* d_err, int64_t n, float tol, uint8_t* d_class,
                                 int64_t* d_off, uint8_t* d_payload, int64_t capacity, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "residual_encode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (capacity < 0) return fail(c, VQHIP_ERR_INVALID, "residual_encode: payload_capacity < 0");
    if (!d_leaves || !d_recon || !d_err || !d_class || !d_off || (!d_payload && capacity > 0)) return fail(c, VQHIP_ERR_INVALID, "residual_encode: null pointer");
    if (n > (int64_t(1) << 32)) return fail(c, VQHIP_ERR_INVALID, "residual_encode: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return rs_encode(c, d_leaves, d_recon, d_err, n, tol, d_class, d_off, d_payload, capacity, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_residual_apply_device(vqhip_codec* c, float* d_leaves, int64_t n, float tol, const uint8_t* d_class, const int64_t* d_off,
                                const uint8_t* d_payload, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "residual_apply: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_class || !d_off) return fail(c, VQHIP_ERR_INVALID, "residual_apply: null pointer");
    if (n > (int64_t(1) << 32)) return fail(c, VQHIP_ERR_INVALID, "residual_apply: n_leaves exceeds 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    return rs_apply(c, d_leaves, n, tol, d_class, d_off, d_payload, stream ? (hipStream_t)stream : c->stream);
}

int vqhip_compress_residual(vqhip_codec* c, const float* leaves, int64_t n, float tol, uint8_t* indices, float* leaf_err, uint8_t* leaf_class,
                            uint8_t* payload, int64_t* payload_bytes)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return fail(c, VQHIP_ERR_INVALID, "compress_residual: n_leaves < 0");
    if (!payload_bytes) return fail(c, VQHIP_ERR_INVALID, "compress_residual: payload_bytes is NULL");
    *payload_bytes = 0;
    if (n == 0) return VQHIP_OK;
    if (!leaves || !indices || !leaf_class || !payload) return fail(c, VQHIP_ERR_INVALID, "compress_residual: null pointer");
    if (int rc = bd_prepare(c)) return rc;
    int64_t total = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = ensure_io(c, m)) return rc;
        if (int rc = bd_ensure_pipe(c, m)) return rc;
        if (int rc = rs_ensure(c, m, false)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->dev_leaves[0], leaves + o * 512, (size_t)m * 2048, hipMemcpyHostToDevice, c->stream));
        int rc = bd_roundtrip_chunk(c, c->dev_leaves[0], m, c->dev_idx[0], nullptr, c->bd_err[0], c->stream);
        if (!rc) rc = rs_encode(c, c->dev_leaves[0], c->bd_recon, c->bd_err[0], m, tol, c->rs_class[0], c->rs_off[0], c->rs_payload[0], m * 2048, c->stream);
        if (rc) {
            hipStreamSynchronize(c->stream);   // the copy above may still read the caller's leaves
            return rc;
        }
        HIPCHK(c, hipMemcpyAsync(indices + o * 64, c->dev_idx[0], (size_t)m * 64, hipMemcpyDeviceToHost, c->stream));
        if (leaf_err)
            HIPCHK(c, hipMemcpyAsync(leaf_err + o * VQHIP_ERR_FLOATS, c->bd_err[0], (size_t)m * VQHIP_ERR_FLOATS * sizeof(float), hipMemcpyDeviceToHost,
                                     c->stream));
        HIPCHK(c, hipMemcpyAsync(leaf_class + o, c->rs_class[0], (size_t)m, hipMemcpyDeviceToHost, c->stream));
        int64_t bytes = 0;
        HIPCHK(c, hipMemcpyAsync(&bytes, c->rs_off[0] + m, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (bytes < 0 || bytes > m * 2048) return fail(c, VQHIP_ERR_DEVICE, "compress_residual: payload size out of range");
        if (bytes > 0) HIPCHK(c, hipMemcpy(payload + total, c->rs_payload[0], (size_t)bytes, hipMemcpyDeviceToHost));
        total += bytes;
    }
    *payload_bytes = total;
    return VQHIP_OK;
}

int vqhip_decompress_residual(vqhip_codec* c, const uint8_t* indices, int64_t n, float tol, const uint8_t* leaf_class, const uint8_t* payload,
                              int64_t payload_bytes, float* leaves)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0 || payload_bytes < 0) return fail(c, VQHIP_ERR_INVALID, "decompress_residual: n_leaves < 0 or payload_bytes < 0");
    if (n == 0) return VQHIP_OK;
    if (!indices || !leaves || !leaf_class || (payload_bytes > 0 && !payload)) return fail(c, VQHIP_ERR_INVALID, "decompress_residual: null pointer");
    int64_t need = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!vqr::code_ok<1>(leaf_class[i]))
            return fail(c, VQHIP_ERR_INVALID, "decompress_residual: class " + std::to_string((int)leaf_class[i]) + " of leaf " + std::to_string(i) +
                                                  " is not 0..16, 254 or 255");
        need += vqr::record_size<1>(leaf_class[i]);
    }
    if (need != payload_bytes)
        return fail(c, VQHIP_ERR_INVALID, "decompress_residual: the classes need " + std::to_string(need) + " payload bytes, the caller gives " +
                                              std::to_string(payload_bytes));
    if (int rc = bd_prepare(c)) return rc;
    std::vector<int64_t> off;
    int64_t at = 0;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        if (int rc = ensure_io(c, m)) return rc;
        if (int rc = rs_ensure(c, m, false)) return rc;
        off.resize((size_t)m + 1);
        off[0] = 0;
        for (int64_t i = 0; i < m; ++i) off[i + 1] = off[i] + vqr::record_size<1>(leaf_class[o + i]);
        HIPCHK(c, hipMemcpy(c->dev_idx[0], indices + o * 64, (size_t)m * 64, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->rs_class[0], leaf_class + o, (size_t)m, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->rs_off[0], off.data(), (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        if (off[m] > 0) HIPCHK(c, hipMemcpy(c->rs_payload[0], payload + at, (size_t)off[m], hipMemcpyHostToDevice));
        at += off[m];
        if (int rc = decode_chunk(c, c->dev_idx[0], m, c->dev_leaves[0], c->stream)) return rc;
        if (int rc = rs_apply(c, c->dev_leaves[0], m, tol, c->rs_class[0], c->rs_off[0], c->rs_payload[0], c->stream)) return rc;
        HIPCHK(c, hipMemcpyAsync(leaves + o * 512, c->dev_leaves[0], (size_t)m * 2048, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VQHIP_OK;
}

}  // extern "C"
