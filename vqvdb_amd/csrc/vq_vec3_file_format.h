// vq_vec3_file_format.h — the .vqv3 container, version 1, on the host (include/vqvdb_hip_vec3_file.h): emit and
// parse of the file header and of a grid's metadata, the offsets of a grid's sections, the whole-file length check and the
// per-grid checks of indices, codes and record sizes.  vq_vec3_file.inc streams chunks through these; vqvdb_amd/vqvdbfile.py
// restates the layout in numpy.  Includes nothing of the GPU runtime: tests/host/vec3_file_check.cpp builds it alone.
//
// Little endian, no padding (the library runs on little-endian hosts only, like the .vqvdb code beside it):
//   file : char magic[6]="VQVEC3" | u8 version=1 | u8 numGrids (1..255) | u32 numCodes | u8 kind | u8 mode | u16 zero | f32 tol | u32 zero
//   grid : u32 nameLength | name | f32 transform[16] | u16 latentShape[3]={4,4,4} | u32 totalBlocks (n) | u8 hasBackground | u8 zero[3]
//          f32 background[3] | u64 payloadBytes | i32 origins[n][3] | u16 indices[n][64]
//          kind 1 only: u64 masks[n][8] | u16 codes[n] | u8 payload[payloadBytes]
// kind 0: indices only (mode 0, tol +0.0f, payloadBytes 0).  kind 1: masks and the compact records of vqvdb_hip_vec3_active.h;
// mode is the decoder mode the records belong to (0 fp32, 1 bf16).
//
// Every byte read here is untrusted.  Nothing is allocated from a header field before the file's length has vouched for it, and
// every offset is a uint64 sum whose terms are bounded first: a name by the bytes left in the file, 206 * totalBlocks < 2^40,
// payloadBytes by the bytes left behind its grid's fixed sections.
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace vqv3f {

constexpr char MAGIC[7] = "VQVEC3";
constexpr int VERSION = 1;
constexpr uint64_t FILE_HEADER_BYTES = 24;
constexpr uint64_t GRID_FIXED_BYTES = 4 + 64 + 6 + 4 + 4 + 12 + 8;   // a grid's metadata without its name
constexpr int KIND_INDICES = 0, KIND_ACTIVE = 1;
constexpr int CODE_KEPT = 0xFFFE, CODE_RAW = 0xFFFF;                 // VQHIP_VEC3_RES_KEPT, VQHIP_VEC3_RES_RAW

// what a file may hold as a leaf's code: a sentinel, or three widths of 0 .. 16 and nothing above them
inline bool code_ok(int code)
{
    if (code == CODE_KEPT || code == CODE_RAW) return true;
    return (code >> 15) == 0 && (code & 31) <= 16 && ((code >> 5) & 31) <= 16 && ((code >> 10) & 31) <= 16;
}

// vqhip_vec3_active_record_bytes for a legal code and 0 <= active <= 512
inline uint64_t record_bytes(int code, int active)
{
    if (code == CODE_KEPT) return 0;
    if (code == CODE_RAW) return 8 * (uint64_t)((3 * active + 1) / 2);
    return 8 * (uint64_t)((active + 63) / 64) * (uint64_t)((code & 31) + ((code >> 5) & 31) + ((code >> 10) & 31));
}

inline int popcount512(const uint64_t* words)
{
    int a = 0;
    for (int j = 0; j < 8; ++j) a += __builtin_popcountll(words[j]);
    return a;
}

struct Header {
    int n_grids = 0;
    uint32_t num_codes = 0;
    int kind = 0, mode = 0;
    float tol = 0.0f;
};

struct Grid {
    std::string name;
    float transform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    uint32_t total = 0;
    int has_background = 0;
    float background[3] = {0.0f, 0.0f, 0.0f};
    uint64_t payload_bytes = 0;
    // absolute offsets in the file (layout)
    uint64_t meta_at = 0, payload_field_at = 0, origins_at = 0, indices_at = 0, masks_at = 0, codes_at = 0, payload_at = 0, end_at = 0;
};

// a file descriptor with positioned reads and writes
class File {
    int fd_ = -1;

public:
    File() = default;
    File(const File&) = delete;
    File& operator=(const File&) = delete;
    ~File() { close(); }
    bool open_read(const char* path) { return (fd_ = ::open(path, O_RDONLY | O_CLOEXEC)) >= 0; }
    bool open_write(const char* path) { return (fd_ = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644)) >= 0; }
    bool is_open() const { return fd_ >= 0; }
    bool close()
    {
        if (fd_ < 0) return true;
        const int rc = ::close(fd_);
        fd_ = -1;
        return rc == 0;
    }
    bool size(uint64_t& bytes) const
    {
        struct stat st;
        if (::fstat(fd_, &st) != 0 || st.st_size < 0) return false;
        bytes = (uint64_t)st.st_size;
        return true;
    }
    bool read_at(uint64_t at, void* dst, uint64_t n) const
    {
        char* p = static_cast<char*>(dst);
        while (n > 0) {
            const ssize_t r = ::pread(fd_, p, (size_t)std::min<uint64_t>(n, uint64_t(1) << 30), (off_t)at);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) return false;
            p += r, at += (uint64_t)r, n -= (uint64_t)r;
        }
        return true;
    }
    bool write_at(uint64_t at, const void* src, uint64_t n) const
    {
        const char* p = static_cast<const char*>(src);
        while (n > 0) {
            const ssize_t r = ::pwrite(fd_, p, (size_t)std::min<uint64_t>(n, uint64_t(1) << 30), (off_t)at);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) return false;
            p += r, at += (uint64_t)r, n -= (uint64_t)r;
        }
        return true;
    }
};

inline void emit_header(const Header& h, unsigned char out[FILE_HEADER_BYTES])
{
    std::memset(out, 0, FILE_HEADER_BYTES);
    std::memcpy(out, MAGIC, 6);
    out[6] = (unsigned char)VERSION;
    out[7] = (unsigned char)h.n_grids;
    std::memcpy(out + 8, &h.num_codes, 4);
    out[12] = (unsigned char)h.kind;
    out[13] = (unsigned char)h.mode;
    std::memcpy(out + 16, &h.tol, 4);
}

inline bool parse_header(const unsigned char in[FILE_HEADER_BYTES], Header& h, std::string& err)
{
    if (std::memcmp(in, MAGIC, 6) != 0) return err = "Invalid file magic; not a .vqv3 file.", false;
    if (in[6] != VERSION) return err = "Unsupported .vqv3 version " + std::to_string((int)in[6]) + " (expected 1).", false;
    h.n_grids = in[7];
    std::memcpy(&h.num_codes, in + 8, 4);
    h.kind = in[12], h.mode = in[13];
    std::memcpy(&h.tol, in + 16, 4);
    uint32_t tol_bits, zero32;
    std::memcpy(&tol_bits, in + 16, 4);
    std::memcpy(&zero32, in + 20, 4);
    if (h.n_grids < 1) return err = ".vqv3: a file holds 1..255 grids, the header says 0", false;
    if (h.num_codes < 1 || h.num_codes > 65536) return err = ".vqv3: numCodes " + std::to_string(h.num_codes) + " is not in 1..65536", false;
    if (h.kind != KIND_INDICES && h.kind != KIND_ACTIVE) return err = ".vqv3: kind " + std::to_string(h.kind) + " is neither 0 nor 1", false;
    if (h.mode > 1) return err = ".vqv3: mode " + std::to_string(h.mode) + " is neither 0 (fp32) nor 1 (bf16)", false;
    if (in[14] || in[15] || zero32) return err = ".vqv3: a reserved field of the file header is not zero", false;
    if (h.kind == KIND_INDICES && (h.mode != 0 || tol_bits != 0)) return err = ".vqv3: a file of kind 0 carries mode 0 and tol +0.0", false;
    return true;
}

// the grid's section offsets from its name's length, total and payload_bytes, the grid beginning at `at`
inline void layout(Grid& g, int kind, uint64_t at)
{
    const uint64_t n = g.total;
    g.meta_at = at;
    g.origins_at = at + GRID_FIXED_BYTES + g.name.size();
    g.payload_field_at = g.origins_at - 8;
    g.indices_at = g.origins_at + 12 * n;
    g.masks_at = g.indices_at + 128 * n;
    g.codes_at = kind == KIND_ACTIVE ? g.masks_at + 64 * n : g.masks_at;
    g.payload_at = kind == KIND_ACTIVE ? g.codes_at + 2 * n : g.masks_at;
    g.end_at = g.payload_at + g.payload_bytes;
}

inline void emit_grid_meta(const Grid& g, std::vector<unsigned char>& out)
{
    out.assign((size_t)(GRID_FIXED_BYTES + g.name.size()), 0);
    unsigned char* p = out.data();
    const uint32_t name_len = (uint32_t)g.name.size();
    const uint16_t shp[3] = {4, 4, 4};
    std::memcpy(p, &name_len, 4), p += 4;
    if (name_len) std::memcpy(p, g.name.data(), name_len);
    p += name_len;
    std::memcpy(p, g.transform, 64), p += 64;
    std::memcpy(p, shp, 6), p += 6;
    std::memcpy(p, &g.total, 4), p += 4;
    *p = (unsigned char)(g.has_background ? 1 : 0), p += 4;
    if (g.has_background) std::memcpy(p, g.background, 12);
    p += 12;
    std::memcpy(p, &g.payload_bytes, 8);
}

// the metadata of the grid that begins at `at` in a file of file_bytes bytes, with its layout; every section lies inside the file
inline bool parse_grid_meta(const File& f, uint64_t file_bytes, int kind, uint64_t at, Grid& g, std::string& err)
{
    const std::string trunc = ".vqv3: file truncated inside the metadata of a grid";
    uint32_t name_len = 0;
    if (at > file_bytes || file_bytes - at < 4 || !f.read_at(at, &name_len, 4)) return err = trunc, false;
    if (file_bytes - at - 4 < name_len || file_bytes - at - 4 - name_len < GRID_FIXED_BYTES - 4) return err = trunc, false;
    g.name.resize(name_len);
    if (name_len && !f.read_at(at + 4, &g.name[0], name_len)) return err = trunc, false;
    unsigned char fx[GRID_FIXED_BYTES - 4];
    if (!f.read_at(at + 4 + name_len, fx, sizeof fx)) return err = trunc, false;
    uint16_t shp[3];
    uint32_t bg_bits[3];
    std::memcpy(g.transform, fx, 64);
    std::memcpy(shp, fx + 64, 6);
    std::memcpy(&g.total, fx + 70, 4);
    g.has_background = fx[74];
    std::memcpy(g.background, fx + 78, 12);
    std::memcpy(bg_bits, fx + 78, 12);
    std::memcpy(&g.payload_bytes, fx + 90, 8);
    const std::string who = ".vqv3: grid '" + g.name + "' ";
    if (shp[0] != 4 || shp[1] != 4 || shp[2] != 4)
        return err = who + "has latent shape [" + std::to_string(shp[0]) + "," + std::to_string(shp[1]) + "," + std::to_string(shp[2]) + "], not [4,4,4]", false;
    if (g.has_background > 1 || fx[75] || fx[76] || fx[77]) return err = who + "has a hasBackground byte above 1 or a reserved byte that is not zero", false;
    if (!g.has_background && (bg_bits[0] | bg_bits[1] | bg_bits[2])) return err = who + "has no background but background values that are not +0.0", false;
    if (kind == KIND_INDICES && g.payload_bytes) return err = who + "belongs to a file of kind 0 but has payloadBytes " + std::to_string(g.payload_bytes), false;
    const uint64_t payload = g.payload_bytes;
    g.payload_bytes = 0;
    layout(g, kind, at);            // at most file_bytes + 206 * 2^32: no overflow
    if (g.payload_at > file_bytes || file_bytes - g.payload_at < payload)
        return err = who + "needs more bytes than the file holds (" + std::to_string(g.total) + " leaves, " + std::to_string(payload) + " payload bytes)", false;
    g.payload_bytes = payload;
    g.end_at = g.payload_at + payload;
    return true;
}

// the file header and every grid's metadata; the file's length must be exactly what they imply
inline bool read_index(const File& f, Header& h, std::vector<Grid>& grids, std::string& err)
{
    uint64_t file_bytes = 0;
    unsigned char hb[FILE_HEADER_BYTES];
    if (!f.size(file_bytes)) return err = ".vqv3: cannot read the file's size", false;
    if (file_bytes < FILE_HEADER_BYTES || !f.read_at(0, hb, FILE_HEADER_BYTES)) return err = "Failed to read file header.", false;
    if (!parse_header(hb, h, err)) return false;
    grids.clear();
    uint64_t at = FILE_HEADER_BYTES;
    for (int i = 0; i < h.n_grids; ++i) {
        Grid g;
        if (!parse_grid_meta(f, file_bytes, h.kind, at, g, err)) return false;
        at = g.end_at;
        grids.push_back(std::move(g));
    }
    if (at != file_bytes)
        return err = ".vqv3: the headers imply " + std::to_string(at) + " bytes, the file holds " + std::to_string(file_bytes), false;
    return true;
}

// one grid before any of it is decoded: every index below num_codes; kind 1: every code legal and the record sizes of the codes
// and the masks' popcounts sum to payloadBytes.  Reads in blocks of at most 4096 leaves.
inline bool check_grid(const File& f, const Header& h, const Grid& g, std::string& err)
{
    constexpr uint64_t BLOCK = 4096;
    const std::string who = ".vqv3: grid '" + g.name + "': ";
    std::vector<uint16_t> idx, code;
    std::vector<uint64_t> mask;
    uint64_t need = 0;
    for (uint64_t o = 0; o < g.total; o += BLOCK) {
        const uint64_t m = std::min<uint64_t>(BLOCK, g.total - o);
        idx.resize((size_t)m * 64);
        if (!f.read_at(g.indices_at + 128 * o, idx.data(), 128 * m)) return err = who + "cannot read the indices", false;
        if (h.num_codes < 65536)
            for (uint64_t i = 0; i < m * 64; ++i)
                if (idx[i] >= h.num_codes)
                    return err = who + "index " + std::to_string(idx[i]) + " at leaf " + std::to_string(o + i / 64) + ", position " + std::to_string(i % 64) +
                                 " is out of range (num_codes " + std::to_string(h.num_codes) + ")", false;
        if (h.kind != KIND_ACTIVE) continue;
        mask.resize((size_t)m * 8);
        code.resize((size_t)m);
        if (!f.read_at(g.masks_at + 64 * o, mask.data(), 64 * m) || !f.read_at(g.codes_at + 2 * o, code.data(), 2 * m))
            return err = who + "cannot read the masks and codes", false;
        for (uint64_t i = 0; i < m; ++i) {
            if (!code_ok(code[i])) {
                char hex[8];
                std::snprintf(hex, sizeof hex, "0x%04X", (unsigned)code[i]);
                return err = who + "code " + hex + " of leaf " + std::to_string(o + i) + " is neither 0xFFFE, 0xFFFF nor three widths of 0..16", false;
            }
            need += record_bytes(code[i], popcount512(&mask[i * 8]));   // at most 6144 * 2^32
        }
    }
    if (h.kind == KIND_ACTIVE && need != g.payload_bytes)
        return err = who + "the codes and masks need " + std::to_string(need) + " payload bytes, the grid's header says " + std::to_string(g.payload_bytes), false;
    return true;
}

}  // namespace vqv3f
