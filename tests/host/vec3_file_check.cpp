// Stand-alone check of the .vqv3 reader / writer core of vqvdb_amd/csrc/vq_vec3_file_format.h on the host: a two-grid kind-1 file and
// a kind-0 file written into a directory and read back, then every refusal: damaged header fields, a file one byte short and one
// long, payloadBytes off by 8, illegal codes, an index >= numCodes, a truncation at every section boundary, and headers whose
// counts would overflow or exhaust memory if they were believed before the length check.  Built with -fsanitize=address,undefined by
// tests/test_vec3_file_format_host.py; exits 0 when every check holds, prints the failed check and exits 1 otherwise.
//   usage: vec3_file_check <directory>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../vqvdb_amd/csrc/vq_vec3_file_format.h"

namespace {

using namespace vqv3f;
using Bytes = std::vector<unsigned char>;

int failures = 0, checks = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        ++checks;                                                         \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

struct GridData {
    Grid meta;
    std::vector<int32_t> origins;
    std::vector<uint16_t> indices, codes;
    std::vector<uint64_t> masks;
    Bytes payload;
};

uint32_t rng_state = 12345;
uint32_t rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

GridData make_grid(const std::string& name, uint32_t n, int kind, bool background, uint32_t num_codes)
{
    GridData g;
    g.meta.name = name;
    for (int i = 0; i < 16; ++i) g.meta.transform[i] = 0.25f * (float)(i + 1);
    g.meta.total = n;
    g.meta.has_background = background;
    if (background) g.meta.background[0] = -0.0f, g.meta.background[1] = 1e30f, g.meta.background[2] = 3.5f;
    const int codes[6] = {CODE_KEPT, CODE_RAW, 0, 1 | 2 << 5 | 16 << 10, 16 | 16 << 5 | 16 << 10, 7};
    for (uint32_t l = 0; l < n; ++l) {
        for (int k = 0; k < 3; ++k) g.origins.push_back((int32_t)(rnd() % 4096) * 8 - 16384);
        for (int k = 0; k < 64; ++k) g.indices.push_back((uint16_t)(rnd() % num_codes));
        if (kind != KIND_ACTIVE) continue;
        uint64_t words[8];
        for (int j = 0; j < 8; ++j) {
            words[j] = ((uint64_t)rnd() << 40) ^ ((uint64_t)rnd() << 20) ^ rnd();
            if (l % 5 == 0) words[j] = 0;                  // a leaf without an active voxel
            if (l % 5 == 1) words[j] = ~uint64_t(0);       // a full leaf
            if (l % 5 == 2) words[j] = j == 3 ? 1 : 0;     // a single voxel
        }
        const int code = codes[l % 6];
        const uint64_t size = record_bytes(code, popcount512(words));
        for (int j = 0; j < 8; ++j) g.masks.push_back(words[j]);
        g.codes.push_back((uint16_t)code);
        for (uint64_t b = 0; b < size; ++b) g.payload.push_back((unsigned char)rnd());
    }
    g.meta.payload_bytes = g.payload.size();
    return g;
}

// the whole file in memory, through the same emit and layout functions the library streams chunks with
Bytes assemble(const Header& h, std::vector<GridData>& grids)
{
    Bytes out(FILE_HEADER_BYTES);
    emit_header(h, out.data());
    Bytes meta;
    for (GridData& g : grids) {
        layout(g.meta, h.kind, out.size());
        emit_grid_meta(g.meta, meta);
        out.insert(out.end(), meta.begin(), meta.end());
        auto put = [&](const void* p, size_t n) { out.insert(out.end(), (const unsigned char*)p, (const unsigned char*)p + n); };
        put(g.origins.data(), g.origins.size() * 4);
        put(g.indices.data(), g.indices.size() * 2);
        if (h.kind == KIND_ACTIVE) {
            put(g.masks.data(), g.masks.size() * 8);
            put(g.codes.data(), g.codes.size() * 2);
            put(g.payload.data(), g.payload.size());
        }
    }
    return out;
}

bool write_file(const std::string& path, const Bytes& b)
{
    File f;
    return f.open_write(path.c_str()) && f.write_at(0, b.data(), b.size()) && f.close();
}

// everything the library does with a file before it decodes a leaf; "" when the file passes
std::string parse(const std::string& path, Header* h_out = nullptr, std::vector<Grid>* grids_out = nullptr)
{
    File f;
    if (!f.open_read(path.c_str())) return "cannot open";
    Header h;
    std::vector<Grid> grids;
    std::string err;
    if (!read_index(f, h, grids, err)) return err.empty() ? "read_index failed without a message" : err;
    for (const Grid& g : grids)
        if (!check_grid(f, h, g, err)) return err.empty() ? "check_grid failed without a message" : err;
    if (h_out) *h_out = h;
    if (grids_out) *grids_out = grids;
    return "";
}

std::string parse_bytes(const std::string& dir, const Bytes& b)
{
    const std::string path = dir + "/case.vqv3";
    if (!write_file(path, b)) return "";   // a case that cannot be written counts as accepted: the check fails
    return parse(path);
}

void roundtrip(const std::string& dir, int kind)
{
    Header h;
    h.n_grids = 3, h.num_codes = 4096, h.kind = kind, h.mode = kind ? 1 : 0, h.tol = kind ? 0.0625f : 0.0f;
    std::vector<GridData> grids = {make_grid("velocity", 37, kind, true, 4096), make_grid("", 0, kind, false, 4096),
                                   make_grid(std::string(300, 'n'), 11, kind, false, 4096)};
    const Bytes bytes = assemble(h, grids);
    const std::string path = dir + (kind ? "/two_grids_active.vqv3" : "/two_grids_indices.vqv3");
    CHECK(write_file(path, bytes));
    Header h2;
    std::vector<Grid> g2;
    const std::string err = parse(path, &h2, &g2);
    CHECK(err.empty());
    if (!err.empty()) {
        std::printf("  %s\n", err.c_str());
        return;
    }
    CHECK(h2.n_grids == 3 && h2.num_codes == 4096 && h2.kind == kind && h2.mode == h.mode && std::memcmp(&h2.tol, &h.tol, 4) == 0);
    CHECK(g2.size() == 3);
    File f;
    CHECK(f.open_read(path.c_str()));
    for (size_t i = 0; i < g2.size() && i < grids.size(); ++i) {
        const Grid &a = grids[i].meta, &b = g2[i];
        CHECK(a.name == b.name && a.total == b.total && a.has_background == b.has_background && a.payload_bytes == b.payload_bytes);
        CHECK(std::memcmp(a.transform, b.transform, 64) == 0 && std::memcmp(a.background, b.background, 12) == 0);
        CHECK(a.meta_at == b.meta_at && a.origins_at == b.origins_at && a.indices_at == b.indices_at && a.masks_at == b.masks_at &&
              a.codes_at == b.codes_at && a.payload_at == b.payload_at && a.end_at == b.end_at && a.payload_field_at == b.payload_field_at);
        std::vector<int32_t> org(grids[i].origins.size());
        std::vector<uint16_t> idx(grids[i].indices.size());
        CHECK(f.read_at(b.origins_at, org.data(), org.size() * 4) && org == grids[i].origins);
        CHECK(f.read_at(b.indices_at, idx.data(), idx.size() * 2) && idx == grids[i].indices);
        if (kind != KIND_ACTIVE) continue;
        std::vector<uint64_t> msk(grids[i].masks.size());
        std::vector<uint16_t> cod(grids[i].codes.size());
        Bytes pay(grids[i].payload.size());
        CHECK(f.read_at(b.masks_at, msk.data(), msk.size() * 8) && msk == grids[i].masks);
        CHECK(f.read_at(b.codes_at, cod.data(), cod.size() * 2) && cod == grids[i].codes);
        CHECK(f.read_at(b.payload_at, pay.data(), pay.size()) && pay == grids[i].payload);
    }
    CHECK(g2.back().end_at == bytes.size());
}

void refusals(const std::string& dir)
{
    Header h;
    h.n_grids = 2, h.num_codes = 512, h.kind = KIND_ACTIVE, h.mode = 0, h.tol = 0.5f;
    std::vector<GridData> grids = {make_grid("a", 13, KIND_ACTIVE, true, 512), make_grid("bb", 7, KIND_ACTIVE, false, 512)};
    const Bytes good = assemble(h, grids);
    CHECK(parse_bytes(dir, good).empty());
    const Grid &A = grids[0].meta, &B = grids[1].meta;
    auto refused = [&](Bytes b) { return !parse_bytes(dir, b).empty(); };
    auto with = [&](size_t at, unsigned char v) {
        Bytes b = good;
        b[at] = v;
        return b;
    };
    auto with_u64 = [&](size_t at, uint64_t v) {
        Bytes b = good;
        std::memcpy(&b[at], &v, 8);
        return b;
    };
    auto with_u32 = [&](size_t at, uint32_t v) {
        Bytes b = good;
        std::memcpy(&b[at], &v, 4);
        return b;
    };
    // the file header
    CHECK(refused(with(0, 'X')));                      // magic
    CHECK(refused(with(6, 2)) && refused(with(6, 0)));   // version
    CHECK(refused(with(7, 0)));                        // no grid
    CHECK(refused(with(7, 3)));                        // a grid more than the file holds
    CHECK(refused(with(7, 1)));                        // a grid fewer: bytes past the last grid
    CHECK(refused(with_u32(8, 0)) && refused(with_u32(8, 65537)));   // numCodes
    CHECK(refused(with(12, 2)));                       // kind
    CHECK(refused(with(12, 0)));                       // kind 0 with a tolerance and payloads
    CHECK(refused(with(13, 2)));                       // mode
    CHECK(refused(with(14, 1)) && refused(with(15, 1)) && refused(with(20, 1)) && refused(with(23, 0x80)));   // reserved
    // a grid's metadata: name "a", so the fixed part begins at meta_at + 5
    const size_t fx = (size_t)A.meta_at + 4 + 1;
    CHECK(refused(with(fx + 64, 5)));                  // latent shape
    CHECK(refused(with(fx + 74, 2)));                  // hasBackground
    CHECK(refused(with(fx + 75, 1)) && refused(with(fx + 77, 1)));   // reserved
    CHECK(refused(with((size_t)B.origins_at - 20, 1)));   // grid "bb" has no background: a background value that is not +0.0
    CHECK(refused(with_u64((size_t)A.payload_field_at, A.payload_bytes + 8)));
    CHECK(refused(with_u64((size_t)A.payload_field_at, A.payload_bytes - 8)));
    CHECK(refused(with_u64((size_t)B.payload_field_at, B.payload_bytes + 8)));
    CHECK(refused(with_u64((size_t)B.payload_field_at, ~uint64_t(0))) && refused(with_u64((size_t)B.payload_field_at, uint64_t(1) << 63)));
    CHECK(refused(with_u32((size_t)A.meta_at, 0xFFFFFFFFu)) && refused(with_u32((size_t)A.meta_at, (uint32_t)good.size())));   // nameLength
    CHECK(refused(with_u32(fx + 70, 0xFFFFFFFFu)) && refused(with_u32(fx + 70, A.total + 1)) && refused(with_u32(fx + 70, A.total - 1)));
    {   // payloadBytes off by 8 with the file grown to match: the lengths agree, the record sizes do not
        Bytes b = with_u64((size_t)B.payload_field_at, B.payload_bytes + 8);
        b.insert(b.end(), 8, 0);
        CHECK(refused(b));
    }
    // the file's length
    {
        Bytes b = good;
        b.pop_back();
        CHECK(refused(b));
        b = good;
        b.push_back(0);
        CHECK(refused(b));
    }
    for (const Grid* G : {&A, &B})
        for (uint64_t cut : {G->meta_at, G->meta_at + 4, G->origins_at - 8, G->origins_at, G->indices_at, G->masks_at, G->codes_at, G->payload_at, G->end_at - 1})
            CHECK(refused(Bytes(good.begin(), good.begin() + (size_t)cut)));
    CHECK(refused(Bytes()) && refused(Bytes(good.begin(), good.begin() + 23)) && refused(Bytes(good.begin(), good.begin() + 24)));
    // codes, masks, indices
    for (uint16_t bad : {(uint16_t)17, (uint16_t)(17 << 5), (uint16_t)(17 << 10), (uint16_t)0x8000, (uint16_t)0xFFFD, (uint16_t)31}) {
        Bytes b = good;
        std::memcpy(&b[(size_t)A.codes_at + 2 * 3], &bad, 2);
        CHECK(refused(b));
    }
    {
        Bytes b = good;   // leaf 7 of grid "a" is raw (7 % 6 == 1) with one active voxel (7 % 5 == 2): two more mask bits grow its record
        const size_t raw_leaf = (size_t)A.masks_at + 64 * 7;
        CHECK(grids[0].codes[7] == CODE_RAW && popcount512(&grids[0].masks[7 * 8]) == 1);
        b[raw_leaf] ^= 0x06;
        CHECK(refused(b));
    }
    {
        Bytes b = good;
        const uint16_t k = 512;
        std::memcpy(&b[(size_t)B.indices_at + 128 * 6 + 2 * 63], &k, 2);
        CHECK(refused(b));
        const uint16_t top = 511;
        std::memcpy(&b[(size_t)B.indices_at + 128 * 6 + 2 * 63], &top, 2);
        CHECK(!refused(b));
    }
    // counts that must not be believed before the length check: 2^32 - 1 leaves in a file of 126 bytes, and of 100
    {
        Header h1;
        h1.n_grids = 1, h1.num_codes = 4096, h1.kind = KIND_ACTIVE, h1.mode = 0, h1.tol = 1.0f;
        Grid g;
        g.total = 0xFFFFFFFFu;
        g.payload_bytes = ~uint64_t(0) - 1000;
        Bytes b(FILE_HEADER_BYTES), meta;
        emit_header(h1, b.data());
        emit_grid_meta(g, meta);
        b.insert(b.end(), meta.begin(), meta.end());
        CHECK(b.size() == 126);
        CHECK(refused(b));
        std::memset(&b[126 - 8], 0, 8);
        CHECK(refused(b));
        b.resize(100);
        CHECK(refused(b));
        h1.n_grids = 255;
        emit_header(h1, b.data());
        CHECK(refused(b));
    }
    // kind 0: mode and tol must be zero, payloadBytes 0
    {
        Header h0;
        h0.n_grids = 1, h0.num_codes = 4096, h0.kind = KIND_INDICES;
        std::vector<GridData> g0 = {make_grid("k0", 5, KIND_INDICES, false, 4096)};
        Bytes b = assemble(h0, g0);
        CHECK(parse_bytes(dir, b).empty());
        Bytes c = b;
        c[13] = 1;
        CHECK(refused(c));
        c = b;
        c[19] = 0x80;   // tol -0.0
        CHECK(refused(c));
        c = b;
        c[(size_t)g0[0].meta.payload_field_at] = 8;
        c.insert(c.end(), 8, 0);
        CHECK(refused(c));
    }
}

void record_sizes()
{
    CHECK(record_bytes(CODE_KEPT, 512) == 0 && record_bytes(CODE_RAW, 0) == 0 && record_bytes(CODE_RAW, 1) == 16 && record_bytes(CODE_RAW, 512) == 6144);
    CHECK(record_bytes(1, 0) == 0 && record_bytes(1, 1) == 8 && record_bytes(1, 64) == 8 && record_bytes(1, 65) == 16 && record_bytes(1, 512) == 64);
    CHECK(record_bytes(16 | 16 << 5 | 16 << 10, 512) == 3072 && record_bytes(16 | 16 << 5 | 16 << 10, 511) == 3072 && record_bytes(2 << 5, 63) == 16);
    CHECK(code_ok(0) && code_ok(CODE_KEPT) && code_ok(CODE_RAW) && code_ok(16 | 16 << 5 | 16 << 10) && !code_ok(17) && !code_ok(0x8000) && !code_ok(0xFFFD));
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::printf("usage: vec3_file_check <directory>\n");
        return 2;
    }
    const std::string dir = argv[1];
    record_sizes();
    roundtrip(dir, KIND_ACTIVE);
    roundtrip(dir, KIND_INDICES);
    refusals(dir);
    if (failures) {
        std::printf("vec3 file: %d of %d checks failed\n", failures, checks);
        return 1;
    }
    std::printf("vec3 file ok: %d checks\n", checks);
    return 0;
}
