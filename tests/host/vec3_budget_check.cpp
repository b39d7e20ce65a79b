// Stand-alone check of the host arithmetic of vqvdb_amd/csrc/vq_vec3_budget_format.h: the pick of a rung from compact sizes and the
// size of a .vqv3 file, against restatements written out here, on the cases of tests/test_vec3_budget_host.py and on the counts that
// only 64-bit sums hold: 2^32 - 1 leaves with a payload of 6144 bytes each, and totals that would pass 2^63 - 1, which must be
// refused and not wrapped.  Built with -fsanitize=address,undefined by tests/test_vec3_budget_format_host.py; exits 0 when every
// check holds, prints the failed check and exits 1 otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../vqvdb_amd/csrc/vq_vec3_budget_format.h"

namespace {

int failures = 0, checks = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        ++checks;                                                         \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// the fields of vqhip_vec3_grid_source that the size depends on or that the writer checks, in a struct of this program's own
struct Source {
    const char* name;
    const float* const* leaf_ptrs;
    const int32_t* origins;
    int64_t n_leaves;
    const uint64_t* masks;
};

const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

// restated: the smallest tolerance by value that fits, NaN never, the first of equals
int ref_pick(const std::vector<int64_t>& bytes, const std::vector<float>& tols, int64_t budget)
{
    int best = -1;
    for (size_t t = 0; t < tols.size(); ++t)
        if (!std::isnan(tols[t]) && bytes[t] <= budget && (best < 0 || tols[t] < tols[(size_t)best])) best = (int)t;
    return best;
}

void check_pick(const std::vector<int64_t>& bytes, const std::vector<float>& tols)
{
    std::vector<int64_t> budgets = {0, INT64_MAX};
    for (int64_t b : bytes)
        for (int64_t d = -1; d <= 1; ++d)
            if (!(b == 0 && d < 0) && !(b == INT64_MAX && d > 0)) budgets.push_back(b + d);
    for (int64_t budget : budgets) {
        int64_t smallest = -7;
        const int got = vqv3b::active_rate_pick(bytes.data(), tols.data(), (int)tols.size(), budget, &smallest);
        CHECK(got == ref_pick(bytes, tols, budget));
        CHECK(got == vqv3b::active_rate_pick(bytes.data(), tols.data(), (int)tols.size(), budget));
        int64_t least = -1;
        for (size_t t = 0; t < tols.size(); ++t)
            if (!std::isnan(tols[t]) && (least < 0 || bytes[t] < least)) least = bytes[t];
        CHECK(smallest == least);
    }
}

void picks()
{
    check_pick({900, 500, 100, 0}, {0.1f, 0.2f, 0.4f, 0.8f});
    check_pick({100, 500, 900, 2000}, {0.1f, 0.2f, 0.4f, 0.8f});              // sizes that rise with the tolerance
    check_pick({700, 300, 900, 200, 650}, {0.1f, 0.2f, 0.4f, 0.8f, 1.6f});
    check_pick({200, 900, 300, 700}, {0.8f, 0.4f, 0.2f, 0.1f});
    check_pick({0, 700, 300}, {NaN, 0.1f, 0.2f});
    check_pick({300, 300, 800, 300}, {0.2f, 0.2f, 0.1f, 0.2f});
    check_pick({6144, 6000, 5000, 0}, {-1.0f, 0.0f, 0.5f, Inf});
    check_pick({10, 10}, {0.0f, -0.0f});
    check_pick({0, 0}, {NaN, NaN});
    check_pick({512}, {0.25f});
    check_pick({INT64_MAX, INT64_MAX - 1}, {0.5f, 1.0f});
    const std::vector<int64_t> b = {100, 500, 900};
    const std::vector<float> t = {0.1f, 0.2f, 0.4f};
    CHECK(vqv3b::active_rate_pick(b.data(), t.data(), 3, 100) == 0);          // a budget equal to a size ...
    CHECK(vqv3b::active_rate_pick(b.data(), t.data(), 3, 99) == -1);          // ... and one byte below it
    const std::vector<int64_t> dup = {300, 300, 800};
    const std::vector<float> dt = {0.2f, 0.2f, 0.1f};
    CHECK(vqv3b::active_rate_pick(dup.data(), dt.data(), 3, 300) == 0 && vqv3b::active_rate_pick(dup.data(), dt.data(), 3, 800) == 2);
    // refusals
    CHECK(vqv3b::active_rate_pick(b.data(), t.data(), 3, -1) == -1);
    CHECK(vqv3b::active_rate_pick(b.data(), t.data(), 0, 1000) == -1);
    CHECK(vqv3b::active_rate_pick(nullptr, t.data(), 3, 1000) == -1 && vqv3b::active_rate_pick(b.data(), nullptr, 3, 1000) == -1);
    std::vector<int64_t> many(65, 7);
    std::vector<float> mt(65, 0.5f);
    CHECK(vqv3b::active_rate_pick(many.data(), mt.data(), 64, 7) == 0 && vqv3b::active_rate_pick(many.data(), mt.data(), 65, 7) == -1);
    const std::vector<int64_t> neg = {100, -1, 900};
    int64_t smallest = 5;
    CHECK(vqv3b::active_rate_pick(neg.data(), t.data(), 3, 1000, &smallest) == -1 && smallest == -1);
    const std::vector<float> nt = {0.1f, NaN, 0.4f};
    CHECK(vqv3b::active_rate_pick(neg.data(), nt.data(), 3, 1000) == -1);     // a negative size is refused on a NaN rung too
}

// restated from the format's description, in 128 bits so that the restatement itself cannot wrap
__int128 ref_bytes(const std::vector<Source>& g, int kind, const std::vector<int64_t>& payload)
{
    __int128 s = 24;
    for (size_t i = 0; i < g.size(); ++i)
        s += 102 + (__int128)std::strlen(g[i].name) + (__int128)g[i].n_leaves * (12 + 128 + (kind == 1 ? 64 + 2 : 0)) + (payload.empty() ? 0 : payload[i]);
    return s;
}

void sizes()
{
    const float* leaf = nullptr;
    const float* const ptrs[1] = {leaf};        // never followed: only tested against NULL
    const int32_t origin[3] = {0, 0, 0};
    const uint64_t mask[8] = {0};
    const std::string long_name(300, 'n');
    for (int kind = 0; kind <= 1; ++kind) {
        std::vector<Source> g = {{"", ptrs, origin, 23, mask}, {"empty", nullptr, nullptr, 0, nullptr}, {long_name.c_str(), ptrs, origin, 9, mask}};
        const std::vector<int64_t> pay = kind ? std::vector<int64_t>{4712, 0, 88} : std::vector<int64_t>{0, 0, 0};
        const int64_t want = 24 + (102 + 0 + 23 * (kind ? 206 : 140)) + (102 + 5) + (102 + 300 + 9 * (kind ? 206 : 140)) + (kind ? 4800 : 0);
        CHECK((__int128)want == ref_bytes(g, kind, pay));
        CHECK(vqv3b::file_bytes(g.data(), 3, kind, pay.data()) == want);
        CHECK(vqv3b::file_bytes(g.data(), 3, kind, (const int64_t*)nullptr) == (kind ? -1 : want));
        CHECK(vqv3b::file_bytes(g.data(), 1, kind, pay.data()) == 24 + 102 + 23 * (kind ? 206 : 140) + pay[0]);
        // the layout the writer uses gives the same end
        vqv3f::Grid M;
        M.name = long_name;
        M.total = 9;
        M.payload_bytes = (uint64_t)pay[2];
        vqv3f::layout(M, kind, 1000);
        CHECK(M.end_at == 1000 + 102 + 300 + 9 * (uint64_t)(kind ? 206 : 140) + (uint64_t)pay[2]);
        // what the writer refuses
        CHECK(vqv3b::file_bytes((const Source*)nullptr, 3, kind, pay.data()) == -1);
        CHECK(vqv3b::file_bytes(g.data(), 0, kind, pay.data()) == -1 && vqv3b::file_bytes(g.data(), 256, kind, pay.data()) == -1);
        CHECK(vqv3b::file_bytes(g.data(), 3, 2, pay.data()) == -1 && vqv3b::file_bytes(g.data(), 3, -1, pay.data()) == -1);
        std::vector<Source> bad = g;
        bad[2].name = nullptr;
        CHECK(vqv3b::file_bytes(bad.data(), 3, kind, pay.data()) == -1);
        bad = g, bad[2].leaf_ptrs = nullptr;
        CHECK(vqv3b::file_bytes(bad.data(), 3, kind, pay.data()) == -1);
        bad = g, bad[2].origins = nullptr;
        CHECK(vqv3b::file_bytes(bad.data(), 3, kind, pay.data()) == -1);
        bad = g, bad[2].masks = nullptr;
        CHECK(vqv3b::file_bytes(bad.data(), 3, kind, pay.data()) == (kind ? -1 : want));      // kind 0 ignores masks
        bad = g, bad[0].n_leaves = -1;
        CHECK(vqv3b::file_bytes(bad.data(), 3, kind, pay.data()) == -1);
        bad = g, bad[0].n_leaves = int64_t(1) << 32;
        CHECK(vqv3b::file_bytes(bad.data(), 3, kind, pay.data()) == -1);
        std::vector<int64_t> p2 = pay;
        p2[1] = -1;
        CHECK(vqv3b::file_bytes(g.data(), 3, kind, p2.data()) == -1);
        p2[1] = 8;
        CHECK(vqv3b::file_bytes(g.data(), 3, kind, p2.data()) == (kind ? want + 8 : -1));    // kind 0 has no payload
    }
    // 2^32 - 1 leaves, every one raw and full: a payload of n * 6144 bytes
    const int64_t n = 0xFFFFFFFFll;
    std::vector<Source> big = {{"big", ptrs, origin, n, mask}};
    std::vector<int64_t> pay = {n * 6144};
    CHECK(vqv3b::file_bytes(big.data(), 1, 1, pay.data()) == 24 + 102 + 3 + n * 206 + n * 6144);
    CHECK((__int128)vqv3b::file_bytes(big.data(), 1, 1, pay.data()) == ref_bytes(big, 1, pay));
    CHECK(vqv3b::file_bytes(big.data(), 1, 0, (const int64_t*)nullptr) == 24 + 102 + 3 + n * 140);
    // 255 such grids still have a 64-bit size
    std::vector<Source> all(255, big[0]);
    std::vector<int64_t> pays(255, n * 6144);
    CHECK((__int128)vqv3b::file_bytes(all.data(), 255, 1, pays.data()) == ref_bytes(all, 1, pays));
    // a sum that would pass 2^63 - 1 is refused, wherever the term that passes it stands; the largest sum that fits is given
    const int64_t fixed = 24 + 102 + 3 + n * 206;
    pay[0] = INT64_MAX - fixed;
    CHECK(vqv3b::file_bytes(big.data(), 1, 1, pay.data()) == INT64_MAX);
    pay[0] = INT64_MAX - fixed + 1;
    CHECK(vqv3b::file_bytes(big.data(), 1, 1, pay.data()) == -1);
    pay[0] = INT64_MAX;
    CHECK(vqv3b::file_bytes(big.data(), 1, 1, pay.data()) == -1);
    std::vector<Source> two = {big[0], {"", nullptr, nullptr, 0, nullptr}};
    std::vector<int64_t> p2 = {INT64_MAX - fixed, 0};
    CHECK(vqv3b::file_bytes(two.data(), 2, 1, p2.data()) == -1);              // the second grid's 102 bytes pass it
    p2 = {INT64_MAX / 2, INT64_MAX / 2};
    CHECK(vqv3b::file_bytes(two.data(), 2, 1, p2.data()) == -1);
    p2 = {INT64_MAX / 2 - fixed, INT64_MAX / 2 - 102};
    CHECK((__int128)vqv3b::file_bytes(two.data(), 2, 1, p2.data()) == ref_bytes(two, 1, p2));
    p2 = {INT64_MAX, INT64_MAX};
    CHECK(vqv3b::file_bytes(two.data(), 2, 1, p2.data()) == -1);
}

}  // namespace

int main()
{
    picks();
    sizes();
    if (failures) {
        std::printf("vec3 budget check: %d of %d checks failed\n", failures, checks);
        return 1;
    }
    std::printf("vec3 budget ok: %d checks\n", checks);
    return 0;
}
