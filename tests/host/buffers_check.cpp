// Stand-alone check of the owning buffer of vqvdb_amd/csrc/vq_buffers.h on the host: the core template over a malloc / free policy
// that counts live blocks and can fail the k-th allocation.  Built with -fsanitize=address,undefined by tests/test_buffers_host.py;
// exits 0 when every check holds, prints the failed check and exits 1 otherwise.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../vqvdb_amd/csrc/vq_buffers.h"

namespace {

struct CountingPolicy {
    using error_type = int;
    static constexpr int ok = 0;
    static int live, allocs, frees, fail_at;   // fail_at: the allocation (counted from 1, from now on) that fails; 0 = none
    static size_t last_bytes;
    static int alloc(void** p, size_t bytes)
    {
        if (fail_at && --fail_at == 0) return 2;
        *p = std::malloc(bytes);
        if (!*p) return 2;
        ++live, ++allocs, last_bytes = bytes;
        return 0;
    }
    static void release(void* p)
    {
        std::free(p);
        --live, ++frees;
    }
};
int CountingPolicy::live = 0, CountingPolicy::allocs = 0, CountingPolicy::frees = 0, CountingPolicy::fail_at = 0;
size_t CountingPolicy::last_bytes = 0;

using P = CountingPolicy;
using Buf = Buffer<double, P>;

int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);  \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

bool empty(const Buf& b) { return b.get() == nullptr && b.capacity() == 0 && b.bytes() == 0 && !b; }
bool holds(const Buf& b, size_t n) { return b.get() != nullptr && b.capacity() == n && b.bytes() == n * sizeof(double); }
void fill(Buf& b)   // every element is the buffer's to write (the sanitizer watches)
{
    for (size_t i = 0; i < b.capacity(); ++i) b[i] = (double)i;
}

void grow_sequence()
{
    Buf b;
    CHECK(empty(b));
    const struct {
        size_t count;
        int allocs, frees;   // what the step allocates and frees
    } steps[] = {{1, 1, 0}, {7, 1, 1}, {7, 0, 0}, {3, 0, 0}, {100, 1, 1}};
    size_t cap = 0;
    for (const auto& s : steps) {
        const int a0 = P::allocs, f0 = P::frees;
        const double* before = b.get();
        CHECK(b.grow(s.count) == 0);
        if (s.count > cap) cap = s.count;
        CHECK(P::allocs - a0 == s.allocs && P::frees - f0 == s.frees);
        CHECK(holds(b, cap) && P::live == 1);
        if (s.allocs) CHECK(P::last_bytes == s.count * sizeof(double));
        else CHECK(b.get() == before);
        fill(b);
    }
    CHECK(b.grow(0) == 0 && holds(b, 100));
}

void failing_first_allocation()
{
    Buf b;
    P::fail_at = 1;
    CHECK(b.grow(5) == 2);
    CHECK(empty(b) && P::live == 0);
    CHECK(b.grow(5) == 0 && holds(b, 5) && P::live == 1);
    fill(b);
}

void failing_regrow()
{
    Buf b;
    CHECK(b.grow(4) == 0);
    P::fail_at = 1;
    CHECK(b.grow(9) == 2);
    CHECK(empty(b) && P::live == 0);   // the old block is gone, nothing half-held
    CHECK(b.grow(2) == 0 && holds(b, 2) && P::live == 1);
    fill(b);
}

void moves()
{
    Buf a;
    CHECK(a.grow(6) == 0);
    double* pa = a.get();
    Buf b(std::move(a));   // move construction
    CHECK(empty(a) && holds(b, 6) && b.get() == pa && P::live == 1);
    Buf c;
    c = std::move(b);      // move assignment onto an empty buffer
    CHECK(empty(b) && holds(c, 6) && c.get() == pa && P::live == 1);
    Buf d;
    CHECK(d.grow(3) == 0 && P::live == 2);
    const int f0 = P::frees;
    d = std::move(c);      // ... onto a non-empty one: its block is freed
    CHECK(P::frees - f0 == 1 && P::live == 1 && empty(c) && holds(d, 6) && d.get() == pa);
    Buf& self = d;
    d = std::move(self);   // ... onto itself: nothing happens
    CHECK(P::frees - f0 == 1 && P::live == 1 && holds(d, 6) && d.get() == pa);
    fill(d);
    c = std::move(a);      // empty onto empty
    CHECK(empty(a) && empty(c) && P::live == 1);
}

void reset_twice()
{
    Buf b;
    CHECK(b.grow(8) == 0);
    const int f0 = P::frees;
    b.reset();
    CHECK(empty(b) && P::frees - f0 == 1 && P::live == 0);
    b.reset();
    CHECK(empty(b) && P::frees - f0 == 1 && P::live == 0);
}

void array_of_buffers()
{
    const int f0 = P::frees;
    {
        Buf slots[5];
        CHECK(slots[0].grow(2) == 0 && slots[2].grow(11) == 0 && slots[4].grow(1) == 0);
        CHECK(P::live == 3 && empty(slots[1]) && empty(slots[3]));
        for (Buf& b : slots) fill(b);
    }
    CHECK(P::live == 0 && P::frees - f0 == 3);
}

}  // namespace

int main()
{
    grow_sequence();
    CHECK(P::live == 0);
    failing_first_allocation();
    CHECK(P::live == 0);
    failing_regrow();
    CHECK(P::live == 0);
    moves();
    CHECK(P::live == 0);
    reset_twice();
    array_of_buffers();
    CHECK(P::live == 0 && P::allocs == P::frees && P::fail_at == 0);
    if (failures) return 1;
    std::printf("buffers ok: %d allocations, %d frees\n", P::allocs, P::frees);
    return 0;
}
