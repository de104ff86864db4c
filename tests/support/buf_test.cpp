// CPU test of the handle's owning buffer (continuousnf.jl_amd/csrc/cnf_buf.h) over a counting allocator that can be told to
// fail its n-th allocation, and of the adjoint's coefficient table built from tsit5_row (the Python side of the test cuts the
// TS_ macros and tsit5_row out of cnf_dev.h into tsit5_rows.inc and compares the printed table with the oracle's digits).
#include "../../continuousnf.jl_amd/csrc/cnf_buf.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "tsit5_rows.inc"

struct Fake {
    static inline std::vector<std::string> log;     // "alloc <bytes>" / "free"
    static inline std::set<void*> live;
    static inline int allocs = 0, frees = 0, calls = 0, fail_at = -1, bad = 0;
    static inline size_t last_bytes = 0;
    static int alloc(void** p, size_t bytes) {
        ++calls;
        last_bytes = bytes;
        log.push_back("alloc " + std::to_string(bytes));
        if (calls == fail_at) { *p = nullptr; return 2; }
        *p = std::malloc(bytes ? bytes : 1);
        live.insert(*p);
        ++allocs;
        return 0;
    }
    static void free(void* p) {
        log.push_back("free");
        if (!live.erase(p)) ++bad;                   // freed twice, or never allocated
        else std::free(p);
        ++frees;
    }
};

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

struct Elem { double a; float b; };       // 16 bytes: the byte count is elements x element size
static_assert(!std::is_copy_constructible<CnfBuf<Elem, Fake>>::value && !std::is_copy_assignable<CnfBuf<Elem, Fake>>::value, "owning: no copies");

int main() {
    {
        CnfBuf<Elem, Fake> b;
        CHECK(b.data() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(0) == 0 && Fake::calls == 0);                     // nothing to hold: nothing is called
        CHECK(b.reserve(10) == 0 && b.capacity() == 10 && b.data() != nullptr);
        CHECK(Fake::last_bytes == 10 * sizeof(Elem));
        CHECK(static_cast<Elem*>(b) == b.data());

        // within capacity: no allocator call, same pointer
        Elem* p0 = b.data();
        const size_t n_log = Fake::log.size();
        CHECK(b.reserve(10) == 0 && b.reserve(3) == 0);
        CHECK(Fake::log.size() == n_log && b.data() == p0 && b.capacity() == 10);

        // growth: exactly one release, and it comes before the allocation
        CHECK(b.reserve(25) == 0 && b.capacity() == 25);
        CHECK(Fake::log.size() == n_log + 2 && Fake::log[n_log] == "free" && Fake::log[n_log + 1] == "alloc " + std::to_string(25 * sizeof(Elem)));

        // a failed allocation: the allocator's error comes back, the buffer is empty -- and usable again
        Fake::fail_at = Fake::calls + 1;
        CHECK(b.reserve(100) == 2);
        CHECK(b.data() == nullptr && b.capacity() == 0);
        CHECK(Fake::live.empty());                                          // the old allocation was released, once
        CHECK(b.reserve(5) == 0 && b.capacity() == 5 && b.data() != nullptr);
        CHECK(Fake::last_bytes == 5 * sizeof(Elem));

        // swap: each side owns what the other did (traj_reserve grows with its contents kept on top of this)
        CnfBuf<Elem, Fake> c;
        CHECK(c.reserve(7) == 0);
        Elem *pb = b.data(), *pc = c.data();
        b.swap(c);
        CHECK(b.data() == pc && b.capacity() == 7 && c.data() == pb && c.capacity() == 5);
        c.release();
        CHECK(c.data() == nullptr && c.capacity() == 0);
        c.release();                                                        // releasing an empty buffer calls nothing
    }
    // every allocation freed exactly once, over a sequence that included a failure
    CHECK(Fake::allocs == Fake::frees && Fake::live.empty() && Fake::bad == 0);
    CHECK(Fake::calls == Fake::allocs + 1);
    std::printf("allocs %d frees %d failures %d\n", Fake::allocs, Fake::frees, failures);

    const AdjTableau t = adj_tableau(tsit5_row);
    for (int m = 0; m < 6; ++m) {
        std::printf("a %d", m);
        for (int i = 0; i < 5; ++i) std::printf(" %.9g", t.a[m][i]);
        std::printf("\nkc %d", m);
        for (int d = 0; d < 5; ++d) std::printf(" %.9g", t.kc[m][d]);
        std::printf("\n");
    }
    std::printf("b");
    for (int i = 0; i < 6; ++i) std::printf(" %.9g", t.b[i]);
    std::printf("\n");
    return failures ? 1 : 0;
}
