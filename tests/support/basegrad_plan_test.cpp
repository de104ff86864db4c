// The layout of the base-gradient buffer (continuousnf.jl_amd/csrc/cnf_basegrad_plan.h) on the CPU: the regions of one plan
// are disjoint and in order, and no word that either kind of base uses as a ticket lies inside a region where the other kind
// (at ANY batch) writes results, partials or whitened rows -- the buffer is cleared only when it grows, and the kind of a
// handle's base may change between calls.
#include "cnf_basegrad_plan.h"
#include <cstdio>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main() {
    const int Bs[] = {1, 15, 16, 17, 64, 65, 300, 4096, 4097, 8192, 100000};
    for (int n_in = 1; n_in <= 1100; n_in += (n_in < 200 ? 1 : 37)) {
        size_t first_non_ticket[3] = {0, (size_t)-1, (size_t)-1};
        int tickets[3] = {0, 0, 0};
        for (int kind = 1; kind <= 2; ++kind)
            for (int B : Bs) {
                const BaseGradPlan p = base_grad_plan(n_in, kind, B);
                const int nt = (n_in + 15) / 16;
                CHECK(p.ntiles == (kind == 1 ? nt : nt * (nt + 1) / 2), "n_in %d kind %d", n_in, kind);
                CHECK(p.chunk % 16 == 0 && p.chunk >= 16 && p.nchunks >= 1 && p.nchunks <= 64, "n_in %d B %d: chunk %d x %d", n_in, B, p.chunk, p.nchunks);
                CHECK((long long)p.chunk * p.nchunks >= B && (long long)p.chunk * (p.nchunks - 1) < B, "n_in %d B %d: chunks do not tile the batch", n_in, B);
                CHECK((size_t)p.ntiles <= p.off_result, "n_in %d kind %d: tickets run into the result", n_in, kind);
                CHECK(p.off_part == p.off_result + (size_t)p.ntiles * BG_REC, "n_in %d kind %d", n_in, kind);
                CHECK(p.off_rows == p.off_part + (size_t)p.nchunks * p.ntiles * BG_REC, "n_in %d kind %d", n_in, kind);
                CHECK(p.floats == p.off_rows + (size_t)B * n_in, "n_in %d kind %d", n_in, kind);
                if (p.off_result < first_non_ticket[kind]) first_non_ticket[kind] = p.off_result;
                tickets[kind] = p.ntiles;
            }
        CHECK((size_t)tickets[1] <= first_non_ticket[2], "n_in %d: a diagonal ticket lies where the dense kind writes", n_in);
        CHECK((size_t)tickets[2] <= first_non_ticket[1], "n_in %d: a dense ticket lies where the diagonal kind writes", n_in);
    }
    std::printf("%s\n", fails ? "failed" : "ok");
    return fails ? 1 : 0;
}
