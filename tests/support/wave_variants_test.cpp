// csrc/cnf_wave_variants.h against the selection functions it replaced, on the CPU.  The whole query space of every form -- input
// tiles 1..3, hidden tiles 1..7, the three modes, both values of each second-layer flag -- one line per query:
//   <form> <ni> <nh> <mode> <tanh2> <id2> none | <class>
// where a class is a distinct tuple of template arguments, numbered by first appearance.  wave_variants.expected is the same
// walk over the nine pick_* functions of cnf_wave.hip at the commit before the header, with the kernel's address in the place
// of the tuple: it pins which variants exist and which queries share one.  (test_wave_variants.py compares the two.)
// Then, here: a tuple belongs to one form only, and there are as many tuples as that commit's cnf_wave.o has kernels.
#include "../../continuousnf.jl_amd/csrc/cnf_wave_variants.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

constexpr int KERNELS = 112;           // k_solve_wave symbols in the gfx950 code object of cnf_wave.o

int main() {
    std::vector<WaveVariant> seen;
    std::vector<int> form_of;          // the form that first returned seen[k]
    int per_form[WF_COUNT] = {};
    for (int form = 0; form < WF_COUNT; ++form)
        for (int ni = 1; ni <= 3; ++ni)
            for (int nh = 1; nh <= 7; ++nh)
                for (int mode = 0; mode < 3; ++mode)
                    for (int tanh2 = 0; tanh2 < 2; ++tanh2)
                        for (int id2 = 0; id2 < 2; ++id2) {
                            const auto v = wave_variant((WaveForm)form, ni, nh, mode, tanh2 != 0, id2 != 0);
                            std::printf("%d %d %d %d %d %d ", form, ni, nh, mode, tanh2, id2);
                            if (!v) { std::printf("none\n"); continue; }
                            // the answer is for the tiles and the mode that were asked about
                            CHECK(v->ni == ni && v->nh == nh && v->mode == mode);
                            size_t k = 0;
                            while (k < seen.size() && !(seen[k] == *v)) ++k;
                            if (k == seen.size()) { seen.push_back(*v); form_of.push_back(form); ++per_form[form]; }
                            CHECK(form_of[k] == form);     // no tuple is two forms' answer
                            std::printf("%zu\n", k);
                        }
    // 5 shapes x 3 modes x {tanh, any} + 3 identity | 12 + 2 | 12 + 3 | 4 + 1 | 15 | 15 | 15
    const int want[WF_COUNT] = {33, 14, 15, 5, 15, 15, 15};
    for (int f = 0; f < WF_COUNT; ++f) CHECK(per_form[f] == want[f]);
    CHECK((int)seen.size() == KERNELS);
    return 0;
}
