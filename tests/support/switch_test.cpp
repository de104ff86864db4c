// The environment switches of libcnfhip.so (continuousnf.jl_amd/csrc/cnf_switch.h) on the CPU: every kind's parse rule at its
// edges, for every row of that kind; the accessor with variables set before its first read, and again after the environment
// changed (a switch is read once per process).  Prints the table's names, one per line, for tests/test_switches.py.
#include "cnf_switch.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Edge { const char* text; int want; };       // text == nullptr: the variable is unset
static void edges(const SwitchRow& r, const Edge* e, int n) {
    for (int i = 0; i < n; ++i) {
        const int got = cnf_switch_parse(r, e[i].text);
        CHECK(got == e[i].want, "%s=%s gives %d, not %d", r.env, e[i].text ? e[i].text : "(unset)", got, e[i].want);
    }
}

// the rule of each kind, for every row that has it
static void parse_rules() {
    int kinds_seen = 0;
    for (int s = 0; s < SW_COUNT; ++s) {
        const SwitchRow& r = CNF_SWITCHES[s];
        const int d = r.dflt;
        kinds_seen |= 1 << r.kind;
        CHECK(cnf_switch_parse(r, nullptr) == d, "%s: unset is %d, the default is %d", r.env, cnf_switch_parse(r, nullptr), d);
        switch (r.kind) {
            case SWK_OFF_AT_0: {
                const Edge e[] = {{nullptr, 1}, {"", 1}, {"0", 0}, {"1", 1}, {"01", 0}, {"x", 1}};
                edges(r, e, 6);
            } break;
            case SWK_ON_AT_1: {
                const Edge e[] = {{nullptr, 0}, {"", 0}, {"0", 0}, {"1", 1}, {"01", 0}, {"x", 0}, {"10", 1}};
                edges(r, e, 7);
            } break;
            case SWK_ON_IF_SET: {         // NAME=0 means on
                const Edge e[] = {{nullptr, 0}, {"", 1}, {"0", 1}, {"1", 1}, {"01", 1}, {"x", 1}};
                edges(r, e, 6);
            } break;
            case SWK_POS_INT: {
                const Edge e[] = {{nullptr, d}, {"", d}, {"0", d}, {"-3", d}, {"x", d}, {"1", 1}, {"01", 1}, {"750", 750}};
                edges(r, e, 8);
            } break;
            case SWK_INT_ABOVE_4: {
                const Edge e[] = {{nullptr, d}, {"", d}, {"0", d}, {"-3", d}, {"x", d}, {"1", d}, {"4", d}, {"5", 5}, {"64", 64}};
                edges(r, e, 9);
            } break;
            case SWK_ANY_INT: {           // (the use site ignores what is out of its range: the table hands it on as it stands)
                const Edge e[] = {{nullptr, d}, {"", 0}, {"0", 0}, {"-3", -3}, {"x", 0}, {"1", 1}, {"01", 1}, {"128", 128}, {"129", 129}};
                edges(r, e, 9);
            } break;
            case SWK_TRISTATE: {
                const Edge e[] = {{nullptr, -1}, {"", 1}, {"0", 0}, {"1", 1}, {"01", 0}, {"x", 1}};
                edges(r, e, 6);
            } break;
        }
    }
    CHECK(kinds_seen == (1 << (SWK_TRISTATE + 1)) - 1, "a kind without a row: %x", kinds_seen);
    // the rows whose rule the name does not tell
    CHECK(CNF_SWITCHES[SW_WAVE_XWG_MIN].kind == SWK_INT_ABOVE_4 && CNF_SWITCHES[SW_WAVE_XWG_MIN].dflt == 513, "CNF_WAVE_XWG_MIN");
    CHECK(CNF_SWITCHES[SW_WGRAD_KS].kind == SWK_ANY_INT && CNF_SWITCHES[SW_WGRAD_KS].dflt == 0, "CNF_WGRAD_KS");
    CHECK(CNF_SWITCHES[SW_ADJ_SPLIT].kind == SWK_TRISTATE && CNF_SWITCHES[SW_ADJ_SPLIT].dflt == -1, "CNF_ADJ_SPLIT");
    CHECK(CNF_SWITCHES[SW_SOLVE_WAIT_US].dflt == 2000 && CNF_SWITCHES[SW_SOLVE_POLL_LIMIT].dflt == 0x7fffffff &&
          CNF_SWITCHES[SW_GRAD_FSTEPS].dflt == 0, "the integers' defaults");
    for (CnfSwitch s : {SW_WGRAD_LDS, SW_WGRAD_VALU, SW_WGRAD_FP32})
        CHECK(CNF_SWITCHES[s].kind == SWK_ON_IF_SET && std::strstr(CNF_SWITCHES[s].meaning, "=0 too"), "%s says that =0 means on", CNF_SWITCHES[s].env);
}

static void read_all(int (&v)[SW_COUNT]) {
#define X(name, kind, dflt, meaning) v[SW_##name] = cnf_switch<SW_##name>();
    CNF_SWITCH_TABLE(X)
#undef X
}

// the accessor: variables set before the first read; the same values after the environment changed
static void accessor() {
    for (int s = 0; s < SW_COUNT; ++s) unsetenv(CNF_SWITCHES[s].env);
    const struct { CnfSwitch s; const char* text; int want; } set[] = {
        {SW_PERSISTENT, "01", 0}, {SW_WAVE_GRAD, "x", 1}, {SW_STEP_V1, "01", 0}, {SW_TRACE_FP32, "1", 1}, {SW_WGRAD_LDS, "0", 1},
        {SW_WGRAD_FP32, "", 1}, {SW_WAVE_XWG_MIN, "4", 513}, {SW_SOLVE_WAIT_US, "-5", 2000}, {SW_SOLVE_POLL_LIMIT, "1", 1},
        {SW_WGRAD_KS, "129", 129}, {SW_ADJ_SPLIT, "", 1},
    };
    int want[SW_COUNT];
    for (int s = 0; s < SW_COUNT; ++s) want[s] = CNF_SWITCHES[s].dflt;
    for (const auto& e : set) { setenv(CNF_SWITCHES[e.s].env, e.text, 1); want[e.s] = e.want; }
    int first[SW_COUNT], second[SW_COUNT];
    read_all(first);
    for (int s = 0; s < SW_COUNT; ++s) CHECK(first[s] == want[s], "%s reads %d, not %d", CNF_SWITCHES[s].env, first[s], want[s]);
    // every variable now says something that would parse to another value than the one read
    for (int s = 0; s < SW_COUNT; ++s) {
        const SwitchRow& r = CNF_SWITCHES[s];
        const char* other = nullptr;
        for (const char* t : {"0", "1", "77"}) if (cnf_switch_parse(r, t) != first[s]) other = t;
        if (other) setenv(r.env, other, 1); else unsetenv(r.env);
        CHECK(cnf_switch_parse(r, getenv(r.env)) != first[s], "%s: no other value to change to", r.env);
    }
    read_all(second);
    for (int s = 0; s < SW_COUNT; ++s) CHECK(second[s] == first[s], "%s was %d and is %d after the environment changed", CNF_SWITCHES[s].env, first[s], second[s]);
}

int main() {
    parse_rules();
    accessor();
    for (int s = 0; s < SW_COUNT; ++s) {
        CHECK(std::strncmp(CNF_SWITCHES[s].env, "CNF_", 4) == 0 && CNF_SWITCHES[s].meaning[0], "row %d", s);
        for (int t = 0; t < s; ++t) CHECK(std::strcmp(CNF_SWITCHES[s].env, CNF_SWITCHES[t].env) != 0, "%s twice", CNF_SWITCHES[s].env);
        std::printf("%s\n", CNF_SWITCHES[s].env);
    }
    if (fails) { std::printf("FAILED (%d)\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
