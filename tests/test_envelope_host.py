"""The envelope sweep's table, restatements and tolerances, checked without a GPU (tests/envelope.py).

- ``mfma_lds_bytes`` reproduces the compile-time layouts of cnf_mfma.hip that can be checked without a device, is monotone
  in width, and puts the plan edges where the table has them;
- every case builds through ``construct`` with the oracle's parameter count, and its oracle numbers are finite;
- the float32 floor of every case (printed with ``-s``) leaves rtol = max(1e-4, 8 x floor) under the cap of 1e-3;
- oracles with a wrong swish s'', a wrong elu s' for a < 0 and softplus switched at 5 fail the bar on at least one case of
  the activation matrix / the regimes: the inputs reach those branches.
"""
import numpy as np
import pytest

from oracle import cnf_oracle as O
from tests import envelope as E
from tests import helpers

T = O.ACT_TANH


# ---------------------------------------------------------------------------------------
# the restatement of mfma_plan_init
# ---------------------------------------------------------------------------------------
def test_lds_bytes_reproduce_the_compile_time_layouts():
    """StLayoutX<...>::total_floats() of the static instantiations (cnf_mfma.hip, "static instantiations": LyCfg3, LyCfg2,
    LyCfg1, LyCfg5, LyCfg5J), worked out by hand from the constexpr formulas of StLayoutX / StLayoutJ (cnf_mfma.hip:90-161:
    img_floats :122, x_off :125, eps_off / du_off / red_off :130-132, red_floats :133, sc_off / bar_off / total_floats :136-138;
    StLayoutJ::tx_off / red_off / total_floats :152-160) -- the same formulas ``mfma_lds_bytes`` restates, so this pins the
    arithmetic, and the device's route assertions (tests/test_gpu_envelope.py) pin the restatement to the C++:
      LyCfg3  32-128-128-32, weights in LDS:  image 128*36 + 128*132 + 32*132 + 288 = 26016; activations 32*(40+136+136+40)
              = 11264; eps, du 2*32*40 = 2560; reduction 256; scalar rows 768; counters 16              -> 40880 floats
      LyCfg2  16-48-16:  image 48*20 + 16*52 + 64 = 1856; 32*(24+56+24) = 3328; 2*32*24 = 1536; 256 + 768 + 16   -> 7760
      LyCfg1  16-16-16:  image 2*16*20 + 32 = 672; 32*3*24 = 2304; 1536; 1040                                    -> 5552
      LyCfg5  128-384-128, streamed (16-sample tiles, images from 0): 16*(136+392+136) = 10624; 2*16*136 = 4352;
              reduction 3*8*32 = 768; 768 + 16                                                                    -> 16528
      LyCfg5J the same with the tangent image tau_1: + 16*392 = 6272                                              -> 22800"""
    assert E.mfma_lds_bytes((32, 128, 128, 32), False) == ("lds", 40880 * 4)
    assert E.mfma_lds_bytes((16, 48, 16), False) == ("lds", 7760 * 4)
    assert E.mfma_lds_bytes((2, 6, 2), False) == ("lds", 5552 * 4)
    assert E.mfma_lds_bytes((128, 384, 128), False) == ("streamed", 16528 * 4)
    assert E.mfma_lds_bytes((128, 384, 128), True) == ("streamed", 22800 * 4)
    # the two state-width edges: 192 bytes under MF_LDS_BYTES; more than 128 padded state rows
    assert E.mfma_lds_bytes((128, 64, 128), True) == ("lds", E.MF_LDS_BYTES - 192)
    assert E.mfma_lds_bytes((129, 64, 129), True)[0] == "none" and E.mfma_lds_bytes((129, 64, 129), False)[0] == "none"
    # a swish layer that is not the last one has no plan; a swish last layer has
    assert E.mfma_lds_bytes((20, 72, 40, 20), False, (E.SW, T, T))[0] == "none"
    assert E.mfma_lds_bytes((20, 72, 40, 20), False, (T, T, E.SW))[0] == "lds"


@pytest.mark.parametrize("jvp", [False, True])
@pytest.mark.parametrize("L", [2, 3, 4, 8])
def test_plan_is_monotone_in_width_and_the_edges_are_the_tables(L, jvp):
    """Over hidden widths 1 .. 2400: lds, then streamed, then none, never back; within a plan the bytes never decrease; the
    edges of ``plan_edges`` are where the plan changes, and the table has a case on each side."""
    order = {"lds": 0, "streamed": 1, "none": 2}
    prev = (0, 0)
    changes = []
    for h in range(1, 2401):
        plan, nbytes = E.mfma_lds_bytes((32,) + (h,) * (L - 1) + (32,), jvp)
        cur = (order[plan], nbytes)
        assert cur[0] >= prev[0], (L, jvp, h, plan)
        if cur[0] == prev[0]:
            assert cur[1] >= prev[1], (L, jvp, h)
        elif h > 1:
            changes.append(h - 1)               # the last width of the previous plan
        if plan != "none":
            assert nbytes <= E.MF_LDS_BYTES
        prev = cur
    a, b, c, d = E.plan_edges(L, jvp)
    assert changes == [a, c] and b == a + 16 and d == c + 16, (L, jvp, changes, (a, b, c, d))
    tag = f"a-L{L}-{'jvp' if jvp else 'vjp'}-h"
    sides = {k: E.CASES[f"{tag}{h}-{k}"] for k, h in zip(("lds-last", "streamed-first", "streamed-last", "beyond"), (a, b, c, d))}
    assert [E.mfma_lds_bytes(s.dims, jvp)[0] for s in sides.values()] == ["lds", "streamed", "streamed", "none"]
    assert sides["lds-last"].route == "mfma-lds" and sides["streamed-first"].route == sides["streamed-last"].route == "mfma-streamed"
    assert sides["beyond"].route in ("generic", "jvp-mfma")
    print(f"\nplan edges L={L} {'JVP' if jvp else 'VJP'}: lds <= {a}, streamed {b} .. {c}, beyond from {d} ({sides['beyond'].route})", end="")


def test_the_other_predicates_have_a_case_on_each_side():
    C = E.CASES
    side = lambda name, fn, *a: fn(C[name].dims, *a)
    assert side("b-grad-inside-1024", E.grad_supported) and not side("b-grad-outside-1025", E.grad_supported)
    assert not any(E.grad_supported(c.dims, c.n_cond) for c in C.values() if max(c.dims) > 1024)
    assert all(E.grad_supported(c.dims, c.n_cond) for c in C.values() if c.grad)
    assert E.grad_supported((16,) + (1024,) * 7 + (16,)), "the LDS bound of k_adj is not reachable before its thread bound"
    assert side("b-adj-mfma-inside-480", E.adj_mfma_supported) and not side("b-adj-mfma-outside-481", E.adj_mfma_supported)
    assert C["b-trace-inside-128"].route_test == "trace-mfma" and C["b-trace-outside-129"].route_test == "generic"
    assert C["b-trace-lds-inside"].route_test == "trace-mfma" and C["b-trace-lds-outside"].route_test == "generic"
    assert E.TRACE_EDGE == (624, 640)
    assert C["b-jvp-mfma-inside-592"].route == "jvp-mfma" and C["b-jvp-mfma-outside-593"].route == "generic"
    for name, inside in (("b-wave-inside-64", True), ("b-wave-outside-65", False), ("b-wave-inside-32x96", True), ("b-wave-outside-32x80", False)):
        assert E.wave_shape(C[name].dims) == inside == C[name].one_launch, name
    assert E.wave_grad_shape(C["b-wave-grad-inside"].dims, C["b-wave-grad-inside"].acts)
    assert not E.wave_grad_shape(C["b-wave-grad-outside-softplus"].dims, C["b-wave-grad-outside-softplus"].acts)
    for name in (n for n in C if n.startswith("b-bcast")):
        assert E.bcast_shape(C[name].dims, C[name].acts) == ("inside" in name) == C[name].one_launch, name


def test_the_activation_matrix_is_complete():
    """Every activation in a hidden and in the last position on every route; swish in a hidden layer takes the generic kernel
    on the shapes k_mfma would hold, a swish last layer stays on k_mfma."""
    for route, (dims, *_rest) in E.ACT_ROUTES.items():
        for a in E.ACTS:
            for pos in ("hidden", "last"):
                if a == T and pos == "last":
                    continue
                c = E.CASES[f"c-{route}-{E.NAME[a]}-{pos}"]
                assert c.acts[0 if pos == "hidden" else -1] == a
                if route == "jvp-mfma":
                    assert c.route == "jvp-mfma" and c.jvp, c.name
                elif route.startswith("mfma") or route.startswith("headline-shape") or route == "trace-mfma":
                    # (in the JVP compute mode k_jvp_mfma takes what k_mfma has no plan for: it keeps the pre-activations)
                    want = (("jvp-mfma" if c.jvp else "generic") if (a == E.SW and pos == "hidden") else
                            ("mfma-streamed" if ("streamed" in route or route == "headline-shape-jvp") else "mfma-lds"))   # (the tangent
                    # images of the JVP mode leave no room for 32-128-128-32's weights in k_mfma's LDS plan)
                    assert c.route == want, (c.name, c.route)
                if route == "trace-mfma":
                    assert c.route_test == "trace-mfma"
    assert E.CASES["c-mfma-lds-swish-last"].route == "mfma-lds" and E.CASES["c-mfma-lds-swish-hidden"].route == "generic"
    waves = [c for c in E.CASES.values() if c.name.startswith("c-wave")]
    assert all(E.wave_shape(c.dims) for c in waves)
    assert all(c.one_launch is True for c in waves if c.route.startswith("mfma")) and E.CASES["c-wave-swish-hidden"].one_launch is False


# ---------------------------------------------------------------------------------------
# every case: construction, finite references, float32 floor
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.CASES))
def test_case_builds_and_its_float32_floor_fits_under_the_cap(name, capsys):
    case = E.CASES[name]
    assert case.route == E.expected_route(case.dims, case.acts, case.jvp, True, case.n_cond)
    assert case.route_test == E.expected_route(case.dims, case.acts, case.jvp, False, case.n_cond)
    assert 1 <= len(case.dims) - 1 <= 8 and 1 <= min(case.dims) and max(case.dims) <= 4096 and case.dims[0] == case.dims[-1] == case.nvars + case.naugs
    icnf = E.model(case)
    flat = case.inputs()[0]
    assert icnf.nn.n_params_internal == case.net.n_params == flat.size
    ref = E.references(name)
    for k, v in ref.items():
        if v is not None:
            assert np.isfinite(v).all(), (name, k)
    fl = E.floors(name)
    with capsys.disabled():
        print(f"\nfloor {name}: " + " ".join(f"{k} {v:.1e}->{E.rtol_of(v):.1e}" for k, v in fl.items()), end="")
    for k, v in fl.items():
        assert np.isfinite(v) and E.rtol_of(v) <= E.RTOL_CAP, (name, k, v)
    if case.grad:
        assert np.abs(ref["grad"]).max() > 0 and np.abs(ref["grad_x"]).max() > 0


def test_regimes_reach_the_pre_activation_ranges_they_are_named_for():
    """First-layer pre-activations: ~1e-3 (tiny), O(1) (unit), |a| of 20..40 on both sides of 15 (saturated)."""
    for c in E.by_family("d"):
        flat, xs, eps, ys, u = c.inputs()
        Ws, bs = O.unflatten_params(c.net, flat.astype(np.float64))
        a = np.abs(Ws[0] @ u[:c.dims[0]].astype(np.float64) + bs[0][:, None])
        regime = c.name.rsplit("-", 1)[1]
        if regime == "tiny":
            assert 2e-4 < np.median(a) < 5e-3 and a.max() < 0.05, (c.name, np.median(a), a.max())
        elif regime == "unit":
            assert 0.1 < np.median(a) < 3, (c.name, np.median(a))
        else:
            assert (a > 20).mean() > 0.2 and (a > 15).any() and (a < 15).any() and np.percentile(a, 90) > 30, (c.name, np.median(a))


# ---------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["swish-d2", "elu-d1", "softplus-5"])
def test_mutant_oracles_fail_the_bar_on_some_case(which):
    """The float64 oracle with one deliberate mistake, held to the bar the device is held to (the case's own rtol): at least
    one case of families (c) / (d) rejects it (the float32 run of the unmutated oracle passes the same bar on all of them:
    test_case_builds_and_its_float32_floor_fits_under_the_cap)."""
    act = {"swish-d2": E.SW, "elu-d1": E.EL, "softplus-5": E.SP}[which]
    cases = [c for c in E.by_family("c") + E.by_family("d") if act in c.acts]
    assert cases
    rejected = []
    for c in cases:
        n_in = c.nvars + c.naugs
        ref, rt = E.references(c.name), E.rtols(c.name)
        over = {k: v / rt[k] for k, v in E.compare(E.mutant_references(c.name, which), ref, n_in).items()}
        if max(over.values()) > 1.0:
            rejected.append((c.name, max(over, key=over.get), max(over.values())))
    print(f"\n{which}: rejected by {len(rejected)} of {len(cases)} cases; worst " +
          ", ".join(f"{n} {k} x{v:.3g}" for n, k, v in sorted(rejected, key=lambda r: -r[2])[:3]), end="")
    assert rejected, which
    if which == "swish-d2":             # s'' enters the gradient only
        assert all(k.startswith("grad") for _, k, _ in rejected)
