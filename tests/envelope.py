"""The accepted network envelope: plan edges, the other support predicates, the activation matrix, pre-activation regimes
(helper module; no GPU needed).

``cnf_create`` takes any Dense chain of 1..8 layers with widths 1..4096, seven activations, either compute mode, with or
without conditioning; a dozen predicates and one LDS-fit computation decide which kernel a network lands on.  This module
restates those decisions in Python (``mfma_lds_bytes``, ``expected_route`` and the ``*_supported`` functions below -- each
names the C++ it restates), derives from them a deterministic table of cases that sit just inside and just outside every
bound, and carries the references and the tolerance rule of the sweep:

    rtol = max(helpers.RTOL, 8 x floor) <= RTOL_CAP = 1e-3,
    floor = what the float32 run of the oracle (numpy float32; the C oracle too where it can run the case) misses the
            float64 oracle by, expressed as the rtol at which it would just meet the bar of ``helpers.assert_parity``
            (state matrices, logpx, regulariser rows) or of the whole-gradient bar  max|err| <= rtol (max|ref| + rms ref).

The floor comes from the oracle alone, never from the device; a case whose floor breaks the cap is changed (smaller scale,
narrower, fewer steps), not loosened -- the table says so where that happened.  The host suite (tests/test_envelope_host.py)
checks the restatements and the floors, the GPU suite (tests/test_gpu_envelope.py) holds the device to them.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import c_oracle as CO
from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import helpers

FLOOR_FACTOR = 8.0
RTOL_CAP = 1e-3
ID, T, SG, SP, RE, SW, EL = (O.ACT_IDENTITY, O.ACT_TANH, O.ACT_SIGMOID, O.ACT_SOFTPLUS, O.ACT_RELU, O.ACT_SWISH, O.ACT_ELU)
ACTS = (ID, T, SG, SP, RE, SW, EL)
NAME = helpers.ACT_NAME

# ---------------------------------------------------------------------------------------
# restatement of the dispatch (continuousnf.jl_amd/csrc)
# ---------------------------------------------------------------------------------------
MF_NB = 32                 # cnf_mfma.h: samples per workgroup tile with the weights in LDS (16 without)
MF_LDS_BYTES = 163840      # cnf_mfma.h
LDS_160K = 160 * 1024


def pad16(x):
    return (x + 15) & ~15


def pad_to(x, residue, modulus):
    """cnf_mfma.hip ``pad_to``: the smallest y >= x with y % modulus == residue."""
    return x + ((residue - x) % modulus + modulus) % modulus


def sw_of(p):              # weight row stride
    return pad_to(p, 4, 16)


def sx_of(p):              # activation row stride
    return pad_to(p, 8, 16)


def pad8m16(x):            # cnf_trace.hip
    return pad16(x) + 8


def _place_lds(P, start, nb, jvp):
    """``place_lds`` of mfma_plan_init: floats of LDS with the images starting at ``start`` and ``nb`` samples per tile."""
    L = len(P) - 1
    o = start + sum(nb * sx_of(p) for p in P)                  # x_off[0..L]
    o += 2 * nb * sx_of(P[0])                                  # eps, du
    if jvp:
        o += sum(nb * sx_of(P[l]) for l in range(1, L))        # tangent images tau_1 .. tau_{L-1}
    o += max(256, 3 * (P[0] >> 4) * MF_NB)                     # the reduction region
    o += MF_NB * 24                                            # scalar-row state
    o += 16                                                    # team-barrier counters / controller scratch
    return o


def mfma_lds_bytes(dims, jvp, acts=None):
    """(plan, bytes) of ``mfma_plan_init`` (cnf_mfma.hip) for the network ``dims`` (dims[0] = n_in: conditioning columns
    do not enter the plan).  plan: "lds" (weights next to the activation images, 32-sample tiles), "streamed" (weights
    stay in HBM / L2, 16-sample tiles, transposed images SWT / wt_off) or "none" (no k_mfma plan: the activations alone
    exceed LDS, more than 128 padded state rows, or a swish layer that is not the last).  bytes: dynamic LDS of the plan
    that was placed last (for "none": of the streamed placement that did not fit, or 0 where placement was not reached)."""
    L = len(dims) - 1
    if acts is not None and any(a == SW for a in acts[:-1]):
        return "none", 0                                       # "sigma' not recoverable from h"
    P = [pad16(d) for d in dims]
    img = sum(P[l + 1] * sw_of(P[l]) for l in range(L)) + sum(P[1:])
    img = (img + 3) & ~3
    total = _place_lds(P, img, MF_NB, jvp)
    plan = "lds"
    if total * 4 > MF_LDS_BYTES:
        plan = "streamed"
        total = _place_lds(P, 0, 16, jvp)
    if total * 4 > MF_LDS_BYTES or P[0] > 128:
        return "none", total * 4
    return plan, total * 4


def _adj_layout(dims, n_cond):
    """The fields of ``adj_mfma_layout`` (cnf_grad.hip) the predicates read."""
    dp = [pad16(dims[0] + n_cond)] + [pad16(d) for d in dims[1:]]
    return dict(dp=dp, sum_o=sum(dp[1:]), maxd=max(dp), nin_p=pad16(dims[0]), L=len(dims) - 1)


def adj_mfma_supported(dims, n_cond=0):
    """cnf_grad.hip: the LDS of k_adj_mfma, (AM_NS PS + AM_EC AM_NS) floats <= 160 KB with AM_NS = 16, AM_EC = 32 and
    PS = pad16(3 sum_o + 2 maxd + nin_p) + 8."""
    m = _adj_layout(dims, n_cond)
    PS = pad16(3 * m["sum_o"] + 2 * m["maxd"] + m["nin_p"]) + 8
    return (16 * PS + 32 * 16) * 4 <= LDS_160K


def grad_supported(dims, n_cond=0):
    """cnf_grad.hip: the generic adjoint k_adj runs one thread per unit of the widest layer, (max_dim + 63) & ~63 <= 1024,
    and keeps AdjLds::per_sample floats (+ one per wave) of LDS per sample, <= 160 KB."""
    in0 = dims[0] + n_cond
    sum_in = in0 + sum(dims[1:-1])
    sum_out = sum(dims[1:])
    mx = max([in0] + list(dims[1:]))
    threads = (mx + 63) & ~63
    per_sample = 2 * (sum_in + dims[-1]) + 3 * sum_out + 2 * mx + dims[0]
    return threads <= 1024 and (per_sample + threads // 64) * 4 <= LDS_160K


def jvp_mfma_supported(dims, jvp, n_cond=0):
    """cnf_trace.hip: k_jvp_mfma (TrainMode, JVP compute mode, beyond k_mfma's plan): two ping-pong buffers of 32 columns
    of PX = pad8m16(maxd) floats, the eps tile and the reduction rows, <= 160 KB."""
    if not jvp:
        return False
    m = _adj_layout(dims, n_cond)
    total = 2 * 32 * pad8m16(m["maxd"]) + 16 * (m["nin_p"] + 8) + 3 * 32 * 16
    return total * 4 <= LDS_160K


def trace_mfma_supported(dims, n_cond=0):
    """cnf_trace.hip: k_trace_mfma (TestMode, three or more layers): at most 8 column tiles per sample (n_in <= 128) and
    ``trace_layout``'s total <= 160 KB."""
    m = _adj_layout(dims, n_cond)
    L = m["L"]
    if L < 3 or m["nin_p"] // 16 > 8:
        return False
    PD, PT = pad8m16(m["sum_o"]), pad8m16(max([16] + m["dp"][1:L]))
    PSf = pad8m16(m["maxd"])
    nbuf = 2 if L >= 4 else 1
    per = m["nin_p"] // 16
    gs, g = 1, 16
    while g >= 1:
        c = g * per
        fl = 16 * PD + nbuf * 16 * c * PT + 16 * 8
        if c <= 8 and (fl * 4 <= 80 * 1024 or g == 1):
            gs = g
            break
        g //= 2
    nct = gs * per
    region = max(nbuf * 16 * nct * PT, 2 * 16 * PSf)
    return (16 * PD + region + 16 * 8) * 4 <= LDS_160K


def wave_shape(dims):
    """csrc/cnf_wave_variants.h ``WF_PLAIN``: two-layer networks of (input tiles, hidden tiles) = (1, 1..4) or (2, 6)."""
    if len(dims) != 3:
        return False
    ni, nh = (dims[0] + 15) // 16, (dims[1] + 15) // 16
    return (ni == 1 and 1 <= nh <= 4) or (ni == 2 and nh == 6)


def wave_grad_shape(dims, acts, n_cond=0):
    """cnf_wave.hip ``wave_grad_supported`` (its shape part): one input tile, tanh first, tanh or identity second, the
    conditioning rows within the input tile."""
    if not wave_shape(dims) or (dims[0] + 15) // 16 != 1:
        return False
    if acts[0] != T or acts[1] not in (T, ID):
        return False
    if acts[1] == ID and (dims[1] + 15) // 16 != 1:
        return False
    return not (n_cond > 0 and dims[0] + n_cond > 16)


def bcast_shape(dims, acts):
    """cnf_bcast.hip ``bcast_solve_supported`` (its shape part): tanh-tanh, 64 < n_in <= 128, 256 < hidden <= 384."""
    return len(dims) == 3 and tuple(acts) == (T, T) and 64 < dims[0] <= 128 and 256 < dims[1] <= 384


def expected_route(dims, acts, jvp, train, n_cond=0):
    """Which RHS kernel ``kernel = auto`` resolves to (cnf_abi.hip ``resolve_kernel``): "mfma-lds" / "mfma-streamed"
    (k_mfma with that plan; TestMode: two-layer networks only, the closed-form trace), "jvp-mfma" (k_jvp_mfma),
    "trace-mfma" (k_trace_mfma) or "generic"."""
    plan, _ = mfma_lds_bytes(dims, jvp, acts)
    if plan != "none" and (train or len(dims) == 3):
        return "mfma-" + plan
    if train:
        return "jvp-mfma" if jvp_mfma_supported(dims, jvp, n_cond) else "generic"
    return "trace-mfma" if trace_mfma_supported(dims, n_cond) else "generic"


# ---------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    family: str                 # "a" plan edges, "b" other predicates, "c" activation matrix, "d" regimes
    dims: tuple                 # (n_in, h1, ..., n_in): without the conditioning inputs
    acts: tuple
    nvars: int
    naugs: int
    B: int
    seed: int
    jvp: bool = False
    n_cond: int = 0
    scale: float = 0.1          # bias scale of glorot_params
    wscale: float = 1.0         # factor on the Glorot weights
    xs_scale: float = 1.0       # factor on the data (and on the RHS state)
    steps: int = 4              # fixed steps over tspan = (0, 1)
    route: str = ""             # expected_route(TrainMode) -- written out, checked against the restatement and the device
    route_test: str = ""        # expected_route(TestMode)
    one_launch: object = None   # True / False: last_stats["launches"] <= 3 of a TrainMode inference separates the sides of the
    #                             bound (as tests/test_gpu_parity.py reads it); None: nothing observable, numbers only
    grad: bool = True           # loss_and_grad is part of the case (False: listed in NO_GRADIENT with the reason)
    test_solve: bool = True     # TestMode inference is part of the case (the exact-trace oracle costs n_in sweeps per evaluation)
    note: str = ""

    @property
    def net(self):
        return O.Net((self.dims[0] + self.n_cond,) + tuple(self.dims[1:]), tuple(self.acts))

    @property
    def dt(self):
        return 1.0 / self.steps

    @property
    def test_grad(self):
        """The TestMode loss gradient is part of the case: the activation matrix and the regimes, on networks the exact-trace
        oracle's per-sample Jacobian products stay cheap for."""
        return self.grad and self.test_solve and self.family in "cd" and max(self.dims) <= 128

    def cfg(self, lam=(1e-2, 1e-2, 1e-2)):
        return O.Cfg(self.net, self.nvars, self.naugs, lam[0], lam[1], lam[2] if self.naugs else 0.0, use_jvp=self.jvp, tspan=(0.0, 1.0))

    def inputs(self):
        """(flat, xs, eps, ys, u_train) in float32."""
        rng = np.random.default_rng(self.seed)
        flat = O.glorot_params(self.net, rng, np.float32, self.scale)
        if self.wscale != 1.0:
            w = np.ones(flat.size, np.float32)
            off = 0
            for i, o in zip(self.net.dims[:-1], self.net.dims[1:]):
                w[off:off + i * o] = self.wscale
                off += i * o + o
            flat = flat * w
        n_in = self.nvars + self.naugs
        xs = (rng.standard_normal((self.nvars, self.B)) * self.xs_scale).astype(np.float32)
        eps = rng.standard_normal((n_in, self.B)).astype(np.float32)
        ys = rng.standard_normal((self.n_cond, self.B)).astype(np.float32) if self.n_cond else None
        u = rng.standard_normal((n_in + 3, self.B)).astype(np.float32)
        u[:n_in] *= self.xs_scale
        return flat, xs, eps, ys, u


def _routes(dims, acts, jvp, n_cond=0):
    return dict(route=expected_route(dims, acts, jvp, True, n_cond), route_test=expected_route(dims, acts, jvp, False, n_cond))


def plan_edges(L, jvp, n_in=32):
    """For equal hidden widths h (multiples of 16) and ``n_in``: (last h with the weights in LDS, first streamed h,
    last streamed h, first h without a k_mfma plan), from ``mfma_lds_bytes``."""
    plan = lambda h: mfma_lds_bytes((n_in,) + (h,) * (L - 1) + (n_in,), jvp)[0]
    h = 16
    while plan(h + 16) == "lds":
        h += 16
    s = h + 16
    while plan(s + 16) == "streamed":
        s += 16
    return h, h + 16, s, s + 16


def _family_a():
    cs = []
    seed = 2000
    for L in (2, 3, 4, 8):
        for jvp in (False, True):
            edges = plan_edges(L, jvp)
            for k, h in enumerate(edges):
                seed += 1
                dims = (32,) + (h,) * (L - 1) + (32,)
                # one ragged multi-workgroup batch in the family (the first streamed width of the 3-layer VJP network),
                # a single sample and one sample more than a 32-sample tile on two others
                B = 100 if (L, jvp, k) == (3, False, 1) else 1 if (L, jvp, k) == (2, True, 1) else 33 if (L, jvp, k) == (4, False, 2) else 17
                wide = max(dims) > 1024
                # Nothing observable separates the LDS plan from the streamed one (both are step launches of k_mfma<RtLayout>
                # reported as MFMA): numbers only on that edge.  The streamed | beyond edge shows in cnf_kernel_for /
                # kernel_used in the VJP compute mode (generic beyond); in the JVP mode k_jvp_mfma takes over: numbers only.
                # One exception: the last LDS width of the 3-layer VJP network IS 32-128-128-32, which matches the static
                # LyCfg3 layout and runs the headline kernels (one-launch solve, k_adj3b), not k_mfma<RtLayout>; the run-time
                # layout beside the first streamed width is a-L3-vjp-unaligned-lds below (pads to 32-112-112-32).
                headline = (L, jvp, k) == (3, False, 0)
                cs.append(Case(f"a-L{L}-{'jvp' if jvp else 'vjp'}-h{h}-{('lds-last', 'streamed-first', 'streamed-last', 'beyond')[k]}", "a",
                               dims, (T,) * L, 32, 0, B, seed, jvp=jvp, one_launch=True if headline else None,
                               steps=2 if max(dims) > 400 else 4, grad=not wide, test_solve=max(dims) <= 400,
                               **_routes(dims, (T,) * L, jvp),
                               note="the static headline layout, not RtLayout" if headline else "K ~ %d" % max(dims)))
    # the two state-width edges of the plan
    cs += [
        Case("a-128x64x128-jvp-192-bytes-under", "a", (128, 64, 128), (T, T), 100, 28, 17, 2101, jvp=True, **_routes((128, 64, 128), (T, T), True)),
        Case("a-129x64x129-jvp-state-rows", "a", (129, 64, 129), (T, T), 100, 29, 17, 2102, jvp=True, **_routes((129, 64, 129), (T, T), True)),
        Case("a-129x64x129-vjp-state-rows", "a", (129, 64, 129), (T, T), 100, 29, 17, 2103, **_routes((129, 64, 129), (T, T), False)),
    ]
    # unaligned versions: widths = 1 and 15 mod 16 on either side of an edge, n_in not a multiple of 16; an augmented and a
    # conditional model among the streamed ones
    l3 = plan_edges(3, False)
    l2j = plan_edges(2, True)
    l4 = plan_edges(4, False)
    l8j = plan_edges(8, True)

    def un(name, dims, acts, nvars, naugs, B, seed, **kw):
        jvp, nc = kw.get("jvp", False), kw.get("n_cond", 0)
        return Case(name, "a", dims, acts, nvars, naugs, B, seed, steps=2 if max(dims) > 400 else 4,
                    test_solve=max(dims) <= 400, **_routes(dims, acts, jvp, nc), **kw)
    cs += [
        # (one 16-block below the edge: widths that pad to 128 would match the static 32-128-128-32 layout; 97 / 111 pad to 112
        # and run k_mfma<RtLayout> with the weights in LDS -- step launches)
        un("a-L3-vjp-unaligned-lds", (30, l3[0] - 31, l3[0] - 17, 30), (T,) * 3, 20, 10, 17, 2111, one_launch=False),
        un("a-L3-vjp-unaligned-streamed-aug", (30, l3[1] - 15, l3[1] - 1, 30), (T,) * 3, 20, 10, 33, 2112),
        un("a-L2-jvp-unaligned-lds", (24, l2j[0] - 15, 24), (T,) * 2, 24, 0, 17, 2113, jvp=True),
        un("a-L2-jvp-unaligned-streamed-cond", (24, l2j[1] - 15, 24), (T,) * 2, 24, 0, 17, 2114, jvp=True, n_cond=5),
        un("a-L4-vjp-unaligned-streamed-last", (17, l4[2] - 15, l4[2] - 1, l4[2] - 15, 17), (T,) * 4, 17, 0, 17, 2115),
        un("a-L4-vjp-unaligned-beyond", (17, l4[3] - 15, l4[3] - 1, l4[3] - 15, 17), (T,) * 4, 17, 0, 17, 2116),
        un("a-L8-jvp-unaligned-streamed-last-cond", (31,) + (l8j[2] - 1, l8j[2] - 15) * 3 + (l8j[2] - 1, 31), (T,) * 8, 25, 6, 17, 2117,
           jvp=True, n_cond=2),
        # eight layers of mixed widths: streamed in the VJP compute mode
        un("a-L8-vjp-mixed-widths", (32, 64, 96, 48, 80, 33, 64, 47, 32), (T, SP, T, SG, T, EL, T, T), 24, 8, 33, 2118),
    ]
    return cs


def _family_b():
    cs = []

    def c(name, dims, acts, nvars, naugs, B, seed, **kw):
        jvp, nc = kw.get("jvp", False), kw.get("n_cond", 0)
        cs.append(Case(name, "b", dims, acts, nvars, naugs, B, seed, **_routes(dims, acts, jvp, nc), **kw))

    # grad_supported: (max_dim + 63) & ~63 <= 1024 threads of k_adj.  (Its LDS bound, per_sample floats <= 160 KB, is not
    # reachable before the thread bound: eight layers of 1024 units need 38 016 floats of the 40 960.)  Outside it the
    # library refuses the gradient (CNF_ERR_UNSUPPORTED); RHS and inference are unaffected.  Streamed forward, so
    # adj_mfma_supported is false as well: k_adj is the pullback inside.
    c("b-grad-inside-1024", (16, 1024, 16), (T, T), 16, 0, 17, 2201, steps=2, test_solve=False)
    c("b-grad-outside-1025", (16, 1025, 16), (T, T), 16, 0, 17, 2202, steps=2, test_solve=False, grad=False,
      note="gradient refused (grad_supported): asserted")
    # adj_mfma_supported: 3 sum_o + 2 maxd + nin_p <= 2520 floats (PS <= 2528 = (160 KB / 4 - 512) / 16).  Two layers, n_in = 16:
    # sum_o = hp + 16, maxd = hp -> 5 hp + 64 <= 2520 -> hp <= 480.  Nothing observable separates k_adj_mfma from k_adj.
    c("b-adj-mfma-inside-480", (16, 480, 16), (T, SP), 10, 6, 33, 2203)
    c("b-adj-mfma-outside-481", (16, 481, 16), (T, SP), 10, 6, 33, 2204)
    # trace_mfma_supported: n_in <= 128 (8 column tiles per sample) ...
    c("b-trace-inside-128", (128, 48, 48, 128), (T, T, T), 128, 0, 17, 2205, steps=2)
    c("b-trace-outside-129", (129, 48, 48, 129), (T, T, T), 129, 0, 17, 2206, steps=2)
    # ... and trace_layout's LDS total <= 160 KB.  For 32-h-h-32 (one buffer; beyond 80 KB the groups shrink to one sample =
    # two column tiles) it is 16 pad8m16(2 hp + 32) + 32 (hp + 8) + 128 floats = 64 hp + 1024 <= 40960 -> hp <= 624:
    # TRACE_EDGE below finds the same from the restatement.
    c("b-trace-lds-inside", (32, TRACE_EDGE[0], TRACE_EDGE[0], 32), (T, SG, T), 32, 0, 17, 2207, steps=2)
    c("b-trace-lds-outside", (32, TRACE_EDGE[1], TRACE_EDGE[1], 32), (T, SG, T), 32, 0, 17, 2208, steps=2)
    # jvp_mfma_supported: 64 PX + 16 (nin_p + 8) + 1536 floats <= 40960 with PX = pad16(maxd) + 8; n_in = 32: pad16(maxd) <= 592
    c("b-jvp-mfma-inside-592", (32, 592, 592, 32), (T, T, T), 32, 0, 17, 2209, jvp=True, steps=2, test_solve=False)
    c("b-jvp-mfma-outside-593", (32, 593, 593, 32), (T, T, T), 32, 0, 17, 2210, jvp=True, steps=2, test_solve=False)
    # wave_solve_supported: (input tiles, hidden tiles) in {(1, 1..4), (2, 6)}: 64 hidden units inside, 65 outside (k_mfma)
    c("b-wave-inside-64", (16, 64, 16), (T, T), 8, 8, 33, 2211, one_launch=True)
    c("b-wave-outside-65", (16, 65, 16), (T, T), 8, 8, 33, 2212, one_launch=False)
    c("b-wave-inside-32x96", (32, 96, 32), (T, T), 32, 0, 17, 2213, one_launch=True)
    c("b-wave-outside-32x80", (32, 80, 32), (T, T), 32, 0, 17, 2214, one_launch=False)
    # wave_grad_supported: one input tile and tanh first: 16 inputs inside; 17 inputs (two input tiles: no wave shape with 48
    # hidden units at all) and a softplus first layer (wave solve, streamed gradient) outside
    c("b-wave-grad-inside", (16, 48, 16), (T, T), 16, 0, 17, 2215, one_launch=True)
    c("b-wave-grad-outside-softplus", (16, 48, 16), (SP, T), 16, 0, 17, 2216, one_launch=True)
    # bcast_solve_supported, shape bound only (its residency bound depends on the device's CU count):
    # tanh-tanh, 64 < n_in <= 128 and 256 < hidden <= 384
    c("b-bcast-inside-65x257", (65, 257, 65), (T, T), 40, 25, 17, 2217, one_launch=True, steps=4)
    c("b-bcast-outside-64x257", (64, 257, 64), (T, T), 40, 24, 17, 2218, one_launch=False, steps=4)
    c("b-bcast-outside-65x256", (65, 256, 65), (T, T), 40, 25, 17, 2219, one_launch=False, steps=4)
    c("b-bcast-inside-128x384-cond", (128, 384, 128), (T, T), 100, 28, 9, 2220, one_launch=True, n_cond=3, steps=4)
    c("b-bcast-outside-128x385", (128, 385, 128), (T, T), 100, 28, 9, 2221, one_launch=False, steps=4)
    # trace_solve_supported / trace_fused_supported: the 32-128-128-32 shape only (its CU-count bound is the device's):
    # the headline network inside (three launches per TestMode inference), 32-128-112-32 outside.  TrainMode: the one-launch
    # headline solve inside, k_mfma step launches outside.
    c("b-trace-solve-inside-headline", (32, 128, 128, 32), (T, T, T), 32, 0, 33, 2222, one_launch=True)
    c("b-trace-solve-outside-112", (32, 128, 112, 32), (T, T, T), 32, 0, 33, 2223, one_launch=False)
    return cs


def _trace_edge():
    h = 16
    while trace_mfma_supported((32, h + 16, h + 16, 32)):
        h += 16
    return h, h + 16


TRACE_EDGE = _trace_edge()

# routes of the activation matrix: a shape per route, every activation in a hidden and in the last position
STREAMED_L3 = plan_edges(3, False)[1]
STREAMED_L3_JVP = plan_edges(3, True)[1]
ACT_ROUTES = {
    # route: (dims, nvars, naugs, B, jvp, n_cond)
    "generic": ((5, 7, 3, 5), 3, 2, 17, False, 0),                      # (kernel = generic on every case as well)
    "mfma-lds": ((20, 72, 40, 20), 12, 8, 33, False, 0),
    "mfma-lds-jvp": ((20, 72, 40, 20), 12, 8, 17, True, 0),
    "mfma-streamed": ((32, STREAMED_L3, STREAMED_L3, 32), 32, 0, 17, False, 0),
    "wave": ((12, 40, 12), 8, 4, 33, False, 0),                        # k_solve_wave<.., TANH = false> unless both are tanh
    "trace-mfma": ((24, 48, 40, 24), 24, 0, 17, False, 0),              # TestMode: k_trace_mfma; pullbacks: k_adj_mfma / k_adj_test
    "headline-shape": ((32, 128, 128, 32), 32, 0, 33, False, 0),        # k_adj3 (not all-tanh) / k_adj3b (tanh)
    # the JVP compute mode on the other routes: k_mfma streamed with tangent images, the wave kernel, the headline shape
    # (k_step3j only when all-tanh; k_adj_mfma<JVP> as the pullback), and k_jvp_mfma beyond the plan (more than 128 state rows)
    "mfma-streamed-jvp": ((32, STREAMED_L3_JVP, STREAMED_L3_JVP, 32), 32, 0, 17, True, 0),
    "wave-jvp": ((12, 40, 12), 8, 4, 33, True, 0),
    "headline-shape-jvp": ((32, 128, 128, 32), 32, 0, 33, True, 0),
    "jvp-mfma": ((129, 48, 129), 100, 29, 17, True, 0),
}
# Left out of the matrix, with the reason: conditional models (the conditioning columns only add to the first layer's
# pre-activation, in front of every activation: families (a) and (b) carry them); k_solve_bcast (tanh-tanh only by its
# predicate); the exact-trace solve k_trace3s with other activations than tanh is the headline-shape route's TestMode half.


def _family_c():
    cs = []
    seed = 2300
    for route, (dims, nvars, naugs, B, jvp, nc) in ACT_ROUTES.items():
        L = len(dims) - 1
        for a in ACTS:
            for pos in ("hidden", "last"):
                seed += 1
                acts = [T] * L
                acts[0 if pos == "hidden" else L - 1] = a
                acts = tuple(acts)
                if a == T and pos == "last":
                    continue                                            # (all-tanh: the hidden-position case already)
                wide = max(dims) > 128
                routes = _routes(dims, acts, jvp, nc)
                # the wave kernel took it: one launch, as tests/test_gpu_parity.py reads it (swish in a hidden layer has no
                # MFMA kernel in the VJP mode: generic step launches; in the JVP mode it is left to the numbers)
                one = (routes["route"].startswith("mfma") or None) if route.startswith("wave") else None
                if route.startswith("wave") and routes["route"] == "generic":
                    one = False
                cs.append(Case(f"c-{route}-{NAME[a]}-{pos}", "c", dims, acts, nvars, naugs, B, seed, jvp=jvp, n_cond=nc,
                               scale=0.3, steps=2 if wide else 4, test_solve=not wide, one_launch=one, **routes,
                               note="swish hidden: the generic kernel" if (a == SW and pos == "hidden") else ""))
    return cs


# pre-activation regimes: (xs / state scale, bias scale).  tiny: pre-activations ~ 1e-3 in the first layer (and in all of
# them for the activations with s(0) = 0); saturated: |a| ~ 20..40 in the first layer (std 25: both sides of softplus's
# switch at 15), and in the later ones for the unbounded activations.
REGIMES = {"tiny": (1e-3, 0.0), "unit": (1.0, 0.3), "saturated": (40.0, 0.3)}
REGIME_NETS = {
    # the headline network: tanh_fast in the step kernels, k_adj3b as the pullback (VJP), k_step3j / k_solve3jb (JVP)
    "headline": ((32, 128, 128, 32), (T, T, T), 32, 0, 33, False),
    "headline-jvp": ((32, 128, 128, 32), (T, T, T), 32, 0, 33, True),
    # the accurate cnf_tanh: k_mfma's run-time layout
    "rt-tanh": ((32, 128, 112, 32), (T, T, T), 32, 0, 33, False),
    "rt-softplus-elu": ((20, 72, 40, 20), (SP, EL, T), 12, 8, 17, False),
    "rt-sigmoid-swish": ((20, 72, 40, 20), (SG, T, SW), 12, 8, 17, False),
    "wave-elu-softplus": ((12, 40, 12), (EL, SP), 8, 4, 33, False),
    "generic-swish-relu": ((5, 7, 3, 5), (SW, RE, EL), 3, 2, 17, False),
    "generic-softplus": ((5, 7, 3, 5), (SP, SP, T), 3, 2, 17, False),
}


def _family_d():
    cs = []
    seed = 2500
    for net, (dims, acts, nvars, naugs, B, jvp) in REGIME_NETS.items():
        for regime, (xscale, bscale) in REGIMES.items():
            seed += 1
            cs.append(Case(f"d-{net}-{regime}", "d", dims, acts, nvars, naugs, B, seed, jvp=jvp, scale=bscale, xs_scale=xscale,
                           one_launch=True if net.startswith("headline") or net.startswith("wave") else None,
                           **_routes(dims, acts, jvp)))
    return cs


def _cases():
    return _family_a() + _family_b() + _family_c() + _family_d()


CASES = {c.name: c for c in _cases()}
assert len(CASES) == len(_cases()), "duplicate case names"
NO_GRADIENT = {c.name: ("hidden width beyond the 1024 threads of the generic adjoint: the library refuses the gradient (asserted)"
                        if max(c.dims) > 1024 else c.note) for c in CASES.values() if not c.grad}


def by_family(f):
    return [c for c in CASES.values() if c.family == f]


def model(case, kernel="auto"):
    """The host-side model of ``case`` (RNODE / CondRNODE with lam = 1e-2, fixed steps); building it needs no device."""
    import continuousnf.jl_amd as cnf
    net = case.net
    layers = [cnf.Dense(a, b, helpers.ACT_NAME[k]) for a, b, k in zip(net.dims[:-1], net.dims[1:], net.acts)]
    cm = cnf.HIPJacVecMatrixMode(kernel) if case.jvp else cnf.HIPVecJacMatrixMode(kernel)
    return cnf.construct(cnf.CondRNODE if case.n_cond else cnf.RNODE, cnf.Chain(*layers), case.nvars, case.naugs, compute_mode=cm,
                         tspan=(0.0, 1.0), lambda1=1e-2, lambda2=1e-2, lambda3=1e-2 if case.naugs else 0.0,
                         sol_kwargs=dict(adaptive=False, dt=case.dt), rng=0)


# ---------------------------------------------------------------------------------------
# references and floors
# ---------------------------------------------------------------------------------------
def _c(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


@lru_cache(maxsize=None)
def references(name, dtype_name="float64", lam=(1e-2, 1e-2, 1e-2)):
    """The oracle's numbers for case ``name`` in ``dtype``: dict with du_train, du_test (None without test_solve ...),
    logpx / regs of a fixed-step TrainMode inference, logpx_test, and (loss, grad, grad_x) where the case has a gradient."""
    case = CASES[name]
    dtype = np.dtype(dtype_name).type
    cfg = case.cfg(lam)
    flat, xs, eps, ys, u = (_c(a, dtype) for a in case.inputs())
    n_in = cfg.n_in
    out = dict(du_train=cfg.rhs(flat, eps, True, ys)(u))
    out["du_test"] = cfg.rhs(flat, None, False, ys)(u[:n_in + 1]) if case.test_solve else None
    _, lp, regs, st = O.inference(cfg, flat, xs, eps, True, ys, dt=case.dt, adaptive=False)
    out["logpx"], out["regs"] = lp, np.stack([np.asarray(r) for r in regs])
    assert st.naccept == case.steps, (name, st.naccept)
    if case.test_solve:
        _, lpt, _, _ = O.inference(cfg, flat, xs, None, False, ys, dt=case.dt, adaptive=False)
        out["logpx_test"] = lpt
    if case.grad:
        val, grad, gst = G.loss_and_grad(cfg, flat, xs, eps, ys, dts=[case.dt] * case.steps)
        out["loss"], out["grad"], out["grad_x"] = float(val), np.asarray(grad), np.asarray(gst.grad_x)
    if case.test_grad:
        val, grad, gst = G.loss_and_grad_test(cfg, flat, xs, ys, dts=[case.dt] * case.steps)
        out["loss_test"], out["grad_test"], out["grad_x_test"] = float(val), np.asarray(grad), np.asarray(gst.grad_x)
    return out


def grad_err(got, ref):
    """max|got - ref| over (max|ref| + rms ref): the whole-gradient bar of the other gradient tests, as a ratio."""
    ref = np.asarray(ref, dtype=np.float64)
    s = float(np.abs(ref).max() + np.sqrt(np.mean(ref * ref)))
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if not np.isfinite(d).all():
        return np.inf
    return float(d.max()) / s if s > 0 else (0.0 if d.max() == 0 else np.inf)


def _state_err(got, ref, n_in):
    return helpers.parity_err(got, ref, helpers.RTOL, None, n_in if np.ndim(ref) == 2 and np.shape(ref)[0] > n_in else None)


def compare(got, ref, n_in):
    """quantity -> error of ``got`` against ``ref`` (both ``references``-shaped dicts; missing keys skipped) as the rtol at
    which it would just meet its bar."""
    out = {}
    for k in ("du_train", "du_test"):
        if got.get(k) is not None and ref.get(k) is not None:
            out[k] = helpers.RTOL * _state_err(got[k], ref[k], n_in)
    for k in ("logpx", "regs", "logpx_test"):
        if got.get(k) is not None and ref.get(k) is not None:
            out[k] = helpers.RTOL * helpers.parity_err(got[k], ref[k], helpers.RTOL)
    for k in ("grad", "grad_x", "grad_test", "grad_x_test"):
        if got.get(k) is not None and ref.get(k) is not None:
            out[k] = grad_err(got[k], ref[k])
    return out


@lru_cache(maxsize=None)
def floors(name):
    """quantity -> float32 floor of case ``name``: the numpy float32 oracle (and the C float32 oracle for the RHS of the
    unconditional cases) against the numpy float64 oracle."""
    case = CASES[name]
    r64, r32 = references(name, "float64"), references(name, "float32")
    n_in = case.nvars + case.naugs
    fl = compare(r32, r64, n_in)
    if not case.n_cond:
        flat, xs, eps, ys, u = case.inputs()
        c = dict(du_train=CO.rhs(case.cfg(), flat, u, eps, True))
        if case.test_solve:
            c["du_test"] = CO.rhs(case.cfg(), flat, u[:n_in + 1], None, False)
        for k, v in compare(c, r64, n_in).items():
            fl[k] = max(fl[k], v)
    return fl


def rtol_of(floor):
    return max(helpers.RTOL, FLOOR_FACTOR * floor)


def rtols(name):
    return {k: rtol_of(v) for k, v in floors(name).items()}


# ---------------------------------------------------------------------------------------
# mutants of the oracle: what the activation matrix and the regimes must be able to see
# ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def mutant(which):
    """The oracle with one deliberate mistake: "swish-d2" (the a ds (1 - 2 s) part of swish's second derivative dropped),
    "elu-d1" (elu' = 1 + a instead of exp(a) for a < 0), "softplus-5" (softplus(a) = a from a > 5 on, not 15)."""
    keep_d2, keep_act = G.act_d2, O.act_apply

    def d2(kind, a):
        if which == "swish-d2" and kind == SW:
            s = O._sigmoid(a)
            return 2 * s * (1 - s)
        return keep_d2(kind, a)

    def act(kind, a):
        h, d = keep_act(kind, a)
        if which == "elu-d1" and kind == EL:
            d = np.where(a > 0, np.ones_like(a), 1 + np.minimum(a, 0))
        if which == "softplus-5" and kind == SP:
            h = np.where(a > 5, a, h)
        return h, d

    G.act_d2, O.act_apply = d2, act
    try:
        yield
    finally:
        G.act_d2, O.act_apply = keep_d2, keep_act


def mutant_references(name, which):
    with mutant(which):
        return references.__wrapped__(name, "float64")
