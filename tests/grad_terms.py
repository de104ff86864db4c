"""Pinning each regulariser term of the loss gradient at its own scale (helper module; no GPU needed).

The TrainMode loss is mean_b(-logpx + lam1 E + lam2 n + lam3 A).  For a fixed step sequence its gradient is affine in
(lam1, lam2, lam3):  g(lam) = g(0) + sum_k lam_k (g(e_k) - g(0)),  so the share of one term is  part_k = g(e_k) - g(0)  and a
run with the one-hot lam = e_k can be compared at the scale of that share instead of the scale of the whole gradient
(at lam = 0.01, where the other gradient tests run, the three shares are ~1 % of the gradient and a bar of 1e-4 of the whole
checks them ~100 times more loosely than it checks the log-density term).

    bar per parameter block (W1, b1, ...) and for d loss / d xs:
        max|got(e_k) - ref64(e_k)|  <=  rtol * (max|part_k| + rms part_k),       part_k restricted to the block
        rtol = max(helpers.RTOL, 8 * floor) <= 1e-3,
        floor = max|ref32(e_k) - ref64(e_k)| / (max|part_k| + rms part_k)        (float32 run of the SAME oracle)

The floor is what float32 arithmetic of the same discrete map costs, taken from the oracle and never from the device; the
factor 8 covers what the oracle's float32 run does not have (the device's summation order, its split-bf16 products).  The
cap 1e-3 is a condition: a case whose floor would ask for more is a finding, not a reason to raise it.
"""
from __future__ import annotations

import contextlib
import dataclasses
import hashlib
import os
from dataclasses import dataclass

import numpy as np

from oracle import cnf_grad_oracle as G
from oracle import cnf_oracle as O
from tests import helpers

TERM_NAMES = {1: "lam1", 2: "lam2", 3: "lam3"}
FLOOR_FACTOR = 8.0
RTOL_CAP = 1e-3
FLOOR_MAX = RTOL_CAP / FLOOR_FACTOR          # 1.25e-4: 8 x floor stays under the cap

RECORDS = []        # one dict per (case, term, block) checked by assert_grad_term: the summary table is made of them


def one_hot(k):
    """lam = e_k (k = 1..3); k = 0: all zero."""
    return tuple(1.0 if j == k else 0.0 for j in (1, 2, 3))


def param_blocks(net, n_cond=0):
    """name -> slice of the flat parameter vector: W1, b1, W2, b2, ... in the layout of ``flatten_grads`` (per layer the
    weight, out x in column-major, then the bias).  ``n_cond``: conditioning inputs to add to the first layer's fan-in
    when ``net`` is the unconditional network."""
    dims = (net.dims[0] + n_cond,) + tuple(net.dims[1:])
    blocks, off = {}, 0
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:]), 1):
        blocks[f"W{l}"] = slice(off, off + i * o)
        off += i * o
        blocks[f"b{l}"] = slice(off, off + o)
        off += o
    return blocks


def block_entry(net, name, idx):
    """Where entry ``idx`` of block ``name`` sits: "row r col c" of the out x in weight (column-major), or "row r"."""
    out = net.dims[int(name[1:])]
    return f"row {idx % out} col {idx // out}" if name[0] == "W" else f"row {idx}"


# ---------------------------------------------------------------------------------------
# the cases: one table for the host suite (floors) and the GPU suite (the device against them)
# ---------------------------------------------------------------------------------------
TOL32 = (("reltol", float(np.sqrt(np.finfo(np.float32).eps))), ("abstol", float(np.finfo(np.float32).eps)))
T = O.ACT_TANH


@dataclass(frozen=True)
class Case:
    name: str
    route: str
    dims: tuple
    acts: tuple
    nvars: int
    naugs: int
    B: int
    seed: int
    tspan: tuple = (0.0, 0.5)
    steps: tuple = ("fixed", 0.25)      # ("fixed", dt) or ("adaptive", ((key, value), ...) of the controller)
    jvp: bool = False
    n_cond: int = 0
    scale: float = 0.1                  # bias scale of glorot_params
    kernel: str = "mfma"
    xs_scale: float = 1.0

    @property
    def terms(self):
        return (1, 2, 3) if self.naugs > 0 else (1, 2)

    @property
    def net(self):
        """The network the oracle runs: conditioning inputs included in the first fan-in."""
        return O.Net((self.dims[0] + self.n_cond,) + tuple(self.dims[1:]), tuple(self.acts))

    def cfg(self, lam):
        return O.Cfg(self.net, self.nvars, self.naugs, float(lam[0]), float(lam[1]), float(lam[2]) if self.naugs else 0.0,
                     use_jvp=self.jvp, tspan=self.tspan)

    @property
    def sol_kw(self):
        """sol_kwargs of the device model; also the arguments of the oracle's own solve."""
        return dict(adaptive=False, dt=self.steps[1]) if self.steps[0] == "fixed" else dict(self.steps[1])

    def inputs(self):
        """(flat, xs, eps, ys) in float32, drawn in the order of the other gradient tests' ``_grad_case``."""
        rng = np.random.default_rng(self.seed)
        flat = O.glorot_params(self.net, rng, np.float32, self.scale)
        xs = (rng.standard_normal((self.nvars, self.B)) * self.xs_scale).astype(np.float32)
        eps = rng.standard_normal((self.nvars + self.naugs, self.B)).astype(np.float32)
        ys = rng.standard_normal((self.n_cond, self.B)).astype(np.float32) if self.n_cond else None
        return flat, xs, eps, ys


def _headline(name, route, B, seed, steps=("fixed", 0.25), **kw):
    return Case(name, route, (32, 128, 128, 32), (T,) * 3, 32, 0, B, seed, steps=steps, **kw)


def _cases():
    cs = [
        # k_solve_wave<GRAD>: small two-layer tanh networks, everything in one launch
        Case("wave-16x48-B32-replay", "wave", (16, 48, 16), (T,) * 2, 8, 8, 32, 1001, tspan=(0.0, 1.0), steps=("adaptive", ()), scale=0.3),
        Case("wave-16x48-B77-replay", "wave", (16, 48, 16), (T,) * 2, 8, 8, 77, 1002, tspan=(0.0, 1.0), steps=("adaptive", TOL32), scale=0.3),
        Case("wave-7x13-B1-backward", "wave", (7, 13, 7), (T,) * 2, 4, 3, 1, 1003, tspan=(1.0, 0.0), scale=0.3),
        Case("wave-16x48-B32-jvp", "wave", (16, 48, 16), (T,) * 2, 8, 8, 32, 1004, tspan=(0.0, 1.0), steps=("adaptive", ()), jvp=True, scale=0.3),
        Case("wave-6x18-B40-cond", "wave", (6, 18, 6), (T,) * 2, 4, 2, 40, 1005, tspan=(0.0, 1.0), steps=("fixed", 0.125), n_cond=3, scale=0.3),
    ]
    # k_adj3b (both launch forms): the headline shape, tile edges of its 32-sample tiles
    for B in (1, 17, 33, 77, 300):
        cs.append(_headline(f"adj3b-B{B}-fixed", "adj3b", B, 1100 + B))
        cs.append(_headline(f"adj3b-B{B}-replay", "adj3b", B, 1500 + B, steps=("adaptive", TOL32)))
    cs += [
        # k_adj3: shapes that pad to the headline shape but are not all-tanh / unconditional
        Case("adj3-30x120x116-aug", "adj3", (30, 120, 116, 30), (T, O.ACT_ELU, T), 20, 10, 33, 1201),
        Case("adj3-softplus-sigmoid", "adj3", (32, 128, 128, 32), (O.ACT_SOFTPLUS, O.ACT_SIGMOID, T), 32, 0, 45, 1202),
        Case("adj3-28x128x128-cond", "adj3", (28, 128, 128, 28), (T,) * 3, 28, 0, 70, 1203, n_cond=4),
        # k_adj_mfma<., VJP> / <., JVP> (both launch forms)
        Case("mfma-cfg5-vjp", "adj_mfma", (128, 384, 128), (T,) * 2, 64, 64, 40, 1301),
        Case("mfma-cfg5-jvp", "adj_mfma", (128, 384, 128), (T,) * 2, 64, 64, 40, 1302, jvp=True),
        Case("mfma-12x64x48-cond-vjp", "adj_mfma", (12, 64, 48, 12), (T, O.ACT_SOFTPLUS, T), 8, 4, 50, 1303, n_cond=3, scale=0.3),
        Case("mfma-12x64x48-cond-jvp", "adj_mfma", (12, 64, 48, 12), (T, O.ACT_SOFTPLUS, T), 8, 4, 50, 1304, n_cond=3, scale=0.3, jvp=True),
        _headline("mfma-headline-jvp-replay", "adj_mfma", 77, 1305, steps=("adaptive", TOL32), jvp=True),
        # the generic (VALU) adjoint
        Case("generic-cfg2", "generic", (16, 48, 16), (T,) * 2, 8, 8, 77, 1401, kernel="generic"),
        _headline("generic-cfg3", "generic", 77, 1402, kernel="generic"),
        Case("generic-cfg5", "generic", (128, 384, 128), (T,) * 2, 64, 64, 40, 1403, kernel="generic"),
    ]
    # the contraction after a larger call on the same handle: ragged K = 6 x steps x B, large data first
    for B in (17, 70, 333):
        cs.append(_headline(f"contraction-B{B}-after-B1100", "contraction", B, 1600 + B, steps=("fixed", 0.1), xs_scale=3.0))
    return cs


GPU_CASES = {c.name: c for c in _cases()}


# ---------------------------------------------------------------------------------------
# oracle runs (memoised: in the process, and in CNF_GRAD_TERMS_CACHE=<dir> across processes)
# ---------------------------------------------------------------------------------------
_MEMO = {}


def _key(cfg, arrays, dts, dtype, tag):
    h = hashlib.sha1()
    h.update(repr((cfg.net.dims, cfg.net.acts, cfg.nvars, cfg.naugs, cfg.lam1, cfg.lam2, cfg.lam3, cfg.use_jvp,
                   tuple(float(t) for t in cfg.tspan), np.dtype(dtype).name, tag)).encode())
    for a in arrays:
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    h.update(np.asarray(dts, dtype=np.float64).tobytes())
    return h.hexdigest()


def cache_dir():
    return os.environ.get("CNF_GRAD_TERMS_CACHE") or None


def save_cache(path):
    """Writes the process's memo to ``path`` (for child processes that run with CNF_GRAD_TERMS_CACHE=path)."""
    os.makedirs(path, exist_ok=True)
    for k, (val, grad, gx) in _MEMO.items():
        f = os.path.join(path, k + ".npz")
        if not os.path.exists(f):
            np.savez(f, val=val, grad=grad, gx=gx)


def oracle_run(cfg, flat, xs, eps, ys, dts, dtype=np.float64, tag=""):
    """(loss, grad, grad_x) of the oracle replaying the steps ``dts`` in ``dtype``."""
    key = _key(cfg, (flat, xs, eps, ys), dts, dtype, tag)
    if key in _MEMO:
        return _MEMO[key]
    d = cache_dir()
    f = os.path.join(d, key + ".npz") if d else None
    if f and os.path.exists(f):
        z = np.load(f)
        out = (float(z["val"]), z["grad"], z["gx"])
    else:
        c = lambda a: None if a is None else np.asarray(a).astype(dtype)
        val, grad, st = G.loss_and_grad(cfg, c(flat), c(xs), c(eps), c(ys), dts=list(dts))
        out = (float(val), np.asarray(grad), np.asarray(st.grad_x))
        if f:
            os.makedirs(d, exist_ok=True)
            np.savez(f, val=out[0], grad=out[1], gx=out[2])
    _MEMO[key] = out
    return out


def resolve_steps(cfg, flat, xs, eps, ys, ora_kw):
    """The step sizes the references replay: ``ora_kw['dts']`` (the device's own), or those of a float64 solve with
    ``ora_kw`` (fixed dt, or the oracle's adaptive controller)."""
    if "dts" in ora_kw:
        return [abs(float(d)) for d in ora_kw["dts"]]
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
    u0 = O.inference_u0(cfg, f64(xs), True)
    _, st = O.tsit5_solve(cfg.rhs(f64(flat), f64(eps), True, f64(ys)), u0, cfg.tspan[0], cfg.tspan[1], **ora_kw)
    return list(st.dts)


@dataclass
class TermRef:
    k: int
    net: O.Net
    dts: list
    ref: tuple          # (loss, grad, grad_x): float64 oracle at lam = e_k
    zero: tuple         # float64 oracle at lam = 0, same steps
    f32: tuple          # float32 oracle at lam = e_k, same steps

    @property
    def part(self):
        return self.ref[1] - self.zero[1]

    @property
    def part_x(self):
        return self.ref[2] - self.zero[2]


def term_reference(cfg, flat, xs, eps, ys, k, ora_kw):
    """The references of term k (1..3) for the model ``cfg`` (its own lam values are ignored): the float64 oracle at
    lam = e_k and at lam = 0 and the float32 oracle at lam = e_k, all three through the same steps (``ora_kw``: ``dts``
    to replay, or the arguments of a float64 solve that chooses them, run at lam = e_k)."""
    with_lam = lambda lam: dataclasses.replace(cfg, lam1=lam[0], lam2=lam[1], lam3=lam[2] if cfg.naugs else 0.0)
    ck, c0 = with_lam(one_hot(k)), with_lam(one_hot(0))
    dts = resolve_steps(ck, flat, xs, eps, ys, ora_kw)
    return TermRef(k, cfg.net, dts,
                   oracle_run(ck, flat, xs, eps, ys, dts, np.float64),
                   oracle_run(c0, flat, xs, eps, ys, dts, np.float64),
                   oracle_run(ck, flat, xs, eps, ys, dts, np.float32))


def _scale(part):
    part = np.asarray(part, dtype=np.float64)
    return float(np.abs(part).max() + np.sqrt(np.mean(part * part))) if part.size else 0.0


def term_floors(ref):
    """block name (and "grad_x") -> (scale of the term's part, float32-oracle error over that scale)."""
    out = {}
    for name, sl in param_blocks(ref.net).items():
        s = _scale(ref.part[sl])
        out[name] = (s, float(np.abs(ref.f32[1][sl].astype(np.float64) - ref.ref[1][sl]).max()) / s if s > 0 else np.inf)
    s = _scale(ref.part_x)
    out["grad_x"] = (s, float(np.abs(ref.f32[2].astype(np.float64) - ref.ref[2]).max()) / s if s > 0 else np.inf)
    return out


def rtol_of(floor):
    return max(helpers.RTOL, FLOOR_FACTOR * floor)


def _worst(d):
    """Index of the largest entry of ``d`` (of the first non-finite one, if any)."""
    bad = ~np.isfinite(d)
    return np.unravel_index(int(np.argmax(bad if bad.any() else d)), d.shape)


def grad_term_report(got, got_x, ref):
    """Per parameter block and for grad_x (``got_x`` None: not compared): dict(block, scale, floor, rtol, err -- all three
    over the scale of the term's part --, where -- the worst entry --, ok)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.ref[1].shape, (got.shape, ref.ref[1].shape)
    floors = term_floors(ref)
    recs = []

    def rec(name, d, where_of):
        scale, floor = floors[name]
        i = _worst(d)
        rtol = rtol_of(floor)
        err = float(d[i]) / scale if scale > 0 else np.inf
        recs.append(dict(block=name, scale=scale, floor=floor, rtol=rtol, err=err, where=where_of(i),
                         ok=bool(np.isfinite(err) and err <= rtol and rtol <= RTOL_CAP)))

    for name, sl in param_blocks(ref.net).items():
        rec(name, np.abs(got[sl] - ref.ref[1][sl]), lambda i, name=name: block_entry(ref.net, name, int(i[0])))
    if got_x is not None:
        gx = np.asarray(got_x, dtype=np.float64)
        assert gx.shape == ref.ref[2].shape, (gx.shape, ref.ref[2].shape)
        rec("grad_x", np.abs(gx - ref.ref[2]), lambda i: f"row {int(i[0])} column (sample) {int(i[1])}")
    return recs


def assert_grad_term(got, got_x, ref, what, route=""):
    """``got`` / ``got_x``: gradient and d loss / d xs of a run at lam = e_k (``ref.k``).  Files err / scale, floor and rtol
    of every block (helpers.note -> parity_report.json on a GPU run) and asserts the bar of the module docstring."""
    recs = grad_term_report(got, got_x, ref)
    term = TERM_NAMES[ref.k]
    for r in recs:
        RECORDS.append(dict(r, what=what, term=term, route=route))
    line = (f"grad term {term} | {what} | block err/scale floor rtol: " +
            "; ".join(f"{r['block']} {r['err']:.2e} {r['floor']:.2e} {r['rtol']:.1e}" for r in recs))
    helpers.note(line)
    print(line)
    for r in recs:
        assert r["scale"] > 0, f"{what} {term} {r['block']}: the term has no share in this block (nothing to compare against)"
        assert r["rtol"] <= RTOL_CAP, (f"{what} {term} {r['block']}: the float32 oracle's own error {r['floor']:.3g} of the term "
                                       f"scale asks for rtol {r['rtol']:.3g} > the cap {RTOL_CAP:g}")
    bad = [r for r in recs if not r["ok"]]
    assert not bad, f"{what}, term {term}: " + "; ".join(
        f"{r['block']} off by {r['err']:.3g} of the term's scale {r['scale']:.3g} at {r['where']} "
        f"(rtol {r['rtol']:.3g}, float32 floor {r['floor']:.3g})" for r in bad)
    return recs


def summary_notes():
    """Per route and term: the largest err / scale and the largest floor over the checks filed so far (parameter blocks and
    grad_x apart)."""
    rows = {}
    for r in RECORDS:
        key = (r["route"], r["term"], "grad_x" if r["block"] == "grad_x" else "params")
        e, f, q = rows.get(key, (0.0, 0.0, 0.0))
        rows[key] = (max(e, r["err"]), max(f, r["floor"]), max(q, r["err"] / r["rtol"]))
    return [f"grad term summary | {route} {term} {kind}: max err/scale {e:.2e}, max float32 floor {f:.2e}, max err/bar {q:.2f}"
            for (route, term, kind), (e, f, q) in sorted(rows.items())]


# ---------------------------------------------------------------------------------------
# degenerate inputs: zero norms
# ---------------------------------------------------------------------------------------
def zero_eps_columns(eps, cols=None):
    """eps = 0 in a few columns of a tile: |eps' J| (|J eps|) is 0 in those columns only."""
    eps = eps.copy()
    B = eps.shape[1]
    cols = sorted({c for c in ((0, 5, B - 1) if cols is None else cols) if 0 <= c < B})
    eps[:, cols] = 0
    return eps


def zero_last_layer(net, flat):
    """W_L = 0, b_L = 0: zdot = 0, J = 0, the augmented rows stay exactly 0 -- all three norms are 0 at every stage."""
    flat = flat.copy()
    blocks = param_blocks(net)
    L = net.n_layers
    flat[blocks[f"W{L}"]] = 0
    flat[blocks[f"b{L}"]] = 0
    return flat


DEGENERATE = ("zero-eps-columns", "zero-last-layer")


def degenerate_inputs(case, which):
    flat, xs, eps, ys = case.inputs()
    if which == "zero-eps-columns":
        eps = zero_eps_columns(eps)
    else:
        assert which == "zero-last-layer", which
        flat = zero_last_layer(case.net, flat)
    return flat, xs, eps, ys


@contextlib.contextmanager
def without_second_derivative():
    """The oracle's pullback with s'' = 0 (a mutant: the q = s'' (W t) sweep dropped)."""
    keep = G.act_d2
    G.act_d2 = lambda kind, a: np.zeros_like(a)
    try:
        yield
    finally:
        G.act_d2 = keep
