"""Every way through solve_core (csrc/cnf_abi.hip) other than the headline body, against the bits the build of the commit named
in tests/golden/solve_routes/solve_routes.npz produced on the same inputs.

tests/test_gpu_headline_bits.py pins k_solve3b on the headline network in TrainMode, in one launch and streamed.  This file pins
the other routes, each on the smallest shape that takes it, and asserts from last_stats (launches, kernel_used) and the change of
solve_fallbacks() that the route the case is about was the route taken:

* wave-*: k_solve_wave on the 2-6-2 network of the JVP tests, B = 16 (one tile) and 24 (a ragged second tile), TrainMode and
  TestMode, adaptive with the automatic initial dt, adaptive with a given dt, fixed dt;
* bcast-*: k_solve_bcast on config 5's 128-384-128 network, TrainMode inference at B = 8 and 20, loss_and_grad at B = 8 (its
  recording form);
* tsolve-*: TestMode inference on the headline network at B = 32, k_trace3s<SOLVE> in three launches, and in the
  CNF_PERSISTENT=0 child the streamed fused-trace route with the fused initial dt;
* generic-*: kernel="generic" on the 2-6-2 network at B = 24 (streamed, generic right-hand side), both modes;
* aux-deep-test: the 10-40-24-10 network of test_exact_trace_mfma_deep_networks, TestMode, B = 32 (streamed, the auxiliary trace
  kernel per stage);
* grad-headline-streamed: loss_and_grad on the headline network at B = 32 in the child (streamed recording on the fused step kernel);
* lockstep-*: one attempt at a time under a shard_reduce callback that returns its input (one shard), headline network B = 32 and
  the generic route at B = 24;  grad-test-recorded: the TestMode recorded solve (loss_and_grad, kernel="generic", 2-6-2, B = 24);
* wg-*: the in-launch gradient (loss_and_grad, 2-6-2, B = 16), both modes;
* path-*: inference_path with K = 4 save times (t0 and t1 among them) in the wave launch (B = 24) and one attempt at a time
  (kernel="generic"), with path_steps;
* jvp-*: inference_jvp with R = 2 on the 2-6-2 network, with jvp_steps: at B = 24 in one launch and, with set_solve_wait(0, 1),
  on the route of test_fallback_route_files_its_steps -- that one at B = 68, that test's batch: up to four tiles are the waves
  of ONE workgroup and meet through LDS, where no wait can run out, so B = 24 never takes the route; five tiles are five
  workgroups that have to meet;
* submit-*: two submitted inferences and a submitted gradient (2-6-2, B = 16), outputs and collected statistics.

Compared, all of it exactly: every output array, (nf, naccept, nreject, launches, kernel_used, fallbacks taken), the step trace
(t, h, EEst, accepted) as the handle filed it (zero rows on the routes that file none), grad_steps of the gradient cases.
Every case ran twice at recording and no (case, field) pair differed between the two runs: nothing is left out of the file.
An array of more than 4096 entries (the gradients of the two wide networks) is kept as a SHA-256 over all its bytes plus its
first and last 1024 entries.

The inputs are seeds, so the file holds outputs only.  Recording (with the library of the commit to pin, on the GPU; every case
runs twice and a case whose two runs differ is refused):  python tests/test_gpu_solve_route_bits.py --record <commit hash> [file]
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "solve_routes", "solve_routes.npz")
SEED_PARAMS, SEED_INPUTS, BIAS_SCALE, TRACE_CAP = 12345, 1, 0.1, 96
DEEP_DIMS, DEEP_ACTS, DEEP_NVARS, DEEP_NAUGS = (10, 40, 24, 10), ("tanh", "sigmoid", "tanh"), 8, 2
SOLVERS = {"hairer": None, "dt": dict(dt=1 / 16), "fixed": dict(adaptive=False, dt=1 / 8)}    # None: the README tolerances, dt = 0
ONE, STREAMED, STEPWISE = "one_launch", "streamed", "stepwise"
FULL_ENTRIES, KEPT_ENDS = 4096, 1024                       # above the first: a digest and that many entries from either end


def _c(name, **spec):
    spec.setdefault("kind", "inference")
    spec.setdefault("solver", "hairer")
    spec.setdefault("kernel", "mfma")
    spec.setdefault("train", True)
    return name, spec


CASES = [_c(f"wave-B{B}-{'train' if train else 'test'}-{solver}", net="small", B=B, train=train, solver=solver, route=ONE, launches=1)
         for B in (16, 24) for train in (True, False) for solver in SOLVERS]
CASES += [_c(f"bcast-B{B}-train", net="cfg5", B=B, route=ONE) for B in (8, 20)]
CASES += [_c("bcast-B8-grad", net="cfg5", B=8, kind="grad", route=ONE)]
CASES += [_c("tsolve-B32-test", net="headline", B=32, train=False, route=ONE, launches=3),
          _c("tsolve-B32-test-streamed", net="headline", B=32, train=False, route=STREAMED, child=True)]
CASES += [_c(f"generic-B24-{'train' if train else 'test'}", net="small", B=24, train=train, kernel="generic", route=STREAMED)
          for train in (True, False)]
CASES += [_c("aux-deep-test", net="deep", B=32, train=False, route=STREAMED)]
CASES += [_c("grad-headline-streamed", net="headline", B=32, kind="grad", route=STREAMED, child=True)]
CASES += [_c("lockstep-headline-B32", net="headline", B=32, lockstep=True, route=STEPWISE),
          _c("lockstep-generic-B24", net="small", B=24, kernel="generic", lockstep=True, route=STEPWISE),
          _c("grad-test-recorded", net="small", B=24, train=False, kernel="generic", kind="grad", route=STEPWISE)]
CASES += [_c(f"wg-B16-{'train' if train else 'test'}", net="small", B=16, train=train, kind="grad", route=ONE) for train in (True, False)]
CASES += [_c("path-wave-B24", net="small", B=24, kind="path", route=ONE),
          _c("path-generic-B24", net="small", B=24, kernel="generic", kind="path", route=STEPWISE)]
CASES += [_c("jvp-B24", net="small", B=24, kind="jvp", route=ONE, launches=2),
          _c("jvp-B68-fallback", net="small", B=68, kind="jvp", route=STEPWISE, fallback=True)]
CASES += [_c("submit-inference-B16", net="small", B=16, kind="submit", route=ONE, launches=1),
          _c("submit-grad-B16", net="small", B=16, kind="submit_grad", route=ONE, launches=1)]


def _model(cnf, spec):
    """-> (icnf, flat, xs, eps or None, extra) for the case's network, built from seeds."""
    from continuousnf.jl_amd import configs
    kw = dict(configs.README_TOLERANCES, **(SOLVERS[spec["solver"]] or {}))
    train, B = spec["train"], spec["B"]
    if spec["net"] == "small":
        from tests import jvp_ref as J
        from tests.helpers import make_icnf
        mode = "vjp" if train else "test"
        flat, xs, _, eps, dps, dxs, _ = J.case_inputs("2-6-2", mode, B)
        return make_icnf(cnf, J.case_cfg("2-6-2", mode), kernel=spec["kernel"], sol_kwargs=kw), flat, xs, eps, (dps[:2], dxs[:2])
    if spec["net"] == "deep":
        nn = cnf.Chain(*[cnf.Dense(a, b, act) for a, b, act in zip(DEEP_DIMS[:-1], DEEP_DIMS[1:], DEEP_ACTS)])
        ic = cnf.construct(cnf.RNODE, nn, DEEP_NVARS, DEEP_NAUGS, compute_mode=cnf.HIPVecJacMatrixMode(spec["kernel"]), sol_kwargs=kw)
        xs = np.random.default_rng(SEED_INPUTS).standard_normal((DEEP_NVARS, B)).astype(np.float32)
        return ic, configs.glorot_params(DEEP_DIMS, SEED_PARAMS, BIAS_SCALE), xs, None, None
    w = configs.BASELINE[3 if spec["net"] == "headline" else 5]
    xs, eps = configs.synthetic_inputs(w, B, SEED_INPUTS)
    return configs.build(w, kernel=spec["kernel"], sol_kwargs=kw), configs.glorot_params(w.dims, SEED_PARAMS, BIAS_SCALE), xs, eps, None


def _assert_route(name, spec, st, fell_back):
    """the route the case is about was the route taken"""
    import continuousnf.jl_amd as cnf
    assert fell_back == (1 if spec.get("fallback") else 0), (name, fell_back, st)
    assert (st["launches"] <= 3) == (spec["route"] == ONE), (name, st)
    if "launches" in spec:
        assert st["launches"] == spec["launches"], (name, st)
    generic = spec["kernel"] == "generic"
    assert st["kernel_used"] == (cnf._lib.KERNEL_GENERIC if generic else cnf._lib.KERNEL_MFMA), (name, st)


def _compute(name, spec):
    """One case on the GPU -> {field: numpy array}."""
    import torch

    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import path as cnf_path

    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ic, flat, xs, eps, extra = _model(cnf, spec)
    T = cnf.TrainMode() if spec["train"] else cnf.TestMode()
    ekw = dict(eps=dev(eps)) if spec["train"] else {}
    xs_d, ps_d = dev(xs), dev(flat)
    trace = ic.set_step_trace(TRACE_CAP)
    if spec.get("lockstep"):
        ic.set_shard_reduce(lambda v: None)                # one shard: the sum over the shards is the input
    if spec.get("fallback"):
        ic.set_solve_wait(0, 1)
    fb0 = ic.solve_fallbacks()
    out, kind = {}, spec["kind"]
    regs_of = lambda regs: torch.stack(list(regs)).cpu().numpy()
    if kind == "inference":
        logpx, regs, sums = cnf.inference(ic, T, xs_d, ps_d, {}, with_sums=True, **ekw)
        out.update(logpx=logpx.cpu().numpy(), regs=regs_of(regs), sums=sums.cpu().numpy())
    elif kind == "grad":
        loss, grad = cnf.loss_and_grad(ic, T, xs_d, ps_d, {}, **ekw)
        out.update(loss=np.asarray([loss], dtype=np.float32), grad=grad.cpu().numpy(), grad_steps=np.array(ic.last_steps, dtype=np.float32))
    elif kind == "path":
        t0, t1 = ic.tspan
        saveat = np.asarray([t0, t0 + 0.3 * (t1 - t0), t0 + 0.7 * (t1 - t0), t1], dtype=np.float32)
        logpx, regs, p = cnf.inference_path(ic, T, xs_d, ps_d, {}, saveat=saveat, **ekw)
        out.update(logpx=logpx.cpu().numpy(), regs=regs_of(regs), path_z=p["z"].contiguous().cpu().numpy(),
                   path_dlogp=p["dlogp"].contiguous().cpu().numpy(), path_E=p["E"].contiguous().cpu().numpy(),
                   path_n=p["n"].contiguous().cpu().numpy(), path_steps=np.stack(cnf_path.path_steps(ic)))
    elif kind == "jvp":
        (logpx, regs), (dl, dr), info = cnf.inference_jvp(ic, T, xs_d, ps_d, {}, d_ps=dev(extra[0]), d_xs=dev(extra[1]), **ekw)
        out.update(logpx=logpx.cpu().numpy(), regs=regs_of(regs), tangent=torch.stack([dl, *dr]).cpu().numpy(), jvp_steps=np.stack(info["steps"]))
    elif kind == "submit":
        xs2 = dev(np.ascontiguousarray(xs[:, ::-1]))
        outs = [cnf.inference_submit(ic, T, x, ps_d, {}, with_sums=True, **ekw) for x in (xs_d, xs2)]
        for i, (logpx, regs, sums) in enumerate(outs):
            st = cnf.inference_collect(ic)
            torch.cuda.synchronize()
            out.update({f"logpx{i}": logpx.cpu().numpy(), f"regs{i}": regs_of(regs), f"sums{i}": sums.cpu().numpy()})
            out[f"stats{i}"] = np.asarray([st[k] for k in ("nf", "naccept", "nreject", "launches", "kernel_used")], dtype=np.int64)
    elif kind == "submit_grad":
        lossd, grad = cnf.loss_and_grad_submit(ic, T, xs_d, ps_d, {}, **ekw)
        cnf.loss_and_grad_collect(ic)
        torch.cuda.synchronize()
        out.update(loss=lossd.cpu().numpy(), grad=grad.cpu().numpy())
    torch.cuda.synchronize()
    st = ic.last_stats
    fell_back = ic.solve_fallbacks() - fb0
    out["stats"] = np.asarray([st["nf"], st["naccept"], st["nreject"], st["launches"], st["kernel_used"], fell_back], dtype=np.int64)
    out["trace"] = trace.cpu().numpy()
    _assert_route(name, spec, st, fell_back)
    ic.close()
    return _filed(out)


def _filed(out):
    """What the golden file keeps of a case's arrays."""
    kept = {}
    for k, v in out.items():
        if v.size > FULL_ENTRIES:
            kept[k + "_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest(), dtype=np.uint8)
            kept[k + "_ends"] = np.ascontiguousarray(np.r_[v.ravel()[:KEPT_ENDS], v.ravel()[-KEPT_ENDS:]])
        else:
            kept[k] = v
    return kept


def _child_cases(tmp_dir):
    """All CNF_PERSISTENT=0 cases from ONE child process -> {"<case>/<field>": array}."""
    import subprocess
    out = os.path.join(str(tmp_dir), "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, CNF_PERSISTENT="0"), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN_FILE))


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    return _child_cases(tmp_path_factory.mktemp("solve_routes"))


def _case(name, spec, child):
    if spec.get("child"):
        return {k.split("/", 1)[1]: v for k, v in child.items() if k.startswith(name + "/")}
    return _compute(name, spec)


@pytest.mark.gpu
@pytest.mark.parametrize("name,spec", CASES, ids=[c[0] for c in CASES])
def test_solve_route_bits_equal_the_pinned_build(name, spec, golden, child):
    got = _case(name, spec, child)
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert want and sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    for k in sorted(got):
        g, x = got[k], want[k]
        assert g.dtype == x.dtype and g.shape == x.shape, (name, k, g.dtype, x.dtype, g.shape, x.shape)
        same = g.tobytes() == x.tobytes()
        if not same and g.dtype == np.float32:
            d = np.flatnonzero(g.view(np.uint32).ravel() != x.view(np.uint32).ravel())
            print(f"{name}/{k}: {d.size} of {g.size} entries differ, first at {d[:4]}: got {g.ravel()[d[:4]]} pinned {x.ravel()[d[:4]]}")
        elif not same:
            print(f"{name}/{k}: got {g.tolist()} pinned {x.tolist()}")
        assert same, f"{name}/{k}: not the bits of commit {str(golden['parent_commit'])}"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":                # the child of _child_cases
        assert os.environ.get("CNF_PERSISTENT") == "0"
        np.savez(sys.argv[2], **{f"{name}/{k}": v for name, spec in CASES if spec.get("child") for k, v in _compute(name, spec).items()})
        sys.exit(0)
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--record", __doc__
    import tempfile
    rec = {"parent_commit": np.asarray(sys.argv[2]), "seeds": np.asarray([SEED_PARAMS, SEED_INPUTS], dtype=np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        runs = [_child_cases(tmp) for _ in range(2)]                    # every case twice: one build gives one set of bits
        for name, spec in CASES:
            first, again = _case(name, spec, runs[0]), _case(name, spec, runs[1])
            assert first and sorted(first) == sorted(again), name
            for k, v in first.items():
                assert v.tobytes() == again[k].tobytes(), f"{name}/{k}: two runs of one build differ"
                rec[f"{name}/{k}"] = v
            print(name, {k: (v.tolist() if v.size <= 6 else v.shape) for k, v in first.items()}, flush=True)
    target = sys.argv[3] if len(sys.argv) == 4 else GOLDEN_FILE
    os.makedirs(os.path.dirname(target), exist_ok=True)
    np.savez_compressed(target, **rec)
    print("recorded", len(CASES), "cases")
