"""The headline evaluation body (csrc/cnf_step3b_eval.inc: k_step3b and every instantiation of k_solve3b) against the bits
the build of the commit named in tests/golden/headline_bits/headline_bits.npz produced on the same inputs.

A change to that body that keeps the arithmetic -- the same MFMAs on the same operands in the same order, the same epilogue
expressions -- keeps every output bit; this file is the check.  The cases are the smallest that reach each code path: B = 32
(one full tile), B = 40 (a second tile with 8 live columns), B = 8224 (257 tiles: the several-tiles form, a second tile on
workgroup 0), each with the adaptive solve at the README tolerances and with fixed dt = 1/4, in one launch and on the
streamed step launches (CNF_PERSISTENT=0, read once per process: ONE child process computes all streamed cases; at
B = 8224 also poll_limit = 1, the switch of the fallback tests -- every wait of the one-launch solve runs out at once and the
call runs again on the streamed driver; one or two workgroups never run out of a wait, so that switch does not reach the small
cases); a conditional model of the headline shape at B = 40; loss_and_grad at B = 32 (the recording form).  Compared, all
of it exactly: logpx, the three regularisers, the five loss sums, nf / naccept / nreject, and the step trace
(t, h, EEst, accepted) as the handle filed it (only one-launch solves file one: on the streamed routes the rows stay zero;
the gradient case: the loss, the gradient vector, the counts, the trace).
The B = 8224 outputs are kept as a SHA-256 over all their bytes plus the columns of workgroup 0's two tiles in full.

The inputs are seeds (configs.glorot_params / configs.synthetic_inputs), so the file holds outputs only.  Recording (with
the library of the commit to pin, on the GPU):  python tests/test_gpu_headline_bits.py --record <commit hash> [file]
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (a folder of its own: every *.npz directly under tests/golden is an oracle case of tests/helpers.py:GOLDEN_CASES)
GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "headline_bits", "headline_bits.npz")
SEED_PARAMS, SEED_INPUTS, BIAS_SCALE, N_COND, TRACE_CAP = 12345, 1, 0.1, 8, 96
SOLVERS = {"adaptive": None, "fixed": dict(adaptive=False, dt=1 / 4)}       # None: the README tolerances
CASES = [(f"B{B}-{solver}-{route}", dict(B=B, solver=solver, route=route))
         for B in (32, 40, 8224) for solver in ("adaptive", "fixed") for route in ("one_launch", "streamed")]
CASES += [("B8224-adaptive-fallback", dict(B=8224, solver="adaptive", route="fallback"))]
CASES += [(f"cond-B40-{solver}-one_launch", dict(B=40, solver=solver, route="one_launch", cond=True))
          for solver in ("adaptive", "fixed")]
CASES += [("grad-B32-adaptive", dict(B=32, solver="adaptive", route="one_launch", grad=True))]
FULL_COLUMNS = 64                                          # above it: a digest and the columns of workgroup 0's tiles


def _compute(spec):
    """One case on the GPU -> {field: numpy array}."""
    import torch

    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs

    w = configs.BASELINE[3]
    B = spec["B"]
    kw = dict(SOLVERS[spec["solver"]] or configs.README_TOLERANCES)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xs, eps = configs.synthetic_inputs(w, B, SEED_INPUTS)
    args = []
    if spec.get("cond"):
        dims = (w.dims[0] + N_COND,) + w.dims[1:]
        nn = cnf.Chain(*[cnf.Dense(a, b, "tanh") for a, b in zip(dims[:-1], dims[1:])])
        ic = cnf.construct(cnf.CondRNODE, nn, w.nvars, w.naugs, compute_mode=cnf.HIPVecJacMatrixMode("mfma"), tspan=w.tspan,
                           lambda1=w.lambdas[0], lambda2=w.lambdas[1], lambda3=w.lambdas[2], sol_kwargs=kw)
        ys = np.random.default_rng(SEED_INPUTS + 1).standard_normal((N_COND, B)).astype(np.float32)
        args.append(dev(ys))
    else:
        dims = w.dims
        ic = configs.build(w, kernel="mfma", sol_kwargs=kw)
    flat = configs.glorot_params(dims, SEED_PARAMS, BIAS_SCALE)
    trace = ic.set_step_trace(TRACE_CAP)
    if spec["route"] == "fallback":
        ic.set_solve_wait(poll_limit=1)
    fb0 = ic.solve_fallbacks()
    out = {}
    if spec.get("grad"):
        loss, grad = cnf.loss_and_grad(ic, cnf.TrainMode(), dev(xs), *args, flat, {}, eps=dev(eps))
        torch.cuda.synchronize()
        out["loss"] = np.asarray([loss], dtype=np.float32)
        out["grad"] = grad.cpu().numpy()
    else:
        logpx, regs, sums = cnf.inference(ic, cnf.TrainMode(), dev(xs), *args, flat, {}, eps=dev(eps), with_sums=True)
        torch.cuda.synchronize()
        out["logpx"] = logpx.cpu().numpy()
        out["regs"] = torch.stack(list(regs)).cpu().numpy()
        out["sums"] = sums.cpu().numpy()
    st = ic.last_stats
    out["counts"] = np.asarray([st["nf"], st["naccept"], st["nreject"]], dtype=np.int64)
    out["trace"] = trace.cpu().numpy()
    # the route the case is about was the route taken
    fell_back = ic.solve_fallbacks() - fb0
    assert fell_back == (1 if spec["route"] == "fallback" else 0), (spec, fell_back, st)
    if not spec.get("grad"):
        assert (st["launches"] <= 3) == (spec["route"] == "one_launch"), (spec, st)
    assert st["kernel_used"] == cnf._lib.KERNEL_MFMA, st
    ic.close()
    return out


def _filed(out):
    """What the golden file keeps of a case's arrays."""
    kept = {}
    for k, v in out.items():
        if k in ("logpx", "regs") and v.shape[-1] > FULL_COLUMNS:
            n = v.shape[-1]
            cols = np.r_[0:32, 32 * ((n - 1) // 32):n]            # workgroup 0: its first tile and the last tile of the batch
            kept[k + "_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest(), dtype=np.uint8)
            kept[k + "_cols"] = np.ascontiguousarray(v[..., cols])
        else:
            kept[k] = v
    return kept


def _streamed_cases(tmp_dir):
    """All streamed cases from ONE child process that has CNF_PERSISTENT=0 -> {"<case>/<field>": array}."""
    import subprocess
    out = os.path.join(str(tmp_dir), "streamed.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--streamed", out], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, CNF_PERSISTENT="0"), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN_FILE))


@pytest.fixture(scope="module")
def streamed(tmp_path_factory):
    return _streamed_cases(tmp_path_factory.mktemp("headline_bits"))


def _case(name, spec, streamed):
    if spec["route"] == "streamed":
        return {k.split("/", 1)[1]: v for k, v in streamed.items() if k.startswith(name + "/")}
    return _filed(_compute(spec))


@pytest.mark.gpu
@pytest.mark.parametrize("name,spec", CASES, ids=[c[0] for c in CASES])
def test_headline_body_bits_equal_the_pinned_build(name, spec, golden, streamed):
    got = _case(name, spec, streamed)
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert want and sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    for k in sorted(got):
        g, x = got[k], want[k]
        assert g.dtype == x.dtype and g.shape == x.shape, (name, k, g.dtype, x.dtype, g.shape, x.shape)
        same = g.tobytes() == x.tobytes()
        if not same and g.dtype == np.float32:
            d = np.flatnonzero(g.view(np.uint32).ravel() != x.view(np.uint32).ravel())
            print(f"{name}/{k}: {d.size} of {g.size} entries differ, first at {d[:4]}: got {g.ravel()[d[:4]]} pinned {x.ravel()[d[:4]]}")
        assert same, f"{name}/{k}: not the bits of commit {str(golden['parent_commit'])}"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--streamed":             # the child of _streamed_cases
        assert os.environ.get("CNF_PERSISTENT") == "0"
        np.savez(sys.argv[2], **{f"{name}/{k}": v for name, spec in CASES if spec["route"] == "streamed"
                                 for k, v in _filed(_compute(spec)).items()})
        sys.exit(0)
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--record", __doc__
    import tempfile
    rec = {"parent_commit": np.asarray(sys.argv[2]), "seeds": np.asarray([SEED_PARAMS, SEED_INPUTS], dtype=np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        runs = [_streamed_cases(tmp) for _ in range(2)]                  # every case twice: one build gives one set of bits
        for name, spec in CASES:
            first, again = _case(name, spec, runs[0]), _case(name, spec, runs[1])
            assert first and sorted(first) == sorted(again), name
            for k, v in first.items():
                assert v.tobytes() == again[k].tobytes(), f"{name}/{k}: two runs of one build differ"
                rec[f"{name}/{k}"] = v
            print(name, {k: (v.tolist() if v.size <= 5 else v.shape) for k, v in first.items()}, flush=True)
    np.savez_compressed(sys.argv[3] if len(sys.argv) == 4 else GOLDEN_FILE, **rec)
    print("recorded", len(CASES), "cases")

