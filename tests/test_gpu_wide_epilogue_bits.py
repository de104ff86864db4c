"""The half boundary of a 16-row tile in the headline evaluation body (csrc/cnf_step3b_eval.inc), which
tests/test_gpu_headline_bits.py does not reach: a wave owns the tile of BOTH sample halves of a 32-column block (columns 0-15
and 16-31), and the wide products run the two halves one after the other, the first half's epilogue among the second half's
MFMAs.  Every accumulator still takes the same MFMAs on the same operands in the same order, so every output bit stays what
the build of the commit named in tests/golden/headline_bits/half_tiles.npz produced on the same inputs.

Batches: B = 1, 15, 16, 17, 31 -- the second half all padding (1, 15, 16), partly live (17), one column short (31); the
adaptive solve at the README tolerances and fixed dt = 1/4; in one launch and on the streamed step launches (CNF_PERSISTENT=0,
read once per process: ONE child process computes all streamed cases).  Compared exactly: logpx, the three regularisers, the
five loss sums, nf / naccept / nreject.

One case needs no golden file: at B = 32 with fixed dt, columns 0-15 of xs and eps swapped with columns 16-31 give logpx and
the regularisers of the unswapped call, swapped, bit for bit (the two halves run the same arithmetic on different registers).

The inputs are seeds (configs.glorot_params / configs.synthetic_inputs), so the file holds outputs only.  Recording (with the
library of the commit to pin, on the GPU):  python tests/test_gpu_wide_epilogue_bits.py --record <commit hash> [file]
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "headline_bits", "half_tiles.npz")
SEED_PARAMS, SEED_INPUTS, BIAS_SCALE = 12345, 1, 0.1
SOLVERS = {"adaptive": None, "fixed": dict(adaptive=False, dt=1 / 4)}       # None: the README tolerances
CASES = [(f"B{B}-{solver}-{route}", dict(B=B, solver=solver, route=route))
         for B in (1, 15, 16, 17, 31) for solver in ("adaptive", "fixed") for route in ("one_launch", "streamed")]


def _solve(spec, xs, eps):
    """One inference of the headline model on the GPU -> {field: numpy array}."""
    import torch

    import continuousnf.jl_amd as cnf
    from continuousnf.jl_amd import configs

    w = configs.BASELINE[3]
    kw = dict(SOLVERS[spec["solver"]] or configs.README_TOLERANCES)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ic = configs.build(w, kernel="mfma", sol_kwargs=kw)
    flat = configs.glorot_params(w.dims, SEED_PARAMS, BIAS_SCALE)
    fb0 = ic.solve_fallbacks()
    logpx, regs, sums = cnf.inference(ic, cnf.TrainMode(), dev(xs), flat, {}, eps=dev(eps), with_sums=True)
    torch.cuda.synchronize()
    st = ic.last_stats
    out = {"logpx": logpx.cpu().numpy(), "regs": torch.stack(list(regs)).cpu().numpy(), "sums": sums.cpu().numpy(),
           "counts": np.asarray([st["nf"], st["naccept"], st["nreject"]], dtype=np.int64)}
    # the route the case is about was the route taken, on the headline kernels
    assert ic.solve_fallbacks() == fb0, (spec, st)
    assert (st["launches"] <= 3) == (spec["route"] == "one_launch"), (spec, st)
    assert st["kernel_used"] == cnf._lib.KERNEL_MFMA, st
    ic.close()
    return out


def _compute(spec):
    from continuousnf.jl_amd import configs
    xs, eps = configs.synthetic_inputs(configs.BASELINE[3], spec["B"], SEED_INPUTS)
    return _solve(spec, xs, eps)


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
    return _streamed_cases(tmp_path_factory.mktemp("half_tiles"))


def _case(name, spec, streamed):
    if spec["route"] == "streamed":
        return {k.split("/", 1)[1]: v for k, v in streamed.items() if k.startswith(name + "/")}
    return _compute(spec)


@pytest.mark.gpu
@pytest.mark.parametrize("name,spec", CASES, ids=[c[0] for c in CASES])
def test_half_tile_bits_equal_the_pinned_build(name, spec, golden, streamed):
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


def _swapped_halves():
    """B = 32, fixed dt: the call and the call on half-swapped columns -> (plain, swapped, column permutation)."""
    from continuousnf.jl_amd import configs
    spec = dict(B=32, solver="fixed", route="one_launch")
    xs, eps = configs.synthetic_inputs(configs.BASELINE[3], 32, SEED_INPUTS)
    perm = np.r_[16:32, 0:16]
    return _solve(spec, xs, eps), _solve(spec, xs[:, perm], eps[:, perm]), perm


@pytest.mark.gpu
def test_swapping_the_halves_of_a_tile_swaps_the_bits():
    plain, swapped, perm = _swapped_halves()
    for k in ("logpx", "regs"):
        assert plain[k].shape[-1] == 32
        assert swapped[k].tobytes() == np.ascontiguousarray(plain[k][..., perm]).tobytes(), k
    assert plain["counts"].tolist() == swapped["counts"].tolist()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--streamed":             # the child of _streamed_cases
        assert os.environ.get("CNF_PERSISTENT") == "0"
        np.savez(sys.argv[2], **{f"{name}/{k}": v for name, spec in CASES if spec["route"] == "streamed"
                                 for k, v in _compute(spec).items()})
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
