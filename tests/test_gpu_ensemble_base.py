"""Ensembles with a base distribution per member on the device: ``bases=`` of ``inference_many`` / ``loss_many``,
``loss_and_grad_many``, ``inference_vjp_many``, ``generate_many``, ``generate_vjp_many``, the differentiable forms,
``reverse_kl_many`` and ``EnsembleDist`` (cnf_ensemble_set_bases; the BASE forms of the ensemble gradient kernel, and the column
kernels of csrc/cnf_ens_base.hip).

References: tests/ensemble_base_ref.py -- ``vjp_ref.vjp64`` / ``gen_vjp_ref`` with ``base=`` and ``base_grad_ref`` replaying, for
every member, the steps that member itself accepted on the device.  Bars: tests/helpers.py for values, ``vjp_ref.assert_vjp``
for parameter and input gradients, ``base_grad_ref.assert_base`` for ``(g_mean, g_scale)`` (tests/test_ensemble_base_host.py
holds the float32 floors of these cases).  Everything else -- the member whose base is (0, I) against the call without bases,
member m against the M = 1 call, repetition, splits -- is compared bit for bit.
"""
import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from continuousnf.jl_amd import _lib
from continuousnf.jl_amd import ensemble as ens_mod
from tests import base_grad_ref as BG
from tests import ensemble_base_ref as EB
from tests import ensemble_vjp_ref as R
from tests import helpers
from tests import vjp_ref as V
from tests.helpers import assert_parity, make_icnf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
M, UNIT = EB.M, EB.UNIT


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _mode(train):
    return cnf.TrainMode() if train else cnf.TestMode()


def _icnf(case, **kw):
    return make_icnf(cnf, case.cfg, jvp=case.jvp, kernel="mfma", sol_kwargs=dict(case.sol_kw), **kw)


def _bases(case, kind, sl=slice(None)):
    mean, scale = EB.bases(case, kind)
    return cnf.EnsembleBases(mean[sl], **{"scale_tril" if kind == "dense" else "std": scale[sl]}), mean, scale


def _t1(case):
    return np.asarray(case.t1, np.float32) if case.t1 is not None else None


def _eps(case, eps):
    return _dev(eps) if case.train else None


def _cot_arg(c):
    return _dev(c[:, 0]), (_dev(c[:, 1]), _dev(c[:, 2]), _dev(c[:, 3]))


def _np(*ts):
    return tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in ts)


def _accepted(rows):
    """The signed sizes of the accepted attempts of a step trace (t, signed h, EEst, accepted)."""
    return [float(r[1]) for r in rows if r[3] != 0]


def _inference(icnf, case, ps, xs, eps, **kw):
    lp, rg, info = cnf.inference_many(icnf, _mode(case.train), _dev(xs[0] if case.shared_xs else xs), _dev(ps), {}, eps=_eps(case, eps),
                                      t1=_t1(case), with_steps=True, **kw)
    return lp.cpu().numpy(), torch.stack(list(rg), dim=1).cpu().numpy(), info


@pytest.mark.parametrize("case,kind", EB.CASE_KINDS, ids=EB.IDS)
def test_inference_many_scores_every_member_under_its_own_base(case, kind):
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    lp, rg, info = _inference(icnf, case, ps, xs, eps, bases=b)
    lp0, rg0, info0 = _inference(icnf, case, ps, xs, eps)
    assert info["launches"] == 2 and info["calls"] == 1 and not info["rerun"] and (info["status"] == _lib.OK).all(), info
    # the base does not enter the solve: regularisers, statistics and step sequences bit for bit those of the call without
    assert np.array_equal(rg, rg0)
    for m in range(M):
        assert np.array_equal(info["steps"][m], info0["steps"][m])
        assert {k: v for k, v in info["stats"][m].items() if k != "launches"} == {k: v for k, v in info0["stats"][m].items() if k != "launches"}
        what = f"inference_many bases {case.name} {kind} member {m}"
        dts = _accepted(info["steps"][m])
        out = V.outputs(R.member_cfg(case, m), ps[m].astype(np.float64), xs[m].astype(np.float64),
                        eps[m].astype(np.float64) if case.train else None, dts, train=case.train, base=EB.gauss(mean, scale, kind, m))[0]
        assert_parity(lp[m], out[0], f"{what} logpx")
        want = EB.loss_of(case, m, out)
        assert abs(info["losses"][m] - want) <= 1e-5 * max(1.0, abs(want)), (what, info["losses"][m], want)
    assert_parity(lp[UNIT], lp0[UNIT].astype(np.float64), f"{case.name} {kind}: the (0, I) member against the call without bases")
    losses = cnf.loss_many(icnf, _mode(case.train), _dev(xs[0] if case.shared_xs else xs), _dev(ps), {}, eps=_eps(case, eps), t1=_t1(case), bases=b)
    assert np.array_equal(losses, info["losses"])
    icnf.close()


def _vjp(icnf, case, ps, xs, eps, cot, **kw):
    res = cnf.inference_vjp_many(icnf, _mode(case.train), _dev(xs), _dev(ps), {}, _cot_arg(cot), eps=_eps(case, eps), t1=_t1(case),
                                 with_x=True, with_steps=True, **kw)
    lp, rg, g, gx, info = res[:5]
    out = _np(lp, torch.stack(list(rg), dim=1), g, gx) + (info,)
    return out + (_np(*res[5]),) if len(res) > 5 else out


@pytest.mark.parametrize("case,kind", EB.CASE_KINDS, ids=EB.IDS)
def test_inference_vjp_many_with_bases_matches_the_float64_adjoint(case, kind):
    icnf = _icnf(case)
    assert cnf.ensemble_vjp_capacity(icnf, _mode(case.train), case.B) >= M
    ps, xs, eps = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    cots = [dict(R.cotangents(case, m), loss=V.loss_cotangent(R.member_cfg(case, m), case.B, case.train).astype(np.float32)) for m in range(M)]
    for name in cots[0]:
        cot = np.stack([cots[m][name] for m in range(M)])
        lp, rg, g, gx, info, gb = _vjp(icnf, case, ps, xs, eps, cot, bases=b, with_base=True)
        assert info["calls"] == 1 and not info["rerun"] and (info["status"] == _lib.OK).all(), info
        for m in range(M):
            what = f"ensemble vjp bases {case.name} {kind} member {m} cot {name}"
            dts = info["steps"][m]
            out, r64, r32 = EB.reference(case, m, ps, xs, eps, cot[m], dts, EB.gauss(mean, scale, kind, m))
            assert_parity(lp[m], out[0], f"{what} logpx")
            V.assert_vjp(g[m], gx[m], r64, r32, case.cfg.net, what)
            if cot[m][0].any():
                b64, b32, summands = EB.base_reference(case, m, ps, xs, eps, cot[m][0], dts, mean, scale, kind)
                BG.assert_base((gb[0][m], gb[1][m]), b64, b32, summands, what)
            else:
                assert not gb[0][m].any() and not gb[1][m].any(), what
    # the member whose base is (0, I): gradients bit for bit those of the call without bases; again: the same bits
    lp0, rg0, g0, gx0, info0 = _vjp(icnf, case, ps, xs, eps, cot)
    assert np.array_equal(g[UNIT], g0[UNIT]) and np.array_equal(gx[UNIT], gx0[UNIT])
    assert np.array_equal(rg, rg0) and all(np.array_equal(info["steps"][m], info0["steps"][m]) for m in range(M))
    again = _vjp(icnf, case, ps, xs, eps, cot, bases=b, with_base=True)
    for u, v in zip((lp, rg, g, gx, gb[0], gb[1]), again[:4] + again[5]):
        assert np.array_equal(u, v)
    if "rejects" in case.name:
        assert info["stats"][0]["nreject"] >= 1, info["stats"]
    # member m of the M = 3 call is the M = 1 call on its slices, bases included, bit for bit (logpx, regularisers, gradients, and
    # the base's own gradient: the post pass and the pullback work member by member)
    for m in range(M):
        sub = R.Case(case.name, case.cfg, case.B, train=case.train, jvp=case.jvp, sol_kw=case.sol_kw,
                     t1=case.t1[m:m + 1] if case.t1 is not None else None)
        one = _vjp(icnf, sub, ps[m:m + 1], xs[m:m + 1], eps[m:m + 1], cot[m:m + 1], bases=_bases(case, kind, slice(m, m + 1))[0], with_base=True)
        for u, v in zip((lp[m], rg[m], g[m], gx[m], gb[0][m], gb[1][m]), (one[0][0], one[1][0], one[2][0], one[3][0], one[5][0][0], one[5][1][0])):
            assert np.array_equal(u, v), (case.name, kind, m)
    im = _inference(icnf, case, ps, xs, eps, bases=b)
    for m in range(M):
        sub = R.Case(case.name, case.cfg, case.B, train=case.train, jvp=case.jvp, sol_kw=case.sol_kw,
                     t1=case.t1[m:m + 1] if case.t1 is not None else None)
        io = _inference(icnf, sub, ps[m:m + 1], xs[m:m + 1], eps[m:m + 1], bases=_bases(case, kind, slice(m, m + 1))[0])
        assert np.array_equal(io[0][0], im[0][m]) and np.array_equal(io[1][0], im[1][m]) and io[2]["losses"][0] == im[2]["losses"][m]
    icnf.close()


def test_a_one_hot_sample_cotangent_leaves_the_other_columns_zero():
    case, kind = EB.BY_NAME["readme-vjp-B33"], "dense"
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    b, _, _ = _bases(case, kind)
    j = 20
    hot = np.zeros((M, 4, case.B), np.float32)
    hot[:, :, j] = [0.3, -0.2, 0.1, 0.05]
    _, _, g, gx, _ = _vjp(icnf, case, ps, xs, eps, hot, bases=b)
    assert np.abs(gx[:, :, j]).min() > 0 and g.any(axis=1).all()
    assert not np.delete(gx, j, axis=2).any()
    icnf.close()


def _lag(icnf, case, ps, xs, eps, t1="case", **kw):
    res = cnf.loss_and_grad_many(icnf, _mode(case.train), _dev(xs), _dev(ps), {}, eps=_eps(case, eps),
                                 t1=_t1(case) if isinstance(t1, str) else t1, with_steps=True, **kw)
    out = (res[0], res[1].cpu().numpy(), res[2])
    return out + (_np(*res[3]),) if len(res) > 3 else out


@pytest.mark.parametrize("case,kind", EB.CASE_KINDS, ids=EB.IDS)
def test_loss_and_grad_many_with_bases(case, kind):
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    val, g, info, gb = _lag(icnf, case, ps, xs, eps, bases=b, with_base=True)
    assert info["launches"] == 3 and info["calls"] == 1 and not info["rerun"] and (info["status"] == _lib.OK).all(), info
    val0, g0, info0 = _lag(icnf, case, ps, xs, eps)
    t1 = _t1(case)
    for m in range(M):
        what = f"loss_and_grad_many bases {case.name} {kind} member {m}"
        assert np.array_equal(info["steps"][m], info0["steps"][m])
        cot = V.loss_cotangent(R.member_cfg(case, m), case.B, case.train).astype(np.float32)
        dts = info["steps"][m]
        out, r64, r32 = EB.reference(case, m, ps, xs, eps, cot, dts, EB.gauss(mean, scale, kind, m))
        V.assert_vjp(g[m], None, r64, r32, case.cfg.net, what)
        want = EB.loss_of(case, m, out)
        assert abs(val[m] - want) <= 1e-5 * max(1.0, abs(want)), (what, val[m], want)
        b64, b32, summands = EB.base_reference(case, m, ps, xs, eps, cot[0], dts, mean, scale, kind)
        BG.assert_base((gb[0][m], gb[1][m]), b64, b32, summands, what)
        # member m of the M = 3 call is the M = 1 call on its slices, bases included, bit for bit
        one = _lag(icnf, case, ps[m:m + 1], xs[m:m + 1], eps[m:m + 1], t1=t1[m:m + 1] if t1 is not None else None,
                   bases=_bases(case, kind, slice(m, m + 1))[0], with_base=True)
        assert np.array_equal(one[0][0], val[m]) and np.array_equal(one[1][0], g[m]), what
        assert np.array_equal(one[3][0][0], gb[0][m]) and np.array_equal(one[3][1][0], gb[1][m]), what
    assert np.array_equal(g[UNIT], g0[UNIT])               # (0, I): the gradient of the call without bases, bit for bit
    assert abs(val[UNIT] - val0[UNIT]) <= 1e-5 * max(1.0, abs(val0[UNIT]))
    icnf.close()


def test_ragged_members_with_lambdas_and_bases_are_the_single_member_calls():
    name, kind, counts = EB.RAGGED
    case = EB.BY_NAME[name]
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    cnt, lam, t1 = np.asarray(counts), EB.RAGGED_LAMBDAS, _t1(case)
    val, g, info, gb = _lag(icnf, case, ps, xs, eps, bases=b, with_base=True, counts=cnt, lambdas=lam)
    lp, rg, iinfo = _inference(icnf, case, ps, xs, eps, bases=b, counts=cnt, lambdas=lam)
    for m in range(M):
        k = int(cnt[m])
        one = _lag(icnf, case, ps[m:m + 1], xs[m:m + 1, :, :k], eps[m:m + 1, :, :k], t1=t1[m:m + 1], lambdas=lam[m:m + 1],
                   bases=_bases(case, kind, slice(m, m + 1))[0], with_base=True)
        what = f"ragged bases member {m} (count {k})"
        assert np.array_equal(one[0][0], val[m]) and np.array_equal(one[1][0], g[m]), what
        # columns behind a count contribute nothing to the base's gradient: the M = 1 call at that count, bit for bit
        assert np.array_equal(one[3][0][0], gb[0][m]) and np.array_equal(one[3][1][0], gb[1][m]), what
        assert np.isnan(lp[m, k:]).all() and np.isfinite(lp[m, :k]).all()
        sub = R.Case(case.name, case.cfg, k, t1=case.t1, seed=case.seed)
        out = V.outputs(R.member_cfg(case, m), ps[m].astype(np.float64), xs[m, :, :k].astype(np.float64), eps[m, :, :k].astype(np.float64),
                        _accepted(iinfo["steps"][m]), train=True, base=EB.gauss(mean, scale, kind, m))[0]
        assert_parity(lp[m, :k], out[0], f"{what} logpx")
        want = EB.loss_of(sub, m, out, lam[m])
        assert abs(iinfo["losses"][m] - want) <= 1e-5 * max(1.0, abs(want)), (what, iinfo["losses"][m], want)
    icnf.close()


@pytest.mark.parametrize("name,kind,n", [("readme-vjp-B33", "dense", 33), ("id2-vjp-B17", "diag", 17)])
def test_sampling_through_the_members_bases(name, kind, n):
    case = EB.BY_NAME[name]
    icnf = _icnf(case)
    ps, _, _ = R.inputs(case)
    normals, eps = EB.sampling_inputs(case, n)
    b, mean, scale = _bases(case, kind)
    rng = np.random.default_rng(77)
    cz = (rng.standard_normal((M, case.cfg.n_in, n)) / n).astype(np.float32)
    cl = (rng.standard_normal((M, n)) / n).astype(np.float32)
    x, lq, g, gz0, info, gb = cnf.generate_vjp_many(icnf, cnf.TrainMode(), _dev(ps), {}, n, (_dev(cz), _dev(cl)), eps=_dev(eps),
                                                    normals=_dev(normals), bases=b, with_z0=True, with_base=True, with_steps=True)
    assert not info["rerun"] and (info["status"] == _lib.OK).all(), info
    x, lq, g, gz0, gm, gs = _np(x, lq, g, gz0, *gb)
    z0 = info["z0"].cpu().numpy()
    xs2, lq2 = cnf.generate_many(icnf, cnf.TrainMode(), _dev(ps), {}, n, eps=_dev(eps), normals=_dev(normals), bases=b, with_logp=True)
    assert np.array_equal(icnf.last_ensemble_info["z0"].cpu().numpy(), z0)
    for m in range(M):
        what = f"sampling bases {name} {kind} member {m}"
        # z0: bit for bit cnf_base_sample of a single handle constructed with that member's base, on the same normals
        single = make_icnf(cnf, case.cfg, jvp=case.jvp, kernel="mfma", sol_kwargs=dict(case.sol_kw))
        single.basedist = b[m]
        flat = _dev(normals[m].T).reshape(-1)
        want = cnf.base_icnf.base_sample(single, flat, n).view(n, case.cfg.n_in).t().cpu().numpy()
        single.close()
        assert np.array_equal(z0[m], want), what
        dts = info["steps"][m]
        gauss = EB.gauss(mean, scale, kind, m)
        zf, lq64, _, _ = EB.sampling_forward(case, m, ps, z0[m], eps, dts, gauss)
        assert_parity(x[m], zf[:case.cfg.nvars], f"{what} xs")
        assert_parity(lq[m], lq64, f"{what} logq")
        assert_parity(xs2[m].cpu().numpy(), zf[:case.cfg.nvars], f"{what} xs (generate_many)")
        assert_parity(lq2[m].cpu().numpy(), lq64, f"{what} logq (generate_many)")
        r64 = EB.sampling_reference(case, m, ps, normals, eps, cz[m], cl[m], dts, mean, scale, kind, np.float64)
        r32 = EB.sampling_reference(case, m, ps, normals, eps, cz[m], cl[m], dts, mean, scale, kind, np.float32)
        s = V.scale(r64[2])
        floor = np.abs(r32[2] - r64[2]).max() / s
        rtol = max(V.RTOL, V.FLOOR_FACTOR * floor)
        err = np.abs(gz0[m] - r64[2]).max() / s
        print(f"{what}: grad_z0 err {err:.2e} floor {floor:.2e} rtol {rtol:.1e}")
        assert rtol <= V.RTOL_CAP and err <= rtol, (what, err, floor, rtol)
        BG.assert_base((gm[m], gs[m]), r64[:2], r32[:2], None, what)
        # the parameter gradient: gen_vjp_ref with base=, from the drawn z0, through the device's own steps
        g64, g32 = EB.sampling_grads(case, m, ps, normals, eps, cz[m], cl[m], dts, mean, scale, kind)
        V.assert_vjp(g[m], None, (g64, None), (g32, None), case.cfg.net, f"{what} grads")
        # member m of the M = 3 call is the M = 1 call on its slices, bases included, bit for bit
        one = cnf.generate_vjp_many(icnf, cnf.TrainMode(), _dev(ps[m:m + 1]), {}, n, (_dev(cz[m:m + 1]), _dev(cl[m:m + 1])),
                                    eps=_dev(eps[m:m + 1]), normals=_dev(normals[m:m + 1]), bases=_bases(case, kind, slice(m, m + 1))[0],
                                    with_z0=True, with_base=True)
        for u, v in zip((x[m], lq[m], g[m], gz0[m], gm[m], gs[m]), _np(one[0][0], one[1][0], one[2][0], one[3][0], one[5][0][0], one[5][1][0])):
            assert np.array_equal(u, v), what
    icnf.close()


def test_autograd_reaches_the_bases_without_a_host_upload(monkeypatch):
    case, kind = EB.BY_NAME["id2-vjp-B17"], "diag"
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    mean, scale = EB.bases(case, kind)
    l = _lib.lib()
    uploads = []
    real = l.cnf_set_basedist
    monkeypatch.setattr(l, "cnf_set_basedist", lambda *a: (uploads.append(1), real(*a))[1])
    mu = _dev(mean).requires_grad_(True)
    log_std = _dev(np.log(scale)).requires_grad_(True)
    p = _dev(ps).requires_grad_(True)
    w = _dev(np.random.default_rng(3).standard_normal((M, case.B)) / case.B)
    opt = torch.optim.SGD([mu, log_std], lr=1e-3)
    wn = w.cpu().numpy().astype(np.float64)
    seen = []
    for it in range(3):                                    # the initial values, then the values behind each of two optimiser steps
        opt.zero_grad()
        p.grad = None                                      # (the parameters are no business of this optimiser: nothing accumulates)
        b = cnf.EnsembleBases(mu, std=log_std.exp())
        lp, _ = cnf.differentiable_inference_many(icnf, cnf.TrainMode(), _dev(xs), p, {}, eps=_dev(eps), bases=b)
        loss = (w * lp).sum()
        loss.backward()
        # the .grads are the explicit pullback's, through the chain std = exp(log_std)
        res = cnf.inference_vjp_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {}, (w, None), eps=_dev(eps),
                                     bases=cnf.EnsembleBases(mu.detach(), std=log_std.detach().exp()), with_base=True)
        gm, gs = res[-1]
        assert torch.equal(mu.grad, gm) and torch.equal(p.grad, res[2])
        assert torch.allclose(log_std.grad, gs * log_std.detach().exp(), rtol=1e-6, atol=0)
        # the float64 reference AT THE CURRENT (mu, log_std), through the steps the device accepted: the outputs are what it says
        # they should be behind every step, and so is the base's gradient
        mean_i = mu.detach().cpu().numpy()
        scale_i = log_std.detach().exp().cpu().numpy()
        want_loss = 0.0
        for m in range(M):
            dts = cnf.ensemble_steps(icnf, m)
            out = V.outputs(R.member_cfg(case, m), ps[m].astype(np.float64), xs[m].astype(np.float64), eps[m].astype(np.float64), dts,
                            train=True, base=EB.gauss(mean_i, scale_i, kind, m))[0]
            assert_parity(lp[m].detach().cpu().numpy(), out[0], f"autograd step {it} member {m} logpx")
            want_loss += float((wn[m] * out[0]).sum())
            b64, b32, summands = EB.base_reference(case, m, ps, xs, eps, wn[m].astype(np.float32), dts, mean_i, scale_i, kind)
            BG.assert_base((gm[m].cpu().numpy(), gs[m].cpu().numpy()), b64, b32, summands, f"autograd step {it} member {m}")
        got_loss = float(loss.detach())
        # (the values bar on a weighted sum: |w| . (rtol |logpx| + atol))
        bar = float((np.abs(wn) * (helpers.RTOL * np.abs(lp.detach().cpu().numpy()) + helpers.ATOL)).sum())
        assert abs(got_loss - want_loss) <= bar, (it, got_loss, want_loss, bar)
        seen.append((got_loss, mean_i.copy(), scale_i.copy()))
        opt.step()
    assert seen[0][0] != seen[1][0] != seen[2][0] and not np.array_equal(seen[0][1], seen[2][1]) and not np.array_equal(seen[0][2], seen[2][2])
    assert not uploads, "a learnable base of an ensemble call must not go through cnf_set_basedist"
    # reverse_kl_many: M restarts, each with its own location-scale family; the .grads are the explicit total pullback's
    n = 17
    mu2, ls2 = _dev(mean).requires_grad_(True), _dev(np.log(scale)).requires_grad_(True)
    target = lambda x: -0.5 * (x * x).sum(dim=1)
    kl = cnf.reverse_kl_many(icnf, cnf.TrainMode(), _dev(ps), {}, n, target, bases=cnf.EnsembleBases(mu2, std=ls2.exp()))
    kl.sum().backward()
    info = icnf.last_ensemble_info
    xs_b = icnf.last_backward_xs
    res = cnf.generate_vjp_many(icnf, cnf.TrainMode(), _dev(ps), {}, n, (xs_b / n, torch.full((M, n), 1.0 / n, device="cuda")),
                                normals=info["normals"], eps=info["eps"], bases=cnf.EnsembleBases(mu2.detach(), std=ls2.detach().exp()),
                                with_base=True)
    # (g_x comes from the forward launch's samples there and from the backward launch's here: the two differ in the last bits)
    for got, want in ((mu2.grad, res[-1][0]), (ls2.grad, res[-1][1] * ls2.detach().exp())):
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), (got, want)
    assert mu2.grad.abs().min() > 0 and torch.isfinite(ls2.grad).all() and not uploads
    icnf.close()


@pytest.mark.parametrize("name,kind", [("readme-vjp-B33", "dense"), ("regr-test-B17", "diag")])
def test_the_single_model_with_that_base_agrees(name, kind):
    """The other route: ``inference`` / ``loss_and_grad`` on a model constructed with ``basedist = bases[m]`` (the recorded solve
    and the streamed pullback; other kernels, their own accepted steps)."""
    case = EB.BY_NAME[name]
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    b, _, _ = _bases(case, kind)
    lp, _, info = _inference(icnf, case, ps, xs, eps, bases=b)
    val, g, _ = _lag(icnf, case, ps, xs, eps, bases=b)
    same = True
    for m in range(M):
        single = make_icnf(cnf, R.member_cfg(case, m), jvp=case.jvp, kernel="mfma", sol_kwargs=dict(case.sol_kw))
        single.basedist = b[m]
        kw = dict(eps=_dev(eps[m])) if case.train else {}
        lp1, _ = cnf.inference(single, _mode(case.train), _dev(xs[m]), _dev(ps[m]), {}, **kw)
        v1, g1 = cnf.loss_and_grad(single, _mode(case.train), _dev(xs[m]), _dev(ps[m]), {}, **kw)
        lp1, g1 = lp1.cpu().numpy(), g1.cpu().numpy()
        assert_parity(lp[m], lp1.astype(np.float64), f"cross-route {name} member {m} logpx")
        scale = np.abs(g1).max() + np.sqrt(np.mean(g1.astype(np.float64) ** 2))
        err = np.abs(g[m] - g1).max() / scale
        print(f"cross-route {name} {kind} member {m}: gradient difference {err:.2e} of its scale, loss {val[m]} vs {v1}")
        assert err <= 1e-4 and abs(val[m] - v1) <= 1e-5 * max(1.0, abs(v1)), (name, m, err, val[m], v1)
        same = same and np.array_equal(lp[m], lp1) and np.array_equal(g[m], g1)
        single.close()
    if same:
        helpers.note(f"ensemble bases {name} {kind}: the single-model route gives the same bits")
    icnf.close()


def test_splits_reruns_and_refusals(monkeypatch):
    case, kind = EB.BY_NAME["regr-vjp-B17-rejects"], "dense"
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    rng = np.random.default_rng(8)
    cot = (rng.standard_normal((M, 4, case.B)) / case.B).astype(np.float32)
    base = _vjp(icnf, case, ps, xs, eps, cot, bases=b, with_base=True)
    ibase = _inference(icnf, case, ps, xs, eps, bases=b)
    # pending bases with the wrong M: CNF_ERR_BAD_ARG, nothing enqueued, the bases consumed
    l, h = _lib.lib(), icnf.handle()
    dm, ds = _dev(mean), _dev(scale)
    assert l.cnf_ensemble_set_bases(h, M - 1, 2, dm.data_ptr(), ds.data_ptr(), None) == _lib.OK
    with pytest.raises(_lib.CNFError) as e:
        _inference(icnf, case, ps, xs, eps)
    assert e.value.status == _lib.ERR_BAD_ARG
    again = _inference(icnf, case, ps, xs, eps)             # (consumed: this call has none)
    assert (again[2]["status"] == _lib.OK).all() and not np.array_equal(again[0], ibase[0])
    # ... and the path calls never ignore them silently
    assert l.cnf_ensemble_set_bases(h, M, 2, dm.data_ptr(), ds.data_ptr(), None) == _lib.OK
    with pytest.raises(_lib.CNFError) as e:
        cnf.inference_path_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {}, saveat=[1.0], eps=_dev(eps))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    lp_plain = cnf.inference_path_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {}, saveat=[1.0], eps=_dev(eps))[0]
    assert torch.isfinite(lp_plain).all()                  # (consumed: the next path call runs)
    with pytest.raises(NotImplementedError, match="bases"):
        cnf.inference_path_many(icnf, cnf.TrainMode(), _dev(xs), _dev(ps), {}, saveat=[1.0], eps=_dev(eps), bases=b)
    # a non-positive sigma in device tensors: the device marks the member, the call names it
    bad = np.ones((M, case.cfg.n_in), np.float32)
    bad[2, 3] = -1.0
    with pytest.raises(_lib.CNFError, match="member 2") as e:
        _inference(icnf, case, ps, xs, eps, bases=cnf.EnsembleBases(_dev(mean), std=_dev(bad)))
    assert e.value.status == _lib.ERR_BAD_ARG
    with pytest.raises(ValueError, match="member 2"):
        cnf.EnsembleBases(mean, std=bad)
    # a model with a base of its own is refused as before
    own = _icnf(case)
    own.basedist = b[0]
    with pytest.raises(NotImplementedError, match="basedist"):
        cnf.inference_many(own, cnf.TrainMode(), _dev(xs), _dev(ps), {}, eps=_dev(eps), bases=b)
    # members that give up are run again with their base (the knob of the existing fallback tests: a bounded wait)
    icnf.set_solve_wait(poll_limit=1)
    try:
        r_lp, _, r_info = _inference(icnf, case, ps, xs, eps, bases=b)
    finally:
        icnf.set_solve_wait(poll_limit=0x7fffffff)
    assert r_info["rerun"], r_info
    for m in r_info["rerun"]:
        assert_parity(r_lp[m], ibase[0][m].astype(np.float64), f"rerun with its base, member {m}")
    # the split: a capacity of two members per launch, the bases sliced with the members
    monkeypatch.setattr(ens_mod, "_device_capacity", lambda *a: 2)
    s = _vjp(icnf, case, ps, xs, eps, cot, bases=b, with_base=True)
    assert s[4]["calls"] == 2
    for u, v in zip(base[:4] + base[5], s[:4] + s[5]):
        assert np.array_equal(u, v)
    si = _inference(icnf, case, ps, xs, eps, bases=b)
    assert si[2]["calls"] == 2 and np.array_equal(si[0], ibase[0])
    icnf.close(); own.close()


def test_ensemble_dist_is_a_mixture_of_components_in_different_places():
    case, kind = EB.BY_NAME["readme-vjp-B33"], "dense"
    icnf = make_icnf(cnf, case.cfg, kernel="mfma")
    ps, xs, _ = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    w = np.asarray([0.5, 0.3, 0.2])
    d = cnf.EnsembleDist(icnf, cnf.TestMode(), _dev(ps), weights=w, bases=b)
    A = _dev(xs[0])
    members = cnf.inference_many(icnf, cnf.TestMode(), A, _dev(ps), {}, bases=b)[0]
    assert torch.equal(d.logpdf_members(A), members)
    assert torch.equal(d.logpdf(A), cnf.ensemble.mixture_logpdf(members, w))
    plain = cnf.EnsembleDist(icnf, cnf.TestMode(), _dev(ps), weights=w).logpdf(A)
    assert not torch.equal(plain, d.logpdf(A))
    # rand draws through the bases: the same seed without bases gives other samples, and the base samples are mean + L n
    icnf.rng = np.random.default_rng(5)
    x = d.rand(40)
    z0, nrm = icnf.last_ensemble_info["z0"].cpu().numpy(), icnf.last_ensemble_info["normals"].cpu().numpy()
    for m in range(M):
        want = BG.drawn_z0(nrm[m], mean[m], scale[m], True, np.float64)
        assert_parity(z0[m], want, f"EnsembleDist.rand member {m}: z0 = mean + L n")
    icnf.rng = np.random.default_rng(5)
    x0 = cnf.EnsembleDist(icnf, cnf.TestMode(), _dev(ps), weights=w).rand(40)
    assert np.array_equal(icnf.last_ensemble_info["z0"].cpu().numpy(), nrm)      # (the draws the default makes, at the same offsets)
    assert x.shape == x0.shape == (case.cfg.nvars, 40) and torch.isfinite(x).all() and not torch.equal(x, x0)
    icnf.close()


def test_a_rerun_member_returns_its_bases_gradient_too():
    """A member whose part of the launch gave up (a bounded wait, the knob of the existing fallback tests) is run again on a twin
    whose ``basedist`` is a ``LearnableNormal`` over its base: loss, gradient and (g_mean, g_scale) are the single-model route's."""
    case, kind = EB.BY_NAME["regr-vjp-B17-rejects"], "dense"
    icnf = _icnf(case)
    ps, xs, eps = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    val, g, info, gb = _lag(icnf, case, ps, xs, eps, bases=b, with_base=True)
    icnf.set_solve_wait(poll_limit=1)
    try:
        rval, rg, rinfo, rgb = _lag(icnf, case, ps, xs, eps, bases=b, with_base=True)
    finally:
        icnf.set_solve_wait(poll_limit=0x7fffffff)
    assert rinfo["rerun"], rinfo
    for m in rinfo["rerun"]:
        what = f"rerun with its base and with_base, member {m}"
        assert abs(rval[m] - val[m]) <= 1e-5 * max(1.0, abs(val[m])), (what, rval[m], val[m])
        cot = V.loss_cotangent(R.member_cfg(case, m), case.B, case.train).astype(np.float32)
        dts = rinfo["steps"][m]
        _, r64, r32 = EB.reference(case, m, ps, xs, eps, cot, dts, EB.gauss(mean, scale, kind, m))
        V.assert_vjp(rg[m], None, r64, r32, case.cfg.net, what)
        b64, b32, summands = EB.base_reference(case, m, ps, xs, eps, cot[0], dts, mean, scale, kind)
        BG.assert_base((rgb[0][m], rgb[1][m]), b64, b32, summands, what)
    icnf.close()


def test_fit_many_keeps_the_bases_constant_and_trains_under_them():
    rng = np.random.default_rng(5)
    Xs = [(2.0 * k + rng.beta(2.0, 4.0, size=(64, 1))).astype(np.float32) for k in range(M)]
    mk = lambda: cnf.construct(cnf.RNODE, cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh")), 1, 1, rng=21, lambda3=1e-2,
                               compute_mode=cnf.HIPVecJacMatrixMode("mfma"))
    fit = lambda **kw: cnf.fit_many(cnf.ICNFModel(mk(), optimizers=(cnf.Adam(eta=2e-2),), n_epochs=2, batch_size=32), 0, Xs,
                                    seeds=[10, 11, 12], **kw)
    plain, rep0 = fit()
    # bases of exactly (0, I): the gradients are the call's without bases bit for bit, hence the same trajectory of parameters
    unit, rep1 = fit(bases=cnf.EnsembleBases(np.zeros((M, 2)), std=np.ones((M, 2))))
    assert all(np.array_equal(a[0], c[0]) for a, c in zip(plain, unit))
    # each fold standardised by its own rows, inside the density
    mean = np.stack([[X.mean(), 0.0] for X in Xs])
    std = np.stack([[X.std(), 1.0] for X in Xs])
    bases = cnf.EnsembleBases(mean, std=std)
    fitted, rep2 = fit(bases=bases)
    assert np.isfinite(rep2["losses"]).all() and rep2["losses"].shape == rep0["losses"].shape
    # the first iteration is loss_and_grad_many under the bases, at the members' initial parameters and first batches (the draws
    # of fit_many, made again: setup, then the permutation, from the member's generator; the probes from a fresh model's)
    from continuousnf.jl_amd.layers import setup
    model = cnf.ICNFModel(mk(), optimizers=(cnf.Adam(eta=2e-2),), n_epochs=2, batch_size=32)
    gens = [np.random.default_rng(sd) for sd in (10, 11, 12)]
    ps0 = np.stack([setup(gn, model.m.nn, init=model.init)[0] for gn in gens])
    xb = np.stack([X.T[:, gn.permutation(64)[:32]] for X, gn in zip(Xs, gens)])
    first = cnf.loss_and_grad_many(model.m, cnf.TrainMode(), _dev(xb), _dev(ps0), {}, bases=bases)[0]
    assert np.array_equal(first, rep2["losses"][:, 0]), (first, rep2["losses"][:, 0])
    assert not np.array_equal(rep2["losses"][:, 0], rep0["losses"][:, 0])
    assert np.array_equal(bases.mean, mean) and np.array_equal(bases.scale, std)          # (kept constant)
    # ... and other parameters at the end
    assert not any(np.array_equal(a[0], c[0]) for a, c in zip(plain, fitted))


def test_ensemble_dist_rand_ragged_takes_the_bases_of_the_live_members():
    case, kind = EB.BY_NAME["readme-vjp-B33"], "dense"
    icnf = make_icnf(cnf, case.cfg, kernel="mfma")
    ps, _, _ = R.inputs(case)
    b, mean, scale = _bases(case, kind)
    d = cnf.EnsembleDist(icnf, cnf.TestMode(), _dev(ps), weights=np.asarray([0.0, 0.0, 1.0]), bases=b)       # a one-hot mixture
    icnf.rng = np.random.default_rng(9)
    x, who = d.rand(24, with_members=True, ragged=True)
    info = icnf.last_ensemble_info
    assert (who == 2).all() and x.shape == (case.cfg.nvars, 24) and len(info["status"]) == 1
    z0, nrm = info["z0"].cpu().numpy(), info["normals"].cpu().numpy()
    assert_parity(z0[0], BG.drawn_z0(nrm[0], mean[2], scale[2], True, np.float64), "rand(ragged=True): the live member's own base")
    icnf.close()
