"""The KKT certificate (tests/kkt_certificate.py), CPU side: it passes the QP's exact solutions and the oracle's answers, it fails on
answers that are subtly wrong, and it rejects what a pin without weight (ndp_cfg.as_gamma ~ 0) produces.

tests/test_kkt_certificate_gpu.py holds every status-0 step of the device to it."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import ref_numpy as R
from tests.kkt_certificate import NU, NX, certificate, worst

MIXED = dict(pos_sigma=0.5, vel_sigma=1.0, quat_sigma=0.15)        # bench.py's `mixed` workload: ~20 % of the instances hit an input bound
HARD = dict(pos_sigma=1.5, vel_sigma=3.0, quat_sigma=0.2)          # test_active_bounds_and_infeasible_start's
WORKLOADS = dict(nominal={}, mixed=MIXED, hard=HARD)


def _qps(oracle, N, kw, B, seed=synth.SEED0 + 40):
    b = synth.make_batch(B, N=N, seed=seed, **kw)
    cfg = oracle.default_cfg(N=N)
    return [oracle.linearize(cfg, b["x0"][i], b["xr"][i], b["ur"][i], None, b["xr"][i], b["ur"][i]) for i in range(B)]


@pytest.mark.parametrize("N", [13, 20, 40])
@pytest.mark.parametrize("work", ["nominal", "mixed", "hard"])
def test_exact_and_oracle_answers_pass(oracle, N, work):
    """The exact dense-KKT solution (R.pdas_solve) and the oracle's active-set answer (qp_mode 0) pass at 1e-11 -- measured 2.4e-13 and
    1.6e-12 at worst; the implied active set is the exact one.  The oracle's interior-point answer at tol 1e-11 stops with a slack mu / lam
    on a bound whose multiplier lam is small, and the natural residual sees that distance: 3.4e-11 (mixed), 6e-9 (hard, N = 40) measured
    -- bars 1e-10 and 2e-8.  No instance of these workloads has a velocity within 1e-6 of its bound (none flagged)."""
    B = 12 if N < 40 else 8
    twin = oracle.default_cfg(N=N)
    twin.qp_mode = 0
    tight = oracle.default_cfg(N=N)
    tight.tol = 1e-11
    n_act = n_ipm = 0
    for qp in _qps(oracle, N, WORKLOADS[work], B):
        dx, du, active = R.pdas_solve(qp)
        c = certificate(qp, dx, du)
        assert not c["flag"] and worst(c) <= 1e-11, (c["eq"], c["stat"], c["vbox"])
        want = np.zeros((N, NU), dtype=np.int8)
        for v, side in active.items():
            if v >= (N + 1) * NX:
                want.reshape(-1)[v - (N + 1) * NX] = 1 if side == "hi" else -1
        assert np.array_equal(c["act"], want)
        n_act += bool(want.any())
        dxo, duo, st = oracle.qp_solve_as(twin, qp)
        assert st.status == 0
        c = certificate(qp, dxo, duo)
        assert not c["flag"] and worst(c) <= 1e-11 and np.array_equal(c["act"], want), (c["eq"], c["stat"])
        dxi, dui, st = oracle.qp_solve(tight, qp)
        if st.status == 0:
            n_ipm += 1
            c = certificate(qp, dxi, dui)
            assert not c["flag"] and worst(c) <= (2e-8 if work == "hard" else 1e-10), (c["eq"], c["stat"])
    assert n_ipm >= B // 2
    if work != "nominal":
        assert n_act >= 1


def _pinned_instance(oracle):
    """A mixed-workload QP whose exact solution has inputs on their bounds, with that solution and the pins' multipliers."""
    for qp in _qps(oracle, 20, MIXED, 16):
        dx, du, active = R.pdas_solve(qp)
        if len(active) >= 2:
            table = {v: (lo, hi) for v, lo, hi in R.bound_table(qp)}
            fixed = [(v, table[v][1] if side == "hi" else table[v][0]) for v, side in sorted(active.items())]
            return qp, dx, du, fixed
    raise AssertionError("no instance with two pins")


def test_mutants_fail(oracle):
    """Each of four subtly wrong answers fails the certificate by orders of magnitude more than the bar (1e-11) -- while the exact answer
    they are made from passes."""
    qp, dx, du, fixed = _pinned_instance(oracle)
    N, base = qp["A"].shape[0], (qp["A"].shape[0] + 1) * NX
    assert worst(certificate(qp, dx, du)) <= 1e-11
    # one du moved by 1e-6
    k, i = 7, 2
    du1 = du.copy()
    du1[k, i] += 1e-6
    assert worst(certificate(qp, dx, du1)) > 1e-9
    # a pinned input released: the rest of the solution as if it were free -- it leaves the box
    dx2, du2, _ = R.kkt_solve(qp, fixed[1:])
    c = certificate(qp, dx2, du2)
    assert c["stat"] > 1e-6
    # a pin with the wrong sign: a free input pinned at its upper bound, below which its optimum lies -- the multiplier pushes it UP
    v = next(v for v in range(base, base + N * NU) if v not in dict(fixed))
    kk, ii = divmod(v - base, NU)
    hi = qp["uu"][kk, ii]
    dx3, du3, mult = R.kkt_solve(qp, fixed + [(v, hi)])
    assert mult[-1] > 0 and du[kk, ii] < hi                          # (a lower bound's multiplier on an upper bound)
    c = certificate(qp, dx3, du3)
    assert c["stat"] > 1e-6 and c["act"][kk, ii] == 1
    # one dynamics row broken by 1e-8: the exact solution of the QP with b_k[j] + 1e-8, held to the true QP
    qpb = dict(qp)
    qpb["b"] = qp["b"].copy()
    qpb["b"][11, 4] += 1e-8
    dx4, du4, _ = R.kkt_solve(qpb, fixed)
    c = certificate(qp, dx4, du4)
    assert c["eq"] > 1e-10 and worst(certificate(qpb, dx4, du4)) <= 1e-11


def test_weightless_pins_are_rejected(oracle):
    """as_gamma = 1e-3 on the oracle's twin of the device's pin rule (qp_mode 0, ndp_oracle.c's active-set loop), 40 mixed instances: a
    pinned input is written onto its bound, yet the rest of the QP was solved with it free.  Every instance reports status 0, 7 of them
    hold pins, and their inputs are up to 1.9 off the exact solution: the certificate fails exactly those 7.  With the default
    as_gamma (1e12) all 40 pass.  (ndp_create refuses such an as_gamma: test_host_logic.py.)"""
    B = 40
    b = synth.make_batch(B, seed=synth.SEED0 + 40, **MIXED)
    cfgl = oracle.default_cfg()
    qps = [oracle.linearize(cfgl, b["x0"][i], b["xr"][i], b["ur"][i], None, b["xr"][i], b["ur"][i]) for i in range(B)]
    for gamma in (1e12, 1e-3):
        c = oracle.default_cfg()
        c.qp_mode = 0
        c.as_gamma = gamma
        X, U = b["xr"].copy(), b["ur"].copy()
        act = np.zeros((B, 20, NU), dtype=np.int8)
        _, st, it, _ = oracle.step_batch_as(c, b["x0"], b["xr"], b["ur"], None, X, U, act)
        assert not st.any() and not it.any()
        pinned = act.any(axis=(1, 2))
        assert pinned.sum() == 7
        res = np.array([worst(certificate(qps[i], X[i] - b["xr"][i], U[i] - b["ur"][i])) for i in range(B)])
        err = np.array([np.abs(U[i] - b["ur"][i] - R.pdas_solve(qps[i])[1]).max() for i in np.flatnonzero(pinned)])
        if gamma == 1e12:
            assert res.max() <= 1e-11 and err.max() < 1e-10
        else:
            assert res[~pinned].max() <= 1e-11 and res[pinned].min() > 1e-3, res[pinned]
            assert 1.5 < err.max() < 2.5
