"""Forward mode of the control step along directions of the cost weights and the mass (RtiWave::jvp_out<true>, rti_mjvp_kernel) without a
GPU.  First the float64 references of tests/model_jvp_ref.py are held themselves: against central differences of the oracle's step in the
model and, by duality, against fixed_set_ref.model_grad_ref and closed_loop_vjp_ref.model_reverse.  Then the device's code on the host wave
emulator (tests/step_model_jvp_emu.cpp) against them: the dense reference, mixed directions, duality with the emulated model gradient,
exact zeros, T against one, a failed step, the edge horizons; the kernels' ISA and the interface.  The device side:
tests/test_step_model_jvp_gpu.py."""
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import closed_loop_chain_ref as R
from tests import closed_loop_vjp_ref as CV
from tests import fixed_set_ref as F
from tests import model_jvp_ref as MR
from tests.deriv_edges import DERIV_EDGE_N
from tests.step_deriv_emu import MIXED, _jvp, _tape, _vjp, step_emu  # noqa: F401
from tests.step_model_jvp_emu import _mjvp, model_jvp_emu  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BAR = 1e-6                                        # test_device_finite_differences_through_set_model's bar


def _force(rng, N, use_fd):
    return rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32) if use_fd else None


def _f64(f):
    return None if f is None else f.astype(np.float64)


def _tmodel(rng, T):
    """Seeded directions of the model on the scale of the model itself (Qd ~ 10..400, Rd ~ 10, mass ~ 1.5): entries ~ N(0, 1)."""
    return rng.normal(size=(T, 16))


def _flat(dX, dU):
    return np.concatenate([np.asarray(dX).ravel(), np.asarray(dU).ravel()])


# ---------------------------------------------------------------- the references, held on the CPU
def test_step_reference_matches_central_differences_of_the_oracles_step(oracle):
    """N = 13 with a force, the mixed workload: the reference tangent along a unit direction in Qd[0], Qd[8], Rd[3] and the mass against
    central differences (step 1e-5 of the entry) of the oracle's step from the same iterate and kept set, on the instances whose final
    set and iteration word do not change -- within 1e-6 of max(1, |z'|max); the mass column's two step sizes in 1 / m agree to 1e-9."""
    N, B = 13, 5
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = R.twin_cfg(oracle, N)
    rng = np.random.default_rng(11)
    f = rng.normal(0.0, 0.3, (B, N + 1, 3))
    X0 = b["xr"] + 0.01 * rng.normal(size=b["xr"].shape)
    U0 = b["ur"] + 0.01 * rng.normal(size=b["ur"].shape)

    def step(c):
        X, U, act = X0.copy(), U0.copy(), np.zeros((B, N, 4), dtype=np.int8)
        _, st, it, _ = oracle.step_batch_as(c, b["x0"], b["xr"], b["ur"], f, X, U, act)
        return X, U, act, (st == 0) & ((it & 0xffff) == 0)

    _, _, act0, ok0 = step(cfg)
    fds = {}
    stable = ok0.copy()
    for col in (0, 8, 13, 14):
        val = cfg.Qd[col] if col < 10 else cfg.Rd[col - 10] if col < 14 else cfg.mass
        h = 1e-5 * val
        runs = []
        for sgn in (1.0, -1.0):
            c = F.copy_cfg(cfg)
            if col < 10:
                c.Qd[col] = val + sgn * h
            elif col < 14:
                c.Rd[col - 10] = val + sgn * h
            else:
                c.mass = val + sgn * h
            X, U, act, ok = step(c)
            stable &= ok & (act == act0).all(axis=(1, 2))
            runs.append((X, U))
        fds[col] = ((runs[0][0] - runs[1][0]) / (2 * h), (runs[0][1] - runs[1][1]) / (2 * h))
    assert stable.sum() >= 3 and act0[stable].any()
    worst = 0.0
    for i in np.flatnonzero(stable):
        c = MR.model_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i], X0[i], U0[i], act0[i])
        assert np.max(np.abs(c["mcols"][14] - c["mcol_m2"])) <= 1e-9 * F.scale(c["mcols"][14])
        for col, (fX, fU) in fds.items():
            _, rX, rU = MR.model_jvp_apply(c, np.eye(16)[col])
            s = max(F.scale(rX), F.scale(rU))
            err = max(np.max(np.abs(fX[i] - rX)), np.max(np.abs(fU[i] - rU))) / s
            worst = max(worst, err)
            assert err <= FD_BAR, (i, col, err)
            assert max(np.abs(rX).max(), np.abs(rU).max()) > 1e-9        # (a tangent that is there to be compared)
    print(f"worst finite-difference distance {worst:.3e} over {int(stable.sum())} instances")


def test_step_reference_is_dual_to_model_grad_ref(oracle):
    """<gz, z'> = sum_j g[j] theta'_j against fixed_set_ref.model_grad_ref on one system, free and pinned finishes: both are solves with one
    K over the same columns -- within 1e-11 of the largest term."""
    N, B = 13, 4
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = R.twin_cfg(oracle, N)
    rng = np.random.default_rng(12)
    pinned = 0
    for i in range(B):
        X, U, _ = _tape(b, i, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3))
        act = np.zeros((1, N, 4), dtype=np.int8)
        Xn, Un = X[None].copy(), U[None].copy()
        _, st, it, _ = oracle.step_batch_as(cfg, b["x0"][i:i + 1], b["xr"][i:i + 1], b["ur"][i:i + 1], f[None], Xn, Un, act)
        if st[0] != 0 or it[0] & 0xffff:
            continue
        pinned += int(act.any())
        th = _tmodel(rng, 1)[0]
        gu0, gX, gU = rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4))
        g, _ = F.model_grad_ref(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act[0], gu0, gX, gU)
        du0, dX, dU = MR.model_jvp_ref(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act[0], th)
        lhs = [gu0 * du0, gX * dX, gU * dU]
        rhs = g[:15] * th[:15]
        # model_grad_ref zeroes nothing at the pinned rows of its adjoint and the tangent's pinned rows are exactly 0: both leave them out
        mag = max(1.0, max(np.abs(x).max() for x in lhs), np.abs(rhs).max())
        assert abs(sum(x.sum() for x in lhs) - rhs.sum()) <= 1e-11 * mag, (i, sum(x.sum() for x in lhs), rhs.sum())
    assert pinned >= 1


def test_closed_loop_reference_is_dual_to_model_reverse(oracle):
    """ext form, B = 65, K = 3, N = 7 (test_model_gradient_composition_against_the_oracles_closed_loop's record and vehicles): the forward
    sweep along a model direction alone against closed_loop_vjp_ref.model_reverse, <G, dx> + <H, du0> + <A, dX> = <gmodel[v], theta'[v]>
    over all 16 columns, within 1e-10 of the largest term; column 15 alone moves the states and leaves tick 0's du0 exactly 0."""
    K, N, B, T = 3, 7, 65, 2
    a = R.ext_inputs(B, K, N, 20231516)
    rec = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], f=a["f"])
    ok = R.set_finish(rec)
    which = [int(v) for v in np.flatnonzero(ok)[:4]]
    G, H, A = R.upstreams(K, B, N, seed=31)
    cfg = R.twin_cfg(oracle, N)
    sys_ = MR.loop_model_systems(oracle, R.systems(oracle, rec, which), rec, cfg)
    tot, _ = CV.model_reverse(oracle, sys_, rec, G, H, A)
    tm = np.random.default_rng(13).normal(size=(B, T, 16))
    tm[:, 1, :15] = 0.0                                                  # direction 1: the plant's mass alone
    dx, du0, dX = MR.loop_forward(sys_, rec, tm)
    lhs = (np.einsum("kvtc,kvc->vt", dx, G[:, which]) + np.einsum("kvtc,kvc->vt", du0, H[:, which])
           + np.einsum("kvtnc,kvnc->vt", dX, A[:, which]))
    terms = tot[:, None, :] * tm[which]
    gap = np.abs(lhs - terms.sum(axis=2)) / np.maximum(1.0, np.maximum(np.abs(terms).max(axis=2), np.abs(lhs)))
    print(f"worst duality gap of the closed-loop reference {gap.max():.3e}")
    assert gap.max() <= 1e-10, gap
    assert not du0[0, :, 1].any() and np.abs(dx[:, :, 1]).max() > 1e-6


# ---------------------------------------------------------------- the device's code on the emulator
@pytest.mark.parametrize("N,B,use_fd", [(2, 4, False), (2, 3, True), (13, 4, True), (13, 3, False), (20, 6, False), (20, 3, True),
                                        (27, 3, True), (27, 2, False)])
def test_emulated_model_jvp_matches_the_dense_reference(oracle, model_jvp_emu, N, B, use_fd):
    """test_emulated_jvp_matches_the_dense_fixed_set_reference's shapes and workload, one random model direction: every set finish within
    1e-10 of max(1, |z'|max) of model_jvp_ref at the step's final set; dX_0 exactly 0, du0 = dU_0 and pinned rows of dU exactly 0.  The
    same instances along model AND data directions together: the sum of the two references, at the same bar."""
    from tests.emu import emu
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd)
    ocfg = oracle.default_cfg(N=N, use_fd=use_fd)
    rng = np.random.default_rng(400 + N)
    checked = pinned = 0
    worst = worst_mixed = 0.0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, use_fd)
        tm = _tmodel(rng, 1)
        tan = (rng.normal(size=(1, 10)), rng.normal(size=(1, N + 1, 10)), rng.normal(size=(1, N, 4)),
               rng.normal(size=(1, N + 1, 3)) if use_fd else None)
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        u0, Xn, Un, st, it, actn, du0, dX, dU = _mjvp(model_jvp_emu, *args, tm)
        mixed = _mjvp(model_jvp_emu, *args, tm, *tan)
        assert st == 0
        if it & 0xffff:                                  # interior point: the duality test below
            continue
        A = actn.reshape(N, 4)
        pinned += int(A.any())
        c = MR.model_system(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], _f64(f), X, U, A)
        assert np.max(np.abs(c["mcols"][14] - c["mcol_m2"])) <= 1e-9 * F.scale(c["mcols"][14])
        r0, rX, rU = MR.model_jvp_apply(c, tm[0])
        s = max(F.scale(rX), F.scale(rU))
        for got, r in zip((du0[0], dX[0], dU[0]), (r0, rX, rU)):
            worst = max(worst, np.max(np.abs(got - r)) / s)
            assert np.max(np.abs(got - r)) <= 1e-10 * s, (i, np.max(np.abs(got - r)) / s)
        assert not dX[0, 0].any() and np.array_equal(du0[0], dU[0, 0]) and not dU[0][A != 0].any()
        m0, mX, mU = MR.model_jvp_apply(c, tm[0], *(None if t is None else t[0] for t in tan))
        s = max(F.scale(mX), F.scale(mU))
        for got, r in zip((mixed[6][0], mixed[7][0], mixed[8][0]), (m0, mX, mU)):
            worst_mixed = max(worst_mixed, np.max(np.abs(got - r)) / s)
            assert np.max(np.abs(got - r)) <= 1e-10 * s, (i, np.max(np.abs(got - r)) / s)
        assert np.array_equal(mixed[7][0, 0], tan[0][0]) and not mixed[8][0][A != 0].any()
        checked += 1
    print(f"N={N} use_fd={use_fd}: {checked} set finishes, {pinned} pinned, worst distance {worst:.3e}, mixed {worst_mixed:.3e}")
    assert checked >= 2
    if N in (13, 20):
        assert pinned >= 1


@pytest.mark.parametrize("N,use_fd,ipm", [(20, True, False), (13, True, False), (27, False, False), (20, True, True), (13, True, True)])
def test_duality_with_the_emulated_model_gradient(step_emu, model_jvp_emu, N, use_fd, ipm):
    """<gz, JVP(theta', t)> = <VJP(gz), t> + sum_{j<15} gmodel[j] theta'_j against wvjp_emu_step on the same tape, model and data directions
    together: 1e-10 of the largest term on set finishes, 1e-6 on interior-point finishes (ipm: qp_mode 1, the velocity box +-3; at least 3
    finish there)."""
    from tests.emu import emu
    B = 6
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd, qp_mode=1 if ipm else 0)
    if ipm:
        for j in range(3):
            cfg.lbv[j], cfg.ubv[j] = -3.0, 3.0
    rng = np.random.default_rng(500 + N)
    worst = {False: 0.0, True: 0.0}
    count = {False: 0, True: 0}
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, use_fd)
        tm = _tmodel(rng, 1)
        tan = (rng.normal(size=(1, 10)), rng.normal(size=(1, N + 1, 10)), rng.normal(size=(1, N, 4)),
               rng.normal(size=(1, N + 1, 3)) if use_fd else None)
        gu0, gX, gU = rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4))
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        j = _mjvp(model_jvp_emu, *args, tm, *tan)
        a = _vjp(step_emu, *args, gu0, gX, gU, model=True)
        for x, y in zip(j[:6], a[:6]):                   # the recompute is the same step
            assert np.array_equal(x, y)
        assert j[3] == 0
        du0, dX, dU = (v[0] for v in j[6:])
        lhs = [gu0 * du0, gX * dX, gU * dU]
        rhs = [g * t[0] for g, t in zip(a[6:10], tan) if t is not None] + [a[10][:15] * tm[0, :15]]
        mag = max(1.0, max(np.abs(x).max() for x in lhs + rhs))
        err = abs(sum(x.sum() for x in lhs) - sum(x.sum() for x in rhs)) / mag
        in_ipm = (j[4] & 0xffff) > 0
        worst[in_ipm] = max(worst[in_ipm], err)
        count[in_ipm] += 1
        assert err <= (1e-6 if in_ipm else 1e-10), (i, in_ipm, err)
    assert count[False] + count[True] == B and (count[True] >= 3 if ipm else count[False] >= 3)
    print(f"N={N} ipm={ipm}: worst duality gap, set finishes {worst[False]:.3e}, interior point {worst[True]:.3e}")


@pytest.mark.parametrize("N", [20, 13])
def test_column_6_and_a_mass_direction_without_a_force_give_exact_zeros(model_jvp_emu, N):
    """Qd[6] weighs the constant 0: a unit direction in column 6 gives exact zeros, with and without a force; gravity and the thrust do not
    see the mass: a mass direction on a step that read no force gives exact zeros (use_fd off, and use_fd on with f NULL).  Column 15 is not
    read by the step."""
    from tests.emu import emu
    b = synth.make_batch(3, N=N, seed=synth.SEED0 + 40, **MIXED)
    rng = np.random.default_rng(600 + N)
    e = np.eye(16)
    for i in range(3):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, True)
        for use_fd, force, tm in ((True, f, e[[6, 15]]), (False, None, e[[6, 14, 15]]), (True, None, e[[14]])):
            cfg = emu.default_cfg(N=N, use_fd=use_fd)
            out = _mjvp(model_jvp_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], force, X, U, act, tm)
            assert out[3] == 0
            for v in out[6:]:
                assert v.shape[0] == tm.shape[0] and not v.any(), (i, use_fd, force is None)
        # ... and with a force the mass does move the step
        out = _mjvp(model_jvp_emu, emu.default_cfg(N=N, use_fd=True), b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, e[[14]])
        assert np.abs(out[7]).max() > 1e-9


@pytest.mark.parametrize("N", [20, 13])
def test_an_rd_direction_is_its_equivalent_ur_direction_with_a_weak_pin(step_emu, model_jvp_emu, N):
    """The input rows' data are dt Rd (u - ur): a direction r' of Rd puts + dt r'_i rho_u,k[i] there, a direction tur of ur puts
    - dt Rd_i tur_k[i], so r' and tur_k[i] = -(r'_i / Rd_i) (u+_k[i] - ur_k[i]) are ONE right-hand side on the free rows, and on the pinned
    rows both are to be 0.  At as_gamma on ndp_create's floor (1e8 x max dt Rd: the weakest pin a handle accepts) a pinned row that kept
    its dt r' rho would move the solution by about |dt r' rho| / as_gamma ~ 1e-9 .. 1e-8, while the two correct calls solve the same
    system with right-hand sides that differ by rounding: held to the dense comparison's 1e-10 of max(1, |z'|max).  (At the default
    as_gamma = 1e12 the same defect moves nothing above 1e-12: what zeroes a pinned row of dU there is the out-pass.)"""
    from tests.emu import emu
    B = 6
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N)
    cfg.as_gamma = 1e8 * cfg.dt * max(cfg.Rd)
    rd = np.array(list(cfg.Rd))
    rng = np.random.default_rng(650 + N)
    pinned, worst = 0, 0.0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        tm = np.zeros((1, 16))
        tm[0, 10:14] = rd * rng.uniform(0.5, 2.0, 4)
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], None, X, U, act)
        m = _mjvp(model_jvp_emu, *args, tm)
        if m[3] != 0 or m[4] & 0xffff:
            continue
        A = m[5].reshape(N, 4)
        pinned += int(A.any())
        tur = -(tm[0, 10:14] / rd) * (m[2].reshape(N, 4) - b["ur"][i])
        d = _jvp(step_emu, *args, tur=tur[None])
        s = max(F.scale(d[7]), F.scale(d[8]))
        err = max(np.max(np.abs(x - y)) for x, y in zip(m[6:], d[6:])) / s
        worst = max(worst, err)
        assert err <= 1e-10, (i, err)
        assert not m[8][0][A != 0].any()
    print(f"N={N}: Rd direction against its ur direction at as_gamma {cfg.as_gamma:.1e}, worst {worst:.3e}, {pinned} pinned instances")
    assert pinned >= 2


@pytest.mark.parametrize("N,use_fd", [(20, False), (13, True)])
def test_three_directions_in_one_call_are_three_calls_bit_for_bit(model_jvp_emu, N, use_fd):
    from tests.emu import emu
    B = 4
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd)
    rng = np.random.default_rng(700 + N)
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, use_fd)
        tm = _tmodel(rng, 3)
        tan = (rng.normal(size=(3, 10)), rng.normal(size=(3, N + 1, 10)), rng.normal(size=(3, N, 4)),
               rng.normal(size=(3, N + 1, 3)) if use_fd else None)
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        three = _mjvp(model_jvp_emu, *args, tm, *tan)
        assert three[3] == 0 and all(np.isfinite(v).all() for v in three[6:])
        for d in range(3):
            one = _mjvp(model_jvp_emu, *args, tm[d:d + 1], *(None if t is None else t[d:d + 1] for t in tan))
            for x, y in zip(three[6:], one[6:]):
                assert np.array_equal(x[d], y[0])


def test_a_zero_model_direction_equals_the_plain_forward_mode_as_numbers(step_emu, model_jvp_emu):
    """What include/ndp_nmpc.h states: with tmodel all zeros the outputs equal jvp_emu_step's on the same data tangents as numbers (the
    sign of a zero may differ: not asserted bit for bit)."""
    from tests.emu import emu
    N, B = 13, 4
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=True)
    rng = np.random.default_rng(8)
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, True)
        tan = (rng.normal(size=(2, 10)), rng.normal(size=(2, N + 1, 10)), rng.normal(size=(2, N, 4)), rng.normal(size=(2, N + 1, 3)))
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        m = _mjvp(model_jvp_emu, *args, np.zeros((2, 16)), *tan)
        p = _jvp(step_emu, *args, *tan)
        for x, y in zip(m, p):
            assert np.array_equal(x, y)


def test_emulated_nan_state_gives_nan_tangents(model_jvp_emu):
    from tests.emu import emu
    N = 20
    b = synth.make_batch(1, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg()
    x0 = b["x0"][0].copy()
    x0[3] = np.nan
    out = _mjvp(model_jvp_emu, cfg, x0, b["xr"][0], b["ur"][0], None, b["xr"][0], b["ur"][0], np.zeros(4 * N, dtype=np.int8), np.ones((3, 16)))
    assert out[3] != 0 and all(np.isnan(g).all() for g in out[6:])


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_edge_horizons_against_the_dense_reference(oracle, model_jvp_emu, N):
    """The horizons at which the out-passes change shape (tests/deriv_edges.py), B = 3 with a force, model and data directions together:
    set finishes within 1e-10 of max(1, |z'|max) of the reference."""
    from tests.emu import emu
    B = 3
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=True)
    ocfg = oracle.default_cfg(N=N, use_fd=True)
    rng = np.random.default_rng(800 + N)
    checked, worst = 0, 0.0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, True)
        tm = _tmodel(rng, 1)
        tan = (rng.normal(size=(1, 10)), rng.normal(size=(1, N + 1, 10)), rng.normal(size=(1, N, 4)), rng.normal(size=(1, N + 1, 3)))
        out = _mjvp(model_jvp_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, tm, *tan)
        assert out[3] == 0
        if out[4] & 0xffff:
            continue
        A = out[5].reshape(N, 4)
        r0, rX, rU = MR.model_jvp_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], _f64(f), X, U, A, tm[0], *(t[0] for t in tan))
        s = max(F.scale(rX), F.scale(rU))
        err = max(np.max(np.abs(out[6][0] - r0)), np.max(np.abs(out[7][0] - rX)), np.max(np.abs(out[8][0] - rU))) / s
        worst = max(worst, err)
        assert err <= 1e-10, (i, err)
        checked += 1
    print(f"N={N}: {checked} set finishes, worst distance {worst:.3e}")
    assert checked >= 1


# ---------------------------------------------------------------- the shipped code object and the interface
def test_mjvp_kernels_exist_and_use_no_scratch():
    """Both rti_mjvp_kernel instantiations (N = 20 and the run-time horizon) exist in the library's code object and keep their state in
    registers."""
    from ndp_nmpc_qd_amd import _lib, build, isa_inspect
    build.build()
    ks = isa_inspect.CodeObject(_lib.LIB_PATH).kernels()
    k = {n: v for n, v in ks.items() if "rti_mjvp_kernel" in n}
    assert len(k) == 2 and all(v["scratch"] == 0 for v in k.values()), k
    assert any("ILi20E" in n for n in k) and any("ILi0E" in n for n in k)


def test_header_declares_the_entries_and_the_binding_knows_them():
    from ndp_nmpc_qd_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "ndp_nmpc.h")) as fh:
        hdr = fh.read()
    for name, n_args in (("ndp_step_jvp_model_device", 20), ("ndp_closed_loop_jvp_model_device", 25)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", hdr)
        assert m and m.group(1).count(",") + 1 == n_args == len(getattr(lib, name).argtypes)
        assert name in _lib.EXPORTS
    m = re.search(r"#define\s+NDP_ABI_VERSION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 9 and lib.ndp_abi_version() == 9


def test_model_tangent_builds_the_columns():
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    q, r = torch.arange(10.0), torch.arange(4.0) + 20
    t = TL.model_tangent(tQd=q, tRd=r, tmass=0.5)
    assert t.shape == (16,) and t.dtype == torch.float64
    assert torch.equal(t[:10], q.double()) and torch.equal(t[10:14], r.double()) and t[14] == 0.5 and t[15] == 0.5
    t = TL.model_tangent(tmass=torch.ones(3))
    assert t.shape == (3, 16) and not t[:, :14].any() and bool((t[:, 14:] == 1).all())
    with pytest.raises(ValueError):
        TL.model_tangent()
    with pytest.raises(ValueError):
        TL.model_tangent(tQd=torch.zeros(2, 10), tRd=torch.zeros(4))
