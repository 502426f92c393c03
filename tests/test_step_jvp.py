"""The forward-mode derivative of the control step (RtiWave::jvp_out) without a GPU: the device's code on the host wave emulator against the
dense fixed-set reference (tests/fixed_set_ref.py), against the adjoint on the same tape (duality), T directions against T calls, failed steps,
pins, interior-point finishes, and the kernels' ISA.  The device side: tests/test_step_jvp_gpu.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.fixed_set_ref import NU, NX, jvp_ref, scale, vjp_ref
from tests.step_deriv_emu import MIXED, _jvp, _tape, _vjp, step_emu  # noqa: F401


def _tangents(rng, N, T, use_fd):
    return (rng.normal(size=(T, 10)), rng.normal(size=(T, N + 1, 10)), rng.normal(size=(T, N, 4)),
            rng.normal(size=(T, N + 1, 3)) if use_fd else None)


def _force(rng, N, use_fd):
    return rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32) if use_fd else None


def _f64(f):
    return None if f is None else f.astype(np.float64)


@pytest.mark.parametrize("N,B,use_fd", [(2, 4, False), (2, 3, True), (13, 4, True), (13, 3, False), (20, 6, False), (20, 3, True),
                                        (27, 3, True), (27, 2, False)])
def test_emulated_jvp_matches_the_dense_fixed_set_reference(oracle, step_emu, N, B, use_fd):
    """One random direction (tx0, txr, tur, tf) on the mixed workload (seed SEED0 + 40; inputs on their bounds among the instances): every
    set finish within 1e-10 of max(1, |z'|max) of jvp_ref at the step's final set; dX_0 = tx0 and du0 = dU_0 exactly, pinned rows of dU
    exactly 0; jvp_ref's two step sizes in the attitude reference agree to 1e-9."""
    from tests.emu import emu
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd)
    ocfg = oracle.default_cfg(N=N, use_fd=use_fd)
    rng = np.random.default_rng(100 + N)
    checked = pinned = 0
    worst = 0.0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, use_fd)
        tan = _tangents(rng, N, 1, use_fd)
        u0, Xn, Un, st, it, actn, du0, dX, dU = _jvp(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act, *tan)
        assert st == 0
        if it & 0xffff:                                  # interior point: test_interior_point_finishes_...
            continue
        A = actn.reshape(N, 4)
        pinned += int(A.any())
        r0, rX, rU, dz2 = jvp_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], _f64(f), X, U, A, *(None if t is None else t[0] for t in tan))
        s = max(scale(rX), scale(rU))
        assert np.max(np.abs(np.concatenate([rX.ravel(), rU.ravel()]) - dz2)) <= 1e-9 * s
        for got, r in zip((du0[0], dX[0], dU[0]), (r0, rX, rU)):
            worst = max(worst, np.max(np.abs(got - r)) / s)
            assert np.max(np.abs(got - r)) <= 1e-10 * s, (i, np.max(np.abs(got - r)) / s)
        assert np.array_equal(dX[0, 0], tan[0][0]) and np.array_equal(du0[0], dU[0, 0]) and not dU[0][A != 0].any()
        checked += 1
    print(f"N={N} use_fd={use_fd}: {checked} set finishes, {pinned} pinned, worst distance {worst:.3e}")
    assert checked >= 2


def test_the_mixed_workload_holds_free_and_pinned_finishes(step_emu):
    """What the dense comparison above rests on, at N = 20: the first instances of the mixed workload finish free AND pinned."""
    from tests.emu import emu
    N, B = 20, 12
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N)
    rng = np.random.default_rng(7)
    kinds = set()
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        out = _jvp(step_emu, cfg, b["x0"][i], b["xr"][i], b["ur"][i], None, X, U, act, tx0=np.ones((1, 10)))
        if out[3] == 0 and not out[4] & 0xffff:
            kinds.add(bool(out[5].any()))
            assert not out[8][0][out[5].reshape(N, 4) != 0].any()
    assert kinds == {False, True}


@pytest.mark.parametrize("N,use_fd,ipm", [(20, False, False), (13, True, False), (27, True, False), (20, False, True), (13, True, True)])
def test_duality_with_the_adjoint_on_the_same_tape(step_emu, N, use_fd, ipm):
    """<gz, JVP(t)> = <VJP(gz), t> for random gz = (gu0, gX, gU) and t = (tx0, txr, tur, tf) against vjp_emu_step: both are solves with one K.
    Bar: 1e-11 of the larger side's magnitude (the largest |term| of either inner product, at least 1), for set finishes and for
    interior-point ones alike (ipm: qp_mode 1, the velocity box +-3): there too both solve ONE system, the last Newton system's, with the
    same sweep.  Every instance is checked (status 0 throughout); with ipm at least 3 finish in the interior-point loop.
    Measured on the emulator: worst 1.4e-13 on set finishes (N = 27; 6.0e-14 at N = 20, 1.9e-14 at N = 13), 3.9e-14 on interior-point
    finishes (N = 20; 8.9e-15 at N = 13)."""
    from tests.emu import emu
    B = 6
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd, qp_mode=1 if ipm else 0)
    if ipm:
        for j in range(3):
            cfg.lbv[j], cfg.ubv[j] = -3.0, 3.0
    rng = np.random.default_rng(200 + N)
    worst = {False: 0.0, True: 0.0}
    count = {False: 0, True: 0}
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, use_fd)
        tan = _tangents(rng, N, 1, use_fd)
        gu0, gX, gU = rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4))
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        j = _jvp(step_emu, *args, *tan)
        a = _vjp(step_emu, *args, gu0, gX, gU)
        for x, y in zip(j[:6], a[:6]):                   # the recompute is the same step
            assert np.array_equal(x, y)
        assert j[3] == 0
        du0, dX, dU = (v[0] for v in j[6:])
        lhs = [gu0 * du0, gX * dX, gU * dU]
        rhs = [g * t[0] for g, t in zip(a[6:], tan) if t is not None]
        mag = max(1.0, max(np.abs(x).max() for x in lhs + rhs))
        err = abs(sum(x.sum() for x in lhs) - sum(x.sum() for x in rhs)) / mag
        in_ipm = (j[4] & 0xffff) > 0
        worst[in_ipm] = max(worst[in_ipm], err)
        count[in_ipm] += 1
        assert err <= 1e-11, (i, in_ipm, err)
    assert count[False] + count[True] == B and (count[True] >= 3 if ipm else count[False] >= 3)
    print(f"N={N} ipm={ipm}: worst duality gap, set finishes {worst[False]:.3e}, interior point {worst[True]:.3e}")


@pytest.mark.parametrize("N,use_fd", [(20, False), (13, True)])
def test_three_directions_in_one_call_are_three_calls_bit_for_bit(step_emu, N, use_fd):
    from tests.emu import emu
    B = 4
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd)
    rng = np.random.default_rng(300 + N)
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, use_fd)
        tan = _tangents(rng, N, 3, use_fd)
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        three = _jvp(step_emu, *args, *tan)
        assert three[3] == 0 and all(np.isfinite(v).all() for v in three[6:])
        for d in range(3):
            one = _jvp(step_emu, *args, *(None if t is None else t[d:d + 1] for t in tan))
            for x, y in zip(three[6:], one[6:]):
                assert np.array_equal(x[d], y[0])


def test_null_tangents_are_zero_and_null_outputs_are_left_alone(step_emu):
    """tx0 alone equals the full call with the other tangents 0, bit for bit; an output that is not asked for is not written."""
    from tests.emu import emu
    N = 13
    b = synth.make_batch(1, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=True)
    rng = np.random.default_rng(9)
    X, U, act = _tape(b, 0, rng, N)
    tx0 = rng.normal(size=(2, 10))
    args = (cfg, b["x0"][0], b["xr"][0], b["ur"][0], _force(rng, N, True), X, U, act)
    a = _jvp(step_emu, *args, tx0=tx0)
    c = _jvp(step_emu, *args, tx0, np.zeros((2, N + 1, 10)), np.zeros((2, N, 4)), np.zeros((2, N + 1, 3)))
    for x, y in zip(a[6:], c[6:]):
        assert np.array_equal(x, y)


def test_emulated_nan_state_gives_nan_tangents(step_emu):
    from tests.emu import emu
    N = 20
    b = synth.make_batch(1, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg()
    x0 = b["x0"][0].copy()
    x0[3] = np.nan
    out = _jvp(step_emu, cfg, x0, b["xr"][0], b["ur"][0], None, b["xr"][0], b["ur"][0], np.zeros(4 * N, dtype=np.int8), tx0=np.ones((3, 10)))
    assert out[3] != 0 and all(np.isnan(g).all() for g in out[6:])


@pytest.mark.parametrize("N,use_fd", [(20, False), (13, True)])
def test_interior_point_finishes_are_as_close_to_the_pinned_reference_as_the_adjoint(oracle, step_emu, N, use_fd):
    """qp_mode 1 with the velocity box shrunk to +-3 (the adjoint's interior-point instances, tests/test_step_vjp.py: seed SEED0 + 70 + N):
    the last Newton system is barrier-smoothed, so the reference pins the bounds that are active at the solution (within 1e-6), and the
    tangent's distance from jvp_ref (of max(1, |z'|max)) is held to 2 x the distance of the adjoint's outputs from vjp_ref on the same
    instances with the same pins (of max(1, |g|max)): the system is barrier-smoothed in both.
    The bar compares the worst values over the instances, as the model gradient's test of the same kind does; per instance the ratio varies.
    Measured on the emulator, worst over the instances: N = 20 tangent 1.3e-3 against adjoint 2.7e-3 (4 instances); N = 13 tangent 1.5e-4
    against adjoint 1.7e-4 (6 instances).  Largest single-instance ratio tangent / adjoint: 3.7 (N = 20, instance 3: 1.2e-4 against 3.2e-5)."""
    from tests.emu import emu
    B = 6
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 70 + N, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=use_fd, qp_mode=1)
    ocfg = oracle.default_cfg(N=N, use_fd=use_fd)
    for j in range(3):
        cfg.lbv[j], cfg.ubv[j] = -3.0, 3.0
        ocfg.lbv[j], ocfg.ubv[j] = -3.0, 3.0
    rng = np.random.default_rng(5)
    n_ipm = 0
    worst_j = worst_a = 0.0
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = _force(rng, N, use_fd)
        gu0, gX, gU = rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4))
        tan = _tangents(rng, N, 1, use_fd)
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        j = _jvp(step_emu, *args, *tan)
        if j[3] != 0 or not (j[4] & 0xffff):
            continue
        n_ipm += 1
        a = _vjp(step_emu, *args, gu0, gX, gU)
        Xn, Un = j[1].reshape(N + 1, NX), j[2].reshape(N, NU)
        qp = oracle.linearize(ocfg, b["x0"][i], b["xr"][i], b["ur"][i], _f64(f) if use_fd else None, X, U)
        lbu, ubu, lbv, ubv = (np.array(list(v)) for v in (cfg.lbu, cfg.ubu, cfg.lbv, cfg.ubv))
        pins = []
        for k in range(N):
            for c in range(NU):
                if abs(Un[k, c] - ubu[c]) < 1e-6 or abs(Un[k, c] - lbu[c]) < 1e-6:
                    pins.append(((N + 1) * NX + NU * k + c, float(qp["uu"][k, c] if abs(Un[k, c] - ubu[c]) < 1e-6 else qp["lu"][k, c])))
        for k in range(1, N + 1):
            for c in range(3):
                if abs(Xn[k, 3 + c] - ubv[c]) < 1e-6 or abs(Xn[k, 3 + c] - lbv[c]) < 1e-6:
                    pins.append((k * NX + 3 + c, float(qp["uv"][k, c] if abs(Xn[k, 3 + c] - ubv[c]) < 1e-6 else qp["lv"][k, c])))
        ref = (b["x0"][i], b["xr"][i], b["ur"][i], _f64(f), X, U, None)
        _, rX, rU, _ = jvp_ref(oracle, ocfg, *ref, *(None if t is None else t[0] for t in tan), pin_v=pins)
        # (the reference's pinned inputs are exactly 0; the interior point holds none exactly: compared as they are)
        dj = max(np.max(np.abs(j[7][0] - rX)), np.max(np.abs(j[8][0] - rU))) / max(scale(rX), scale(rU))
        g = vjp_ref(oracle, ocfg, *ref, gu0, gX, gU, pin_v=pins)
        da = max(np.max(np.abs(x - y)) for x, y in zip(a[6:], g)) / max(scale(y) for y in g)
        print(f"N={N} i={i} pins={len(pins)} tangent distance {dj:.3e}  adjoint distance {da:.3e}")
        worst_j, worst_a = max(worst_j, dj), max(worst_a, da)
    print(f"N={N}: worst tangent distance {worst_j:.3e}, worst adjoint distance {worst_a:.3e}")
    assert n_ipm >= 3
    assert worst_j <= 2.0 * worst_a, (worst_j, worst_a)


def test_jvp_kernels_use_no_scratch_and_leave_the_adjoint_kernels_alone():
    """Both rti_jvp_kernel instantiations (N = 20 and the run-time horizon) exist in the library's one code object and keep their state in
    registers; rti_vjp_kernel and rti_wvjp_kernel still have exactly their two each."""
    from ndp_nmpc_qd_amd import _lib, build, isa_inspect
    build.build()
    ks = isa_inspect.CodeObject(_lib.LIB_PATH).kernels()
    k = {n: v for n, v in ks.items() if "rti_jvp_kernel" in n}
    assert len(k) == 2 and all(v["scratch"] == 0 for v in k.values()), k
    assert len([n for n in ks if "rti_vjp_kernel" in n]) == 2 and len([n for n in ks if "rti_wvjp_kernel" in n]) == 2


def test_header_declares_the_entry_and_the_abi_stays():
    import ctypes as C
    import os
    import re
    from ndp_nmpc_qd_amd import _lib, build
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndp_nmpc.h")).read()
    assert re.search(r"\bint\s+ndp_step_jvp_device\s*\(", hdr)
    m = re.search(r"#define\s+NDP_ABI_VERSION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 9
    build.build()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "ndp_step_jvp_device")
