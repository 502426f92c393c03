"""The plant side and the closed loop on the device at models other than the reference's constants (run with -m gpu).

tests/test_model_envelope_gpu.py holds the control step, its derivatives, the tick and the forward plant step at other models; everything
on the plant side that differentiates, the force on the plant, the K-neighbour prediction, the formation rollouts and the one-call
closed loop ran at mass 1.4844, g 9.81 and r_horiz 1 only.  Here the handles are created at (or moved by ndp_set_model to) the models
and radii of tests/plant_side_cases.py and held to references built at the same model by code that shares nothing with the device.  A
kernel that compared a gate distance against 1.0, a 1 / mass that stayed stale in one of its readers or a folded g would pass every
other module and fail here: tests/test_plant_side_envelope.py asserts, on the CPU, that the reference at the default model or radius
lies at least 100 bars from each of these comparisons' references, and checks the conditions the inputs must meet.

Groups, bars (none from what the device gives) and their sources:
  a  plant rollout, VJP, JVP at light_lowg (mass 0.6, g 7.0) and m09 (mass 0.9): B = 65, 3 ticks, substeps 1 and 4, with a force.
     1e-13 of max(1, the row's largest reference entry), no row left out (plant_deriv_ref.within_bar); forward rows bit-equal to
     successive ndp_plant_step_device calls; set_model(mass) on a live handle = a handle created with that mass, bit for bit.
  b  plant_force[_multi] and their VJP / JVP at r_horiz 0.75 and 1.5, (B, K) = (7, 3) and (64, 3), gate on: BAR = 1e-5
     (tests/test_plant_force_deriv_gpu.py) against plant_force_deriv_ref at that radius; bit-equal to the prediction's derivatives on
     packed windows; the rim at 0.75; every pair between 0.75 and 1.0 apart: exact zeros at 0.75, the gate-off bits at 1.5.
  c  downwash_multi and its VJP / JVP on windows at r_horiz 0.75, (B, K) = (64, 3): BAR = 1e-5 (tests/test_downwash_multi_deriv_gpu.py),
     and the rim per slot.
  d  both formation rollouts at mass 0.9, g 7.0, r_horiz 0.75, 2 pairs / 2 triples, 12 ticks, the offset workload, compensate on and
     off: bit-equal to the host composition; positions within POS_BAR = 2.17e-6 m (tests/test_formation_rollout_gpu.py) of the CPU loop
     at that cfg and radius; every status 0.
  e  the one-call closed loop and its reverse at LOOP_CASE (distinct weights, mass 0.9, the asymmetric box, g 7.0), B = 65, K = 3,
     N = 20 and 7: values, status words, tape slots and the engine's state bit-equal to the plain loop; every leaf gradient within
     BAR["ext"] = 1.24e-11 (tests/test_closed_loop_chain_gpu.py) of closed_loop_chain_ref.reverse on the device's record; the model
     gradient within STEP_BAR = 1e-9 max(1, |g|max) per tick (columns 0..14) and BAR["ext"] max(1, |gfp|max) sum_k |fp_k|_1 / m with
     this model's m (column 15) (tests/test_closed_loop_vjp_gpu.py); device central differences through set_model in Qd[0], Rd[3] and
     the mass (column 14 + column 15) within FD_BAR = 1e-6 on the vehicles whose sets and iteration words do not move, at least 40 of
     65; set_model(Qd, Rd, mass) before the warm-up step = the created handle, every output of both calls; one run with dt = 0.05,
     substeps = 3 (K = 2).
  f  the one call at N = 2, 27, 28, 40, default model, B = 65, K = 2, with and without a tape: bit-equal to the plain loop, guard rows
     intact; at N = 28 the reverse call returns -2, names itself and the N <= 27 rule, and touches nothing.
The float64 references' own checks at these models (tests/test_plant_side_envelope.py: the sweep against the oracle's differences
6.8e-9, the model gradient 9.7e-10, both of FD_BAR = 1e-6) do not resolve a tenth of the 1e-13 and 1e-11 bars any more than they do at
the default model; the bars are the project's, unchanged.

Measured on the first device run (MI355X), the worst of each group (DESIGN.md section 9 has the same):
  a  xs 3.7e-16, gx0 1.7e-15, gu 5.6e-17, gf 1.1e-16, dxs 1.2e-15 of the row's scale (bar 1e-13)
  b  g_w 9.2e-7, g_z 1.8e-6, df 1.2e-6, f 1.9e-6 (bar 1e-5); 7 / 16 of 21 and 65 / 163 of 192 slots open at 0.75 / 1.5
  c  g_w 3.7e-7, g_z 2.9e-6, df 3.3e-6 (bar 1e-5); 65 of 192 slots open, 15 slots in another state than at r = 1
  d  positions 1.3e-13 m (pairs) and 6.9e-14 m (triples) from the CPU loop (bar 2.17e-6 m), u0 8.7e-12
  e  all 65 vehicles set finishes at both horizons, 63 (N = 20) and 56 (N = 7) of them with an input on the asymmetric box; against the
     oracle's loop u0 6.7e-15; leaves N = 20: x0 1.13e-11, xr 2.2e-12, ur 1.7e-12, f 4.7e-12, fp 1.6e-12; N = 7: x0 6.3e-13, xr 4.6e-13,
     ur 3.0e-13, f 4.1e-13, fp 2.7e-15; dt 0.05 / 3 substeps: x0 7.0e-12, xr 2.3e-12, ur 1.7e-12, f 4.5e-12, fp 1.7e-12 (bar 1.24e-11);
     model gradient 1.0e-3 / 8.9e-5 (columns 0..14) and 1.7e-2 / 5.1e-5 (column 15) of its bars at N = 20 / 7; device differences Qd[0]
     3.3e-11, Rd[3] 2.7e-10, mass 1.8e-9 (bar 1e-6), 65 of 65 stable.
     The x0 figure at N = 20 is 91 % of its bar and fifty times the default model's 2.2e-13.  It is one vehicle, number 0 (the other five:
     5.9e-15 .. 9.8e-13), the one whose three KKT systems have condition 3.7e6 .. 4.8e6 (the others 6.8e5 .. 1.2e6) and for which the
     float64 reference's forward and reverse sweeps disagree with each other by 9.5e-12 (the others 3.8e-13 .. 1.7e-12): the figure is
     as much the reference's rounding as the device's.  The bar is the chain's, unchanged (see the note where it is asserted).
  f  bit-equal at all four horizons, with and without a tape."""
import ctypes as C_

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import closed_loop_chain_ref as R
from tests import formation_ref as FR
from tests import model_cases as MC
from tests import plant_deriv_ref as P
from tests import plant_force_deriv_ref as PF
from tests import plant_side_cases as C
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.test_closed_loop_chain_gpu import BAR as CHAIN_BAR, FD_BAR, STEP_BAR, VALUE_ATOL
from tests.test_closed_loop_vjp_gpu import OUTS, _engine, _forward, _loop, _np, _reverse, _state
from tests.test_downwash_multi_deriv_gpu import BAR as MULTI_BAR, _multi_forward, _multi_jvp, _multi_vjp
from tests.test_formation_multi_rollout_gpu import _device_rollout as _multi_rollout, _host_composition as _multi_composition
from tests.test_formation_rollout_gpu import POS_BAR, _device_rollout, _host_composition
from tests.test_plant_force_deriv_gpu import BAR as FORCE_BAR, _directions, _force, _jvp as _force_jvp, _mixed_case, _vjp as _force_vjp
from tests.test_plant_rollout_gpu import dev, forward, host, jvp, run, vjp

pytestmark = pytest.mark.gpu

LEAF_BAR = CHAIN_BAR["ext"]
assert (FORCE_BAR, MULTI_BAR, FD_BAR, STEP_BAR) == (1e-5, 1e-5, 1e-6, 1e-9) and abs(POS_BAR - 2.17e-6) < 1e-12 and abs(LEAF_BAR - 1.24e-11) < 1e-17


@pytest.fixture(scope="module")
def blob():
    return _lib.load_weights()


@pytest.fixture(scope="module")
def engines(ndp):
    """Engines shared per module, keyed by their arguments."""
    made = {}

    def get(batch, **kw):
        key = (batch, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))
        if key not in made:
            made[key] = ndp.BatchedNMPC(batch, **kw)
        return made[key]
    yield get
    for e in made.values():
        e.close()


# ================================================================ a. the plant's rollout and its derivatives
def _plant_engine(engines, name):
    eng = engines(C.B, load_mlp=False, **MC.engine_kw(MC.PLANT_CASES[name]))
    mass, g = MC.model_of(MC.PLANT_CASES[name])[2:4]
    assert (eng.cfg.mass, eng.cfg.gravity) == (mass, g)
    return eng


def _plant_calls(eng, r, sub):
    """(xs, gx0, gu, gf, dxs) of the three calls on a case's inputs, as numpy."""
    x0, u, f = dev(r["x0"]), dev(r["u"]), dev(r["f"])
    xs = forward(eng, x0, u, f, sub)
    got = vjp(eng, x0, u, f, xs, dev(r["gxs"]), sub)
    dxs, _ = jvp(eng, x0, u, f, sub, dev(r["tx0"]), dev(r["tu"]), dev(r["tf"]))
    return [host(t) for t in (xs, *got, dxs)]


@pytest.mark.parametrize("sub", C.PLANT_SUBSTEPS)
@pytest.mark.parametrize("name", sorted(MC.PLANT_CASES))
def test_plant_rollout_and_its_derivatives_follow_the_model(engines, name, sub):
    """Forward rows bit-equal to successive ndp_plant_step_device calls on the same handle and within the plant bar of the float64
    rollout at the case's mass and g; gx0, gu, gf and dxs (T = 4) within the plant bar of the complex-step Jacobian at that model."""
    eng, r = _plant_engine(engines, name), C.plant_reference(name, sub)
    xs, gx0, gu, gf, dxs = _plant_calls(eng, r, sub)
    x, du, df = dev(r["x0"]), dev(r["u"]), dev(r["f"])
    for k in range(C.PLANT_TICKS):
        run(eng, lambda: eng._check(eng._lib.ndp_plant_step_device(eng._h, C_.c_void_p(x.data_ptr()), C_.c_void_p(du[k].data_ptr()),
                                                                   C_.c_void_p(df[k].data_ptr()), C.DT, sub, None), "ndp_plant_step_device"))
        assert np.array_equal(xs[k], host(x)), k
    figures = {"xs": P.within_bar(xs, P.rollout(r["x0"], r["u"], r["f"], C.DT, sub, r["mass"], r["g"]))}
    for n, dv, rf in zip(("gx0", "gu", "gf"), (gx0, gu, gf), P.vjp(r["J"], r["gxs"])):
        figures[n] = P.within_bar(dv, rf)
    figures["dxs"] = P.within_bar(dxs, P.jvp(r["J"], r["tx0"], r["tu"], r["tf"]))
    print(f"{name} substeps {sub}: worst |dev - ref| / max(1, row max): " + " ".join(f"{n} {v[1]:.2e}" for n, v in figures.items()))
    for n, (ok, ratio) in figures.items():
        assert ok, (n, ratio)


@pytest.mark.parametrize("name", sorted(MC.PLANT_CASES))
def test_set_model_mass_gives_the_created_handles_bits_in_all_three_plant_calls(ndp, engines, name):
    """A handle created with the DEFAULT mass (and the case's g: set_model has no g) after set_model(mass=...) against the handle created
    with that mass: the rollout, its VJP and its JVP, bit for bit."""
    case = MC.PLANT_CASES[name]
    r = C.plant_reference(name, 4)
    live = ndp.BatchedNMPC(C.B, load_mlp=False, **MC.engine_kw({k: v for k, v in case.items() if k != "mass"}))
    assert live.cfg.mass == MC.MASS0
    before = _plant_calls(live, r, 4)
    live.set_model(mass=case["mass"])
    moved = _plant_calls(live, r, 4)
    live.close()
    made = _plant_calls(_plant_engine(engines, name), r, 4)
    for n, a, b, c in zip(("xs", "gx0", "gu", "gf", "dxs"), moved, made, before):
        assert np.array_equal(a, b), n
        if n in ("xs", "gf", "dxs"):
            assert not np.array_equal(a, c), n                                   # (the mass does reach these three)


# ================================================================ b. the force on the plant
def _force_engine(engines, Bf, r):
    eng = engines(Bf, N=20, disturbance=True, r_horiz=r)
    assert eng.cfg.r_horiz == r
    return eng


@pytest.mark.parametrize("r", MC.RADII)
@pytest.mark.parametrize("Bf,K", C.FORCE_SHAPES)
def test_plant_force_derivatives_against_the_float64_reference_at_the_radius(engines, blob, Bf, K, r):
    """g_w (every parameter group), g_z per slot, df (T = 2) and the force, gate on, on shared-state inputs redrawn at THIS radius."""
    c = C.force_case(blob, Bf, K, r)
    ref = C.force_reference(blob, c, r)
    x, idx = c["x"], c["index"]
    eng = _force_engine(engines, Bf, r)
    gz, gw = _force_vjp(eng, x, idx, ref["gf"])
    df, fc = _force_jvp(eng, x, idx, ref["tx"], ref["tw"], 2)
    assert ref["margin"][idx >= 0].min() >= PF.R.MARGIN and ref["open"].any() and ((idx >= 0) & ~ref["open"]).any()
    e = C.force_errors(gz, gw, df, fc, ref)
    print(f"B = {Bf} K = {K} r = {r}: {int(ref['open'].sum())} of {Bf * K} slots open; " + " ".join(f"{n} {v:.3e}" for n, v in e.items()))
    assert np.array_equal(fc, _force(eng, x, idx)) and not gz[~ref["open"]].any()
    assert max(e.values()) <= FORCE_BAR, e


@pytest.mark.parametrize("r", MC.RADII)
@pytest.mark.parametrize("Bf,K", C.FORCE_SHAPES)
def test_plant_force_derivatives_are_the_predictions_on_packed_windows_at_the_radius(engines, blob, Bf, K, r):
    """tests/test_plant_force_deriv_gpu.py's first test on an engine at r_horiz = r: windows other[o][node] = x[o], ego_ref[v][node] = x[v],
    ego_xy = x[v][0:2]; d_gz is node 0 of ndp_downwash_multi_vjp_device's, d_df node 0 of ndp_downwash_multi_jvp_device's, d_f_check
    ndp_plant_force_multi_device's force -- all bit for bit, and the gates are those of the radius."""
    import torch
    n, gate, scale, T = 20, True, 0.7, 2
    eng = _force_engine(engines, Bf, r)
    x, idx = _mixed_case(10 * Bf + K, Bf, K)
    has = (idx >= 0) & (idx < Bf)
    if not (has & ~PF.gather(x, idx, gate, r * r)[1]).any():                    # 7 vehicles within +-0.75 m: no pair 1.5 m apart, so one
        v, k = next((v, k) for v in range(Bf) for k in range(K) if has[v, k] and idx[v, k] != v)      # neighbour is moved 2 m away
        x[idx[v, k], 0] = x[v, 0] + 2.0
    op, op1 = PF.gather(x, idx, gate, r * r)[1], PF.gather(x, idx, gate)[1]
    assert op.any() and (has & ~op).any() and (op != op1).any()
    gf = np.random.default_rng(Bf * K).normal(size=(Bf, 3))
    gz, gw = _force_vjp(eng, x, idx, gf, gate, scale)
    assert not gz[~op].any() and np.abs(gz[op]).max(axis=1).min() > 0 and np.isfinite(gw).all() and np.abs(gw).max() > 0
    win = _t(np.ascontiguousarray(np.broadcast_to(x[:, None], (Bf, n + 1, 10))))
    idw, exy = _t(np.where(has, idx, -1).astype(np.int32)), _t(x[:, :2])
    up = np.zeros((Bf, n + 1, 3))
    up[:, 0] = scale * gf
    wz = torch.full((Bf, K, n + 1, 6), -7.0, dtype=torch.float64, device=_dev())
    eng.downwash_multi_vjp_device(win, idw, win, _t(up), ego_xy=exy, gz=wz)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(gz, wz.cpu().numpy()[:, :, 0])
    tx, tw = _directions(7 + Bf + K, blob, Bf, T)
    df, fc = _force_jvp(eng, x, idx, tx, tw, T, gate, 1.0)
    tz = np.zeros((Bf, T, K, n + 1, 6))
    o = np.where(has, idx, np.arange(Bf)[:, None])
    tz[:, :, :, 0] = (tx[o][..., :6] - tx[:, None, :, :6]).transpose(0, 2, 1, 3)
    wd = torch.full((Bf, T, n + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    eng.downwash_multi_jvp_device(win, idw, win, tz=_t(tz), tw=_t(tw), ego_xy=exy, n_tan=T, df=wd)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(df, wd.cpu().numpy()[:, :, 0]) and not df[~op.any(axis=1)].any()
    assert np.array_equal(fc, _force(eng, x, idx, gate, 1.0)) and not fc[~op.any(axis=1)].any()
    assert np.abs(fc[op.any(axis=1)]).max(axis=1).min() > 0
    if K == 3 and Bf == 7:                                                       # single against multi at this radius
        one = idx[:, :1].copy()
        sz, sw = _force_vjp(eng, x, one, gf, gate, scale, single=True)
        mz, mw = _force_vjp(eng, x, one, gf, gate, scale)
        sd, sf = _force_jvp(eng, x, one, tx, tw, T, gate, scale, single=True)
        md, mf = _force_jvp(eng, x, one, tx, tw, T, gate, scale)
        assert np.array_equal(sz, mz) and np.array_equal(sw, mw) and np.array_equal(sd, md) and np.array_equal(sf, mf)
        assert np.array_equal(eng.plant_force(x, one[:, 0], gate=True, scale=scale), sf)


def test_plant_force_gate_is_strict_at_the_rim_of_the_radius(engines, blob):
    """r_horiz = 0.75, whose square is exact: distance^2 == r^2 exactly is closed, one ulp inside is open -- in the force, its single
    and multi forms, the adjoint (an exactly zero g_z) and forward mode; gate off: open everywhere."""
    Bf, r = 6, 0.75
    eng = _force_engine(engines, Bf, r)
    x = PF.draw_states(np.random.default_rng(5), Bf)
    x[0, 0:3], x[1, 0:3] = (0.25, -0.5, 1.0), (0.25 + r, -0.5, 1.5)                       # on the rim: dx = r exactly, dy = 0
    x[2, 0:3], x[3, 0:3] = (0.25, 0.5, 1.0), (np.nextafter(0.25 + r, 0.0), 0.5, 1.5)      # one ulp inside
    x[4, 0:3], x[5, 0:3] = (-0.5, 0.0, 1.0), (-0.5, 0.25, 1.5)                            # well inside
    assert (x[1, 0] - x[0, 0]) ** 2 == r * r and (x[3, 0] - x[2, 0]) ** 2 < r * r
    idx = (np.arange(Bf, dtype=np.int32) ^ 1)[:, None]
    f = eng.plant_force(x, idx[:, 0], gate=True)
    assert np.array_equal(f[0:2], np.zeros((2, 3))) and np.all(np.any(f[2:] != 0.0, axis=1))
    assert np.array_equal(eng.plant_force_multi(x, idx, gate=True), f) and np.array_equal(_force(eng, x, idx), f)
    f_open = eng.plant_force(x, idx[:, 0], gate=False)
    assert np.all(np.any(f_open != 0.0, axis=1)) and np.array_equal(f_open[2:], f[2:])
    gf = np.random.default_rng(6).normal(size=(Bf, 3))
    tx, tw = _directions(8, blob, Bf, 2)
    for single in (False, True):
        gz, gw = _force_vjp(eng, x, idx, gf, single=single)
        gz_open, _ = _force_vjp(eng, x, idx, gf, gate=False, single=single)
        df, fc = _force_jvp(eng, x, idx, tx, tw, 2, single=single)
        df_open, _ = _force_jvp(eng, x, idx, tx, tw, 2, gate=False, single=single)
        assert not gz[0:2].any() and not df[0:2].any() and np.array_equal(fc, f)
        assert np.array_equal(gz[2:], gz_open[2:]) and np.array_equal(df[2:], df_open[2:])
        assert np.abs(gz_open[:, 0]).max(axis=1).min() > 0 and np.abs(df_open).max(axis=(1, 2)).min() > 0
        # the two closed slots carry nothing into the weights: the same call without them
        without = idx.copy()
        without[0:2] = -1
        assert np.array_equal(gw, _force_vjp(eng, x, without, gf, single=single)[1])


def test_pairs_between_the_radii_are_closed_at_the_small_one_and_open_at_the_large_one(engines, blob):
    """Every (vehicle, neighbour) pair 0.75 .. 1.0 apart: exact zeros in every output at r_horiz = 0.75; at 1.5 the gate-off call's bits --
    and those are not the bits of the gate at 1.0 on the same states only because there every slot is open too: the engine at the
    default radius is asked as well, and must agree with 1.5 and differ from 0.75."""
    Bf, K = 7, 3
    x, idx = C.ring_case(3, Bf, K)
    gf = np.random.default_rng(1).normal(size=(Bf, 3))
    tx, tw = _directions(2, blob, Bf, 2)
    small, large, unit = (_force_engine(engines, Bf, r) for r in (0.75, 1.5, 1.0))
    gz, gw = _force_vjp(small, x, idx, gf)
    df, fc = _force_jvp(small, x, idx, tx, tw, 2)
    assert not gz.any() and not gw.any() and not df.any() and not fc.any() and not _force(small, x, idx).any()
    off = _force_vjp(large, x, idx, gf, gate=False) + _force_jvp(large, x, idx, tx, tw, 2, gate=False)
    for eng in (large, unit):
        on = _force_vjp(eng, x, idx, gf) + _force_jvp(eng, x, idx, tx, tw, 2)
        for a, b in zip(on, off):
            assert np.array_equal(a, b) and np.abs(a).max() > 0


# ================================================================ c. the K-neighbour prediction on windows
def test_window_prediction_derivatives_against_the_float64_reference_at_the_radius(engines, blob):
    """downwash_multi, its VJP and its JVP at r_horiz = 0.75 on own-row inputs whose gates were drawn around 0.75 (closed slots between
    0.825 and 2.25 away, a share of them inside 1.0)."""
    c = C.multi_case(blob)
    Bm, K = C.MULTI_SHAPE
    ref = C.multi_reference(blob, c, C.MULTI_R)
    eng = engines(Bm, N=C.MULTI_N, disturbance=True, r_horiz=C.MULTI_R)
    gz, gw = _multi_vjp(eng, c, ref["gf"])
    df, fc = _multi_jvp(eng, c, ref["tz"], ref["tw"], 2)
    op = ref["open"]
    assert ref["margin"].min() >= PF.R.MARGIN and np.array_equal(op, c["open"]) and (op != (c["d2"] < 1.0)).sum() >= 10
    e = C.multi_errors(gz, gw, df, ref)
    print(f"B = {Bm} K = {K} r = {C.MULTI_R}: {int(op.sum())} of {Bm * K} slots open, {int((op != (c['d2'] < 1.0)).sum())} of them another "
          f"state than at r = 1; " + " ".join(f"{n} {v:.3e}" for n, v in e.items()))
    assert not gz[~op].any() and np.abs(gz[op]).max(axis=(1, 2)).min() > 0
    assert np.array_equal(fc, _multi_forward(eng, c)) and not fc[~op.any(axis=1)].any()
    assert max(e.values()) <= MULTI_BAR, e


def test_window_prediction_gate_is_strict_at_the_rim_of_the_radius_per_slot(engines, blob):
    """tests/test_downwash_multi_gpu.py's rim construction at r = 0.75 on the derivatives: row 0 of `other` sits exactly on the rim of
    every instance's ego_xy, row 1 one ulp inside.  The gated calls give the bits of the UNGATED calls in which the rim slots are
    empty: g_z of a rim slot is exactly 0, and it adds nothing to g_w, df or the force."""
    Bm, K, N, r = 4, 2, C.MULTI_N, 0.75
    eng = engines(Bm, N=N, disturbance=True, r_horiz=r)
    rng = np.random.default_rng(3)
    xr, other = rng.normal(0.0, 0.7, (Bm, N + 1, 10)), rng.normal(0.0, 0.7, (2, N + 1, 10))
    ego_xy = np.tile(np.array([0.25, -0.5]), (Bm, 1))
    other[0, 0, 0:2] = (0.25 + r, -0.5)
    other[1, 0, 0:2] = (np.nextafter(0.25 + r, 0.0), -0.5)
    assert (other[0, 0, 0] - 0.25) ** 2 == r * r and (other[1, 0, 0] - 0.25) ** 2 < r * r
    idx = np.array([[0, 1], [1, 0], [0, 0], [1, 1]], np.int32)
    gated = dict(other=other, index=idx, xr=xr, ego_xy=ego_xy)
    plain = dict(other=other, index=np.where(idx == 0, -1, idx).astype(np.int32), xr=xr, ego_xy=None)
    gf = rng.normal(size=(Bm, N + 1, 3))
    tz = rng.normal(size=(Bm, 2, K, N + 1, 6))
    tw = (np.asarray(blob, dtype=np.float64)[None] * 0.1 * rng.normal(size=(2, mlp_frag.NPARAM))).astype(np.float32)
    a = _multi_vjp(eng, gated, gf) + _multi_jvp(eng, gated, tz, tw, 2)
    b = _multi_vjp(eng, plain, gf) + _multi_jvp(eng, plain, tz, tw, 2)
    for s, t in zip(a, b):
        assert np.array_equal(s, t)
    gz = a[0]
    assert not gz[idx == 0].any() and np.abs(gz[idx == 1]).max(axis=(1, 2)).min() > 0 and not a[2][2].any() and not a[3][2].any()


# ================================================================ d. the formation rollouts
@pytest.mark.parametrize("compensate", [True, False])
@pytest.mark.parametrize("multi", [False, True])
def test_formation_rollouts_follow_the_model_and_the_radius(ndp, oracle, blob, multi, compensate):
    """2 pairs (multi: 2 triples), 12 ticks of the offset workload at mass 0.9, g 7.0, r_horiz 0.75: log, log_u, log_f and the worst
    status bit-equal to the host composition on a second handle; positions within POS_BAR of the CPU loop at that cfg and radius;
    every status 0; and the force log exactly 0 -- every neighbour flies between 0.75 and 1.0 away, where the default radius hears
    newtons (tests/test_plant_side_envelope.py)."""
    cfg = C.form_cfg(oracle)
    tr, x0, (cpu_states, cpu_u, _, cpu_st) = C.form_reference(blob, cfg, MC.radius_of(C.FORM_CASE), multi, compensate)
    Bv, idx = x0.shape[0], tr["other_index"]
    engs = [ndp.BatchedNMPC(Bv, disturbance=compensate, load_mlp=True, **MC.engine_kw(C.FORM_CASE)) for _ in range(2)]
    for e in engs:
        FR.set_trajectory(e, tr)
        assert (e.cfg.mass, e.cfg.gravity, e.cfg.r_horiz) == (0.9, 7.0, 0.75)
    if multi:
        states, u0s, fs, sts = _multi_composition(engs[0], idx, idx if compensate else None, x0, C.FORM_TICKS, 0.0, 1.0)
        x_end, log, log_u, log_f, worst = _multi_rollout(engs[1], x0, idx, C.FORM_TICKS)
    else:
        states, u0s, fs, sts = _host_composition(engs[0], tr, x0, C.FORM_TICKS, 0.0, compensate, 1.0)
        x_end, log, log_u, log_f, worst = _device_rollout(engs[1], x0, idx, C.FORM_TICKS)
    for e in engs:
        e.close()
    assert np.array_equal(log_f, fs) and np.array_equal(log_u, u0s)
    assert np.array_equal(log, states) and np.array_equal(x_end, states[-1]) and np.array_equal(worst, sts.max(axis=0))
    dpos, du = float(np.abs(log[:, :, 0:3] - cpu_states[:, :, 0:3]).max()), float(np.abs(log_u - cpu_u).max())
    print(f"multi {multi} compensate {compensate}: max |position - CPU loop| {dpos:.3e} m (bar {POS_BAR:.2e}), max |u0 - CPU loop| {du:.3e}")
    assert not worst.any() and not cpu_st.any() and not log_f.any()
    assert dpos <= POS_BAR, dpos


# ================================================================ e. the one-call closed loop and its reverse
def _assert_values(v, rec, eng, t, after_fwd, after_loop):
    ticks = rec["u0"].shape[0]
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(v["us"], rec["u0"], equal_nan=True)
    assert np.array_equal(v["Xs"], rec["X"], equal_nan=True) and np.array_equal(v["status"], rec["st"])
    for x, y in zip(after_fwd, after_loop):
        assert np.array_equal(x, y, equal_nan=True)
    if t["tape"] is not None:
        for k in range(ticks):
            X, U, A = (_np(s) for s in eng.closed_loop_tape_slot(t["tape"], k))
            assert np.array_equal(X, rec["Xpre"][k], equal_nan=True) and np.array_equal(U, rec["Upre"][k], equal_nan=True)
            assert np.array_equal(A, rec["act_pre"][k])


def _on(g, which):
    return dict(x0=g["gx0"][which], xr=g["gxr"][:, which], ur=g["gur"][:, which], f=g["gf"][:, which], fp=g["gfp"][:, which])


LOOP_KW = MC.engine_kw(MC.LOOP_CASE)


@pytest.fixture(scope="module")
def loops():
    cache = {}
    yield cache
    for r in cache.values():
        r["eng"].close()


def loop(ndp, oracle, N, cache):
    """Everything the tests of one horizon share, computed once and left unchanged: the oracle's record at LOOP_CASE (the referenced
    six), the device's record from the plain loop, ONE run of the one call and of its reverse with every output, and the reference on
    the device's record at LOOP_CASE's cfg.  The engine of the one call stays open."""
    if N in cache:
        return cache[N]
    a, cpu, cpu_ok, which, ups = C.loop_record(oracle, N)
    cfg = C.loop_cfg(oracle, N)
    eng = _engine(ndp, a, N, **LOOP_KW)
    q, rd, m, g, lb, ub, _ = MC.model_of(MC.LOOP_CASE)
    assert (list(eng.cfg.Qd), list(eng.cfg.Rd), eng.cfg.mass, eng.cfg.gravity) == (list(q), list(rd), m, g)
    assert (list(eng.cfg.lbu), list(eng.cfg.ubu)) == (list(lb), list(ub))
    rec = _loop(eng, a, C.LOOP_K, R.SUBSTEPS)
    after_loop = _state(eng)
    eng.close()
    eng = _engine(ndp, a, N, **LOOP_KW)
    t, vals = _forward(eng, a, N, ticks=C.LOOP_K)
    after_fwd = _state(eng)
    grads = _reverse(eng, t, N, ups)
    r = dict(a=a, cpu=cpu, which=which, ups=ups, cfg=cfg, rec=rec, ok=R.set_finish(rec), after_loop=after_loop, eng=eng, t=t, vals=vals,
             after_fwd=after_fwd, grads=grads, after_bwd=_state(eng))
    if r["ok"][which].all():
        r["sys"] = R.systems(oracle, rec, which, cfg=cfg)
        r["ref"] = R.reverse(r["sys"], rec, *ups)
    cache[N] = r
    return r


@pytest.mark.parametrize("N", C.LOOP_HORIZONS)
def test_closed_loop_values_at_the_loop_model_are_the_plain_loops_bits(ndp, oracle, loops, N):
    """xs, us, Xs, the status words, the tape slots and the engine's iterate and kept set afterwards against the plain loop at LOOP_CASE;
    the reverse call leaves the engine's state alone and recomputes the forward's status words.  And the inputs' conditions on the device:
    the referenced six are set finishes with the oracle's sets, at most B // 4 vehicles are none."""
    r = loop(ndp, oracle, N, loops)
    rec, which, ok = r["rec"], r["which"], r["ok"]
    print(f"N={N}: {int((~ok).sum())} of {C.B} vehicles are no set finishes on the device; referenced {which}; "
          f"{int(rec['act'].any(axis=(0, 2, 3)).sum())} with a pinned input")
    assert len(which) == 6 and ok[which].all() and (~ok).sum() <= C.B // 4
    assert np.array_equal(rec["act"][:, which], r["cpu"]["act"][:, which])
    lo, hi = np.array(MC.LOOP_CASE["lbu"]), np.array(MC.LOOP_CASE["ubu"])
    assert (rec["u0"][:, ok] >= lo - 1e-9).all() and (rec["u0"][:, ok] <= hi + 1e-9).all() and rec["act"].any()       # the asymmetric box binds
    _assert_values(r["vals"], rec, r["eng"], r["t"], r["after_fwd"], r["after_loop"])
    assert np.array_equal(r["grads"]["status_check"], rec["st"])
    for x, y in zip(r["after_fwd"], r["after_bwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    # the oracle's loop at this model, within the value bar of the chain's tests (VALUE_ATOL) on the referenced six
    errs = [float(np.abs(rec[n][:, which] - r["cpu"][n][:, which]).max()) for n in ("u0", "x", "X")]
    print(f"N={N}: against the oracle's loop at this model, worst absolute difference u0 {errs[0]:.2e}, x {errs[1]:.2e}, X {errs[2]:.2e}")
    assert max(errs) <= VALUE_ATOL, errs


@pytest.mark.parametrize("N", C.LOOP_HORIZONS)
def test_closed_loop_gradients_at_the_loop_model(ndp, oracle, loops, N):
    """Every leaf gradient within BAR["ext"] of closed_loop_chain_ref.reverse on the device's record with the systems at LOOP_CASE's cfg;
    the model gradient within its bars with this model's 1 / m; column 6 is exactly 0 although Qd[6] = 7 here (row 6 of the cost's
    residual is the constant 0 whatever Qd[6] is: tests/test_model_envelope.py)."""
    r = loop(ndp, oracle, N, loops)
    which = r["which"]
    e = C.loop_leaf_errors(_on(r["grads"], which), r["ref"])
    per = [R.rel_err(r["grads"]["gx0"][[v]], r["ref"]["x0"][[j]], 1) for j, v in enumerate(which)]
    print(f"N={N}: x0 per referenced vehicle " + " ".join(f"{v}: {x:.2e}" for v, x in zip(which, per)))
    gm = r["grads"]["gmodel"]
    e14, e15, tot = C.loop_model_errors(oracle, r["sys"], r["rec"], r["ups"], gm[which], r["cfg"], LEAF_BAR, STEP_BAR)
    print(f"N={N}: leaves " + " ".join(f"{n} {v:.3e}" for n, v in e.items()) + f" (bar {LEAF_BAR:.2e}); model gradient's worst share of its "
          f"bar: columns 0..14 {e14:.3e}, column 15 {e15:.3e}")
    # N = 20: x0 stands at 91 % of this bar through ONE vehicle (number 0) whose KKT systems have condition 4e6 and whose float64
    # reference disagrees with itself by 9.5e-12 (module docstring).  A margin of 9 % on a figure that is partly the reference's
    # rounding can go with another compiler, ROCm or LAPACK: if this fails, look at the per-vehicle line above before the kernel --
    # the other five vehicles are the ones that tell a defect (they sit at 1e-12 and below).
    assert max(e.values()) <= LEAF_BAR, e
    assert e14 <= 1.0 and e15 <= 1.0
    assert np.isfinite(gm[r["ok"]]).all() and not gm[r["ok"]][:, 6].any() and np.abs(gm[which, 15]).max() > 1e-3


@pytest.mark.parametrize("N", C.LOOP_HORIZONS)
def test_closed_loop_device_finite_differences_in_the_model(ndp, oracle, loops, N):
    """Central differences of L over the device's own closed loop at LOOP_CASE through set_model in Qd[0], Rd[3] and the mass (steps 1e-5
    of the value; the mass moves controller and plant: column 14 + column 15), every tick of every perturbed run restarted from the
    recorded iterate and kept set: within FD_BAR of max(1, |g|) on the vehicles whose sets and iteration words move in no run, at least
    40 of the 65."""
    r = loop(ndp, oracle, N, loops)
    a, rec, gm = r["a"], r["rec"], r["grads"]["gmodel"]
    G, H, A = r["ups"]
    eng = ndp.BatchedNMPC(C.B, N=N, disturbance=True, **LOOP_KW)
    eng.reset(a["xr"][0], a["ur"][0])
    Qd0, Rd0, m0 = np.array(list(eng.cfg.Qd)), np.array(list(eng.cfg.Rd)), float(eng.cfg.mass)
    assert (Qd0[0], Rd0[3], m0) == (120.0, 13.0, 0.9)
    cases = [("Qd", 1e-5 * Qd0[0], gm[:, 0]), ("Rd", 1e-5 * Rd0[3], gm[:, 13]), ("mass", 1e-5 * m0, gm[:, 14] + gm[:, 15])]
    stable, fds = r["ok"].copy(), []
    for name, h, _ in cases:
        L = []
        for sgn in (1.0, -1.0):
            q, rd, m = Qd0.copy(), Rd0.copy(), m0
            if name == "Qd":
                q[0] += sgn * h
            elif name == "Rd":
                rd[3] += sgn * h
            else:
                m += sgn * h
            eng.set_model(Qd=q, Rd=rd, mass=m)
            x, tot = a["x0"].copy(), np.zeros(C.B)
            for k in range(C.LOOP_K):
                eng.set_iterate(rec["Xpre"][k], rec["Upre"][k])
                eng.set_active_set(rec["act_pre"][k])
                u, X, U, st, it = eng.update(x, a["xr"][k], a["ur"][k], f=a["f"][k], raise_on_status=False, full=True)
                stable &= (st == 0) & ((it & 0xffff) == 0) & (eng.active_set()[1] == rec["act"][k]).all(axis=(1, 2))
                x = eng.plant_step(x, u, a["fp"][k], dt=R.DT, substeps=R.SUBSTEPS)
                tot += (G[k] * x).sum(axis=1) + (H[k] * u).sum(axis=1) + (A[k] * X).sum(axis=(1, 2))
            L.append(tot)
        fds.append((L[0] - L[1]) / (2 * h))
    eng.close()
    print(f"N={N}: {int(stable.sum())} of {C.B} vehicles keep their sets and iteration words in every run")
    assert stable.sum() >= 40
    for (name, h, got), fd in zip(cases, fds):
        err = float((np.abs(fd - got)[stable] / np.maximum(1.0, np.abs(got[stable]))).max())
        print(f"N={N}: {name} worst |fd - g| / max(1, |g|) = {err:.2e}, |g|max {np.abs(got[stable]).max():.2e}")
        assert err <= FD_BAR and np.abs(got[stable]).max() > 1e-3, (name, err)


@pytest.mark.parametrize("N", C.LOOP_HORIZONS)
def test_set_model_before_the_warm_up_gives_the_created_handles_bits(ndp, oracle, loops, N):
    """A handle created with LOOP_CASE's box and g but the DEFAULT Qd, Rd and mass, given set_model(Qd, Rd, mass) before its warm-up step:
    every output of the one call and of its reverse is bit-equal to the created handle's."""
    r = loop(ndp, oracle, N, loops)
    q, rd, m = MC.model_of(MC.LOOP_CASE)[:3]
    kw = MC.engine_kw({k: v for k, v in MC.LOOP_CASE.items() if k not in ("Qd", "Rd", "mass")})
    eng = _engine(ndp, r["a"], N, moved=(q, rd, m), **kw)
    t, vals = _forward(eng, r["a"], N, ticks=C.LOOP_K)
    after = _state(eng)
    grads = _reverse(eng, t, N, r["ups"])
    for n in ("xs", "us", "Xs", "status"):
        assert np.array_equal(vals[n], r["vals"][n], equal_nan=True), n
    for k in range(C.LOOP_K):                                                    # (slot by slot: a slot's padding bytes are nobody's)
        for s, u in zip(eng.closed_loop_tape_slot(t["tape"], k), r["eng"].closed_loop_tape_slot(r["t"]["tape"], k)):
            assert np.array_equal(_np(s), _np(u), equal_nan=True), k
    eng.close()
    for x, y in zip(after, r["after_fwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    for n in OUTS + ("gmodel", "status_check"):
        assert np.array_equal(grads[n], r["grads"][n], equal_nan=True), n


def test_closed_loop_at_a_plant_step_that_is_no_power_of_two(ndp, oracle, loops):
    """K = 2 at N = 20 with the call's dt = 0.05 and substeps = 3 (h = dt / 3): values the plain loop's bits at that dt and substeps and within
    VALUE_ATOL of the oracle's loop at this model, dt and substeps on the referenced six, leaf
    gradients within BAR["ext"] of the reference with the plant's Jacobian at that dt and substeps, the model gradient within its bars."""
    run_ = C.LOOP_DT_RUN
    N, ticks, dt, sub = run_["N"], run_["K"], run_["dt"], run_["substeps"]
    r0 = loop(ndp, oracle, N, loops)
    a, which, cfg = r0["a"], r0["which"], r0["cfg"]
    eng = _engine(ndp, a, N, **LOOP_KW)
    rec = _loop(eng, a, ticks, sub, dt=dt)
    after_loop = _state(eng)
    eng.close()
    eng = _engine(ndp, a, N, **LOOP_KW)
    t, v = _forward(eng, a, N, ticks=ticks, substeps=sub, dt=dt)
    _assert_values(v, rec, eng, t, _state(eng), after_loop)
    ups = tuple(u[:ticks] for u in r0["ups"])
    g = _reverse(eng, t, N, ups)
    eng.close()
    assert R.set_finish(rec)[which].all() and np.abs(rec["x"][1:] - r0["rec"]["x"][1:ticks + 1]).max() > 1e-3         # (another plant tick)
    cpu = R.nominal_cpu(oracle, a["x0"], a["xr"][:ticks], a["ur"][:ticks], a["fp"][:ticks], f=a["f"][:ticks], dt=dt, substeps=sub, cfg=cfg)
    errs = [float(np.abs(rec[n][:, which] - cpu[n][:, which]).max()) for n in ("u0", "x", "X")]
    print(f"dt {dt} substeps {sub}: against the oracle's loop at this model, worst absolute difference u0 {errs[0]:.2e}, x {errs[1]:.2e}, X {errs[2]:.2e}")
    assert max(errs) <= VALUE_ATOL, errs
    sys_ = R.systems(oracle, rec, which, dt=dt, substeps=sub, cfg=cfg)
    e = C.loop_leaf_errors(_on(g, which), R.reverse(sys_, rec, *ups))
    e14, e15, _ = C.loop_model_errors(oracle, sys_, rec, ups, g["gmodel"][which], cfg, LEAF_BAR, STEP_BAR)
    print(f"dt {dt} substeps {sub}: leaves " + " ".join(f"{n} {x:.3e}" for n, x in e.items()) + f" (bar {LEAF_BAR:.2e}); model gradient's "
          f"worst share of its bar: columns 0..14 {e14:.3e}, column 15 {e15:.3e}")
    assert max(e.values()) <= LEAF_BAR, e
    assert e14 <= 1.0 and e15 <= 1.0


# ================================================================ f. the horizons of the one call
@pytest.mark.parametrize("N", C.EDGE_HORIZONS)
def test_one_call_at_the_edge_horizons_is_the_plain_loop(ndp, N):
    """Default model, B = 65, K = 2, N = 2 and 27 (the ends of the three-slot range), 28 and 40 (five slots): xs, us, Xs, the status
    words, the tape slots and the engine's state afterwards are the plain loop's bits, with a tape and without one; the guard rows stay
    (checked in _forward).  At N = 28 the reverse call returns -2, names itself and the N <= 27 rule, and leaves every output buffer, the
    tape and the engine's state untouched."""
    import torch
    a = R.ext_inputs(C.B, C.EDGE_K, N, C.EDGE_SEED)
    eng = _engine(ndp, a, N)
    rec = _loop(eng, a, C.EDGE_K, R.SUBSTEPS)
    after_loop = _state(eng)
    eng.close()
    assert (rec["st"] == 0).sum() >= rec["st"].size // 2                         # (most steps are served; the bits are compared on all)
    for tape in (True, False):
        eng = _engine(ndp, a, N)
        t, v = _forward(eng, a, N, ticks=C.EDGE_K, tape=tape)
        after = _state(eng)
        _assert_values(v, rec, eng, t, after, after_loop)
        if tape and N == 28:
            ups = R.upstreams(C.EDGE_K, C.B, N, seed=C.LOOP_UPS_SEED)
            kept = _np(t["tape"]).copy()
            n = C.B
            shapes = dict(gx0=(n, 10), gxr=(C.EDGE_K, n, N + 1, 10), gur=(C.EDGE_K, n, N, 4), gf=(C.EDGE_K, n, N + 1, 3), gfp=(C.EDGE_K, n, 3),
                          gmodel=(n, 16))
            o = {k: torch.full(s, -7.0, dtype=torch.float64, device=_dev()) for k, s in shapes.items()}
            st = torch.full((C.EDGE_K, n), -7, dtype=torch.int32, device=_dev())
            g = [_t(u) for u in ups]
            torch.cuda.synchronize()
            with pytest.raises(ndp.NdpError, match=r"ndp_closed_loop_vjp_device failed \(-2\): ndp_closed_loop_vjp_device.*N <= 27"):
                eng.closed_loop_vjp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["tape"], f=t["f"], fp=t["fp"], gxs=g[0], gus=g[1],
                                           gXs=g[2], status_check=st, **o)
            eng.synchronize()
            torch.cuda.synchronize()
            for k, buf in o.items():
                assert (_np(buf) == -7.0).all(), k
            assert (_np(st) == -7).all() and np.array_equal(_np(t["tape"]), kept)
            for x, y in zip(_state(eng), after):
                assert np.array_equal(x, y, equal_nan=True)
        eng.close()
