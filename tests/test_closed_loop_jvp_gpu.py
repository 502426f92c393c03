"""The one-call forward mode of the closed loop on the device (run with -m gpu): ndp_closed_loop_jvp_device against the composed float64
forward sweep of tests/closed_loop_chain_ref.py, against its own links (ndp_step_jvp_device bit for bit, the plant's complex-step
Jacobian), and in duality with ndp_closed_loop_vjp_device on the same record -- at N = 20 (the compile-time kernels) and N = 7 (the
run-time-horizon kernels), K = 3 ticks, B = 65 (one vehicle past a full 64-lane workgroup of the link kernel).
CPU side: tests/test_closed_loop_jvp.py.

Inputs: closed_loop_chain_ref.ext_inputs(65, 3, N, 20231516), the inputs of tests/test_closed_loop_vjp_gpu.py (whose `full` builds the
record, the one call's forward and its reverse once per horizon); directions closed_loop_chain_ref.tangents(K, B, N, T, seed = 41).

Bars, none of them from what the code under test gives:
  tangents     BAR["ext"] = 1.24e-11 of tests/test_closed_loop_chain_gpu.py (ten times what the hand-chained forward mode through the same
               links measured), by closed_loop_chain_ref.rel_err with lead 3
  step link    bit-equality with ndp_step_jvp_device on the same tape slot and directions
  plant link   the plant's own PLANT_BAR = 1e-13 (plant_deriv_ref.within_bar) against the complex-step Jacobian at (x_k, u0_k, fp_k)
  duality      K x 1e-10 of the largest term (test_forward_mode_chained_by_hand's bar for the ext form)
  other model  per vehicle max(BAR["ext"], 10 x that vehicle's own forward / reverse duality gap of the float64 reference), the gap taken
               as |lhs - rhs| in the worst direction (closed_loop_jvp_cases.reference_gap says why not over the largest term)
Measured on the first device run (MI355X), all 65 vehicles set finishes on the device at both horizons:
  tangents     N = 20: dxs 1.1e-13, dus 8.8e-13, dXs 1.2e-12; N = 7: dxs 2.6e-13, dus 8.6e-13, dXs 8.0e-13
  plant link   1.5e-15 (N = 20), 6.7e-16 (N = 7); substeps 1 / 16 (K = 2): 7.0e-16 / 1.3e-15; the bits are plant_rollout_jvp_device's
               at every tick and substep count (reported, not required)
  duality      7.2e-14 (N = 20), 2.6e-14 (N = 7); substeps 1 / 16: 1.7e-13 / 1.3e-13
  other model  vehicle 0 (the ill-conditioned one): dxs 4.0e-12, dus 1.6e-11, dXs 1.7e-11 against its own bar 6.5e-11 (the reference's
               gap 6.5e-12); the other five at most 1.4e-12 against the flat bar (their gaps 2.8e-13 .. 9.7e-13)
With 1 / 1.4844 in place of 1 / cfg.mass in the tangent link's plant arguments (a temporary build, nothing of it kept) the other-model
test fails and the other 22 pass."""
import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import closed_loop_jvp_cases as J
from tests import model_cases as MC
from tests import plant_deriv_ref as P
from tests import plant_side_cases as C
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.test_closed_loop_chain_gpu import BAR, PLANT_BAR
from tests.test_closed_loop_vjp_gpu import GUARD, _engine, _forward, _guarded, _loop, _np, _reverse, _state, full

pytestmark = pytest.mark.gpu

K, B = J.K, J.B
HORIZONS = list(J.HORIZONS)
OUTS = ("dxs", "dus", "dXs", "dUs")
WHO = "ndp_closed_loop_jvp_device"


def _jvp(eng, t, N, tan, ask=("dXs", "dUs"), stream=None, status=True):
    """closed_loop_jvp_device into guarded, -7.0-filled outputs on the record t (_forward's); tan: {tx0, txr, tur, tf, tfp} numpy arrays
    or None.  Returns {name: numpy} of dxs, dus, what was asked for and status_check, and under "tensors" the device tensors."""
    import torch
    ticks, n = t["xr"].shape[0], t["x0"].shape[0]
    T = next(v.shape[1 if name == "tx0" else 2] for name, v in tan.items() if v is not None)
    shapes = dict(dxs=(ticks, n, T, 10), dus=(ticks, n, T, 4), dXs=(ticks, n, T, N + 1, 10), dUs=(ticks, n, T, N, 4))
    o = {k: _guarded(*shapes[k]) for k in ("dxs", "dus") + tuple(ask)}
    st = _guarded(ticks, n, dtype=torch.int32, fill=-7) if status else None
    d = {name: None if v is None else _t(v if name == "tx0" else v[:ticks]) for name, v in tan.items()}
    torch.cuda.synchronize()
    eng.closed_loop_jvp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["tape"], o["dxs"][0], o["dus"][0], f=t["f"], fp=t["fp"],
                               dXs=o["dXs"][0] if "dXs" in o else None, dUs=o["dUs"][0] if "dUs" in o else None,
                               status_check=st[0].view(ticks, n) if status else None, dt=t.get("dt", R.DT), substeps=t["substeps"],
                               stream=stream, **d)
    eng.synchronize()
    torch.cuda.synchronize()
    for k, v in list(o.items()) + ([("status_check", st)] if status else []):
        assert (_np(v[1])[-GUARD:] == -7).all(), k
    out = {k: _np(v[0]) for k, v in o.items()}
    if status:
        out["status_check"] = _np(st[0]).reshape(ticks, n)
    out["tensors"] = dict({k: v[0] for k, v in o.items()}, **d)
    return out


def _same(a, b, names=OUTS):
    for n in names:
        assert np.array_equal(a[n], b[n], equal_nan=True), n


def _only(tan, T=None, keep=None, ticks=None):
    """A copy of the directions: the first T of them, only the names in keep (the others None)."""
    out = {}
    for name, v in tan.items():
        if keep is not None and name not in keep:
            out[name] = None
            continue
        out[name] = v if T is None else np.ascontiguousarray(v[:, T] if name == "tx0" else v[:, :, T])
    return out


@pytest.fixture(scope="module")
def shared():
    cache = {}
    yield cache
    for r in cache.values():
        r["eng"].close()


def jfull(ndp, oracle, N, cache):
    """tests/test_closed_loop_vjp_gpu.py's `full` of one horizon (inputs, record, the one call's forward and reverse, the reference
    systems), plus ONE forward-mode run along T = 2 directions with every output and the float64 forward sweep on the device's record:
    computed once and left unchanged."""
    r = full(ndp, oracle, N, cache)
    if "jv" not in r:
        r["tan"] = J.directions(K, B, N, 2)
        r["jv"] = _jvp(r["eng"], r["t"], N, r["tan"])
        r["after_jvp"], r["tape_after_jvp"] = _state(r["eng"]), _np(r["t"]["tape"])
        r["st_ok"] = (r["vals"]["status"] == 0).all(axis=0)
        if "sys" in r:
            r["jref"] = J.reference(r["sys"], r["rec"], r["tan"])
    return r


# ---- 1. against the float64 reference
@pytest.mark.parametrize("N", HORIZONS)
def test_tangents_match_the_forward_sweep(ndp, oracle, shared, N):
    """dxs, dus, dXs of the six referenced vehicles against closed_loop_chain_ref.forward on the device's own record, by rel_err with
    lead 3, held to BAR["ext"]."""
    r = jfull(ndp, oracle, N, shared)
    jv = r["jv"]
    assert r["ok"][r["which"]].all() and np.array_equal(jv["status_check"], r["vals"]["status"])
    e = J.errors((jv["dxs"], jv["dus"], jv["dXs"]), r["jref"], r["which"])
    print(f"N={N}: one call against the forward sweep, measured " + " ".join(f"{n} {v:.3e}" for n, v in e.items()) + f"; bar {BAR['ext']:.2e}")
    assert np.isfinite(jv["dxs"][:, r["ok"]]).all() and np.abs(jv["dxs"][:, r["which"]]).max() > 1e-3
    assert max(e.values()) <= BAR["ext"], e


# ---- 2. the step link is the existing kernel
@pytest.mark.parametrize("N", HORIZONS)
def test_the_step_link_is_the_step_forward_mode_bit_for_bit(ndp, oracle, shared, N):
    """Per tick, step_jvp_device by hand on closed_loop_tape_slot(k) with tx0 = the one call's own dxs[k-1] (tx0 at k = 0) reproduces the
    one call's dus[k], dXs[k] and dUs[k] bit for bit, and dUs[k][:, :, 0] is dus[k] -- what holds dUs (the reference sweep returns none)."""
    import torch
    r = jfull(ndp, oracle, N, shared)
    eng, t, jv, ten, ok = r["eng"], r["t"], r["jv"], r["jv"]["tensors"], r["st_ok"]
    T = jv["dxs"].shape[2]
    assert ok.sum() >= B - B // 4
    for k in range(K):
        z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
        du0, dX, dU = z(B, T, 4), z(B, T, N + 1, 10), z(B, T, N, 4)
        torch.cuda.synchronize()
        eng.step_jvp_device(t["x0"] if k == 0 else t["xs"][k - 1], t["xr"][k], t["ur"][k], eng.closed_loop_tape_slot(t["tape"], k),
                            tx0=ten["tx0"] if k == 0 else ten["dxs"][k - 1], txr=ten["txr"][k], tur=ten["tur"][k], tf=ten["tf"][k],
                            f=t["f"][k], du0=du0, dX=dX, dU=dU)
        eng.synchronize()
        assert np.array_equal(_np(du0)[ok], jv["dus"][k][ok]), k
        assert np.array_equal(_np(dX), jv["dXs"][k], equal_nan=True) and np.array_equal(_np(dU), jv["dUs"][k], equal_nan=True), k
        assert np.array_equal(jv["dUs"][k][ok][:, :, 0], jv["dus"][k][ok]), k
    assert np.array_equal(_np(t["tape"]), r["tape_after_jvp"])


# ---- 3. the plant link
def _plant_errors(eng, t, jv, tan, ok, substeps, dt=R.DT):
    """(the worst within_bar ratio of dxs[k] against the plant's complex-step Jacobian at (x_k, u0_k, fp_k) applied to the one call's own
    (dxs[k-1], dus[k], tfp[k]) over the vehicles in ok; whether every tick's bits are plant_rollout_jvp_device(ticks = 1)'s)."""
    import torch
    ticks = jv["dxs"].shape[0]
    xs, us, fp = _np(t["xs"]), _np(t["us"]), _np(t["fp"])
    ten, worst, bits = jv["tensors"], 0.0, True
    for k in range(ticks):
        xk = _np(t["x0"]) if k == 0 else xs[k - 1]
        txk = tan["tx0"] if k == 0 else jv["dxs"][k - 1]
        Jk = P.jacobian(xk[ok], us[k][ok][None], fp[k][ok][None], dt, substeps, float(eng.cfg.mass), float(eng.cfg.gravity))
        ref = P.jvp(Jk, tx0=txk[ok], tu=jv["dus"][k][ok][None], tf=tan["tfp"][k][ok][None])[0]
        good, ratio = P.within_bar(jv["dxs"][k][ok], ref, PLANT_BAR)
        worst = max(worst, ratio)
        alone = torch.full_like(ten["dxs"][k], -7.0)[None]
        torch.cuda.synchronize()
        eng.plant_rollout_jvp_device(t["x0"] if k == 0 else t["xs"][k - 1], t["us"][k][None], alone, f=t["fp"][k][None],
                                     tx0=ten["tx0"] if k == 0 else ten["dxs"][k - 1], tu=ten["dus"][k][None], tf=ten["tfp"][k][None],
                                     dt=dt, substeps=substeps)
        eng.synchronize()
        bits = bits and np.array_equal(_np(alone)[0][ok], jv["dxs"][k][ok])
    return worst, bits


@pytest.mark.parametrize("N", HORIZONS)
def test_the_plant_link_meets_the_plants_bar(ndp, oracle, shared, N):
    r = jfull(ndp, oracle, N, shared)
    worst, bits = _plant_errors(r["eng"], r["t"], r["jv"], r["tan"], r["st_ok"], R.SUBSTEPS)
    print(f"N={N}: plant link against the complex-step Jacobian, worst {worst:.3e} (bar {PLANT_BAR:.0e}); "
          f"bit-equal to plant_rollout_jvp_device(ticks = 1): {bits} (reported, not required)")
    assert worst <= PLANT_BAR


@pytest.mark.parametrize("substeps", [1, 16])
def test_the_plant_link_at_substeps_1_and_16(ndp, oracle, shared, substeps):
    """K = 2 at N = 20: the plant link against the Jacobian at that number of substeps, and duality with the reverse call."""
    N, ticks = 20, 2
    r0 = jfull(ndp, oracle, N, shared)
    eng = _engine(ndp, r0["a"], N)
    t, v = _forward(eng, r0["a"], N, ticks=ticks, substeps=substeps)
    tan = {n: (x if n == "tx0" else x[:ticks]) for n, x in r0["tan"].items()}
    jv = _jvp(eng, t, N, tan)
    ups = tuple(u[:ticks] for u in r0["ups"])
    g = _reverse(eng, t, N, ups, ask=("gx0", "gxr", "gur", "gf", "gfp"))
    ok = (v["status"] == 0).all(axis=0)
    worst, bits = _plant_errors(eng, t, jv, tan, ok, substeps)
    eng.close()
    gap = J.duality_gap((jv["dxs"], jv["dus"], jv["dXs"]), dict(x0=g["gx0"], xr=g["gxr"], ur=g["gur"], f=g["gf"], fp=g["gfp"]), tan, ups)
    print(f"substeps {substeps}: plant link worst {worst:.3e} (bar {PLANT_BAR:.0e}), bit-equal to the stand-alone kernel: {bits}; "
          f"duality gap {gap[ok].max():.3e} (bar {ticks * 1e-10:.0e})")
    assert worst <= PLANT_BAR and gap[ok].max() <= ticks * 1e-10


# ---- 4. duality with the reverse call
@pytest.mark.parametrize("N", HORIZONS)
def test_duality_with_the_reverse_call(ndp, oracle, shared, N):
    """<G, dxs> + <H, dus> + <A, dXs> = <gx0, tx0> + <gxr, txr> + <gur, tur> + <gf, tf> + <gfp, tfp> on the same record, per vehicle and
    direction over all set finishes: the gap over the largest term within K x 1e-10."""
    r = jfull(ndp, oracle, N, shared)
    jv, g = r["jv"], r["grads"]
    gap = J.duality_gap((jv["dxs"], jv["dus"], jv["dXs"]), dict(x0=g["gx0"], xr=g["gxr"], ur=g["gur"], f=g["gf"], fp=g["gfp"]), r["tan"],
                        r["ups"])[r["ok"]]
    print(f"N={N}: duality of the one-call forward mode with the one-call reverse mode over {int(r['ok'].sum())} vehicles, worst gap "
          f"{gap.max():.3e} of the largest term (bar {K * 1e-10:.0e})")
    assert r["ok"].sum() >= B - B // 4 and gap.max() <= K * 1e-10


# ---- 5. directions and shapes
@pytest.mark.parametrize("N", HORIZONS)
def test_t_directions_in_one_call_are_t_calls_of_one(ndp, oracle, shared, N):
    """T = 8 (520 lanes) and T = 3 (195 lanes, a last workgroup of 3): one call equals T one-direction calls, bit for bit."""
    r = jfull(ndp, oracle, N, shared)
    eng, t = r["eng"], r["t"]
    tan8 = J.directions(K, B, N, 8)
    all8 = _jvp(eng, t, N, tan8)
    all3 = _jvp(eng, t, N, _only(tan8, T=slice(0, 3)))
    for d in range(8):
        one = _jvp(eng, t, N, _only(tan8, T=slice(d, d + 1)))
        for n in OUTS:
            assert np.array_equal(one[n][:, :, 0], all8[n][:, :, d], equal_nan=True), (n, d)
            if d < 3:
                assert np.array_equal(one[n][:, :, 0], all3[n][:, :, d], equal_nan=True), (n, d)
    assert np.array_equal(all8["status_check"], r["vals"]["status"]) and np.isfinite(all8["dxs"][:, r["ok"]]).all()


@pytest.mark.parametrize("N", HORIZONS)
def test_single_tangents_and_optional_outputs(ndp, oracle, shared, N):
    """Each of the five directions given alone, the others NULL, equals the same direction beside explicit zeros, bit for bit (tfp alone:
    tick 0's step is launched on four NULLs); dXs / dUs NULL, or the status log NULL, leave dxs and dus bit-unchanged."""
    r = jfull(ndp, oracle, N, shared)
    eng, t, tan = r["eng"], r["t"], r["tan"]
    for name in J.NAMES:
        alone = _jvp(eng, t, N, _only(tan, keep=(name,)))
        zeros = _jvp(eng, t, N, {n: (v if n == name else np.zeros_like(v)) for n, v in tan.items()})
        _same(alone, zeros)
        assert np.abs(alone["dxs"][:, r["ok"]]).max() > 0.0, name
    for ask in ((), ("dXs",), ("dUs",)):
        part = _jvp(eng, t, N, tan, ask=ask, status=(ask != ()))
        _same(part, r["jv"], ("dxs", "dus") + ask)


@pytest.mark.parametrize("N", HORIZONS)
def test_one_vehicle_one_tick_one_direction_and_no_force(ndp, oracle, shared, N):
    """B = 1, ticks = 1, T = 1 gives vehicle 0's tick-0 rows of the full run's direction 0 (a vehicle's arithmetic knows neither B nor T);
    a use_fd = 0 engine without forces runs, and refuses a force direction."""
    import torch
    r = jfull(ndp, oracle, N, shared)
    a = r["a"]
    one = {k: (v[:1] if k == "x0" else v[:, :1]) for k, v in a.items()}
    eng = _engine(ndp, one, N)
    t, v = _forward(eng, one, N, ticks=1)
    tan1 = {n: np.ascontiguousarray(x[:1, :1] if n == "tx0" else x[:1, :1, :1]) for n, x in r["tan"].items()}
    jv = _jvp(eng, t, N, tan1)
    eng.close()
    for n in OUTS:
        assert np.array_equal(jv[n][0, 0, 0], r["jv"][n][0, 0, 0], equal_nan=True), n
    eng = _engine(ndp, a, N, force=False)
    t, v = _forward(eng, a, N, force=False)
    nof = _jvp(eng, t, N, _only(r["tan"], keep=("tx0", "txr", "tur", "tfp")))
    assert np.isfinite(nof["dxs"][:, (v["status"] == 0).all(axis=0)]).all()
    out = torch.full((K, B, 2, 10), -7.0, dtype=torch.float64, device=_dev()), torch.full((K, B, 2, 4), -7.0, dtype=torch.float64, device=_dev())
    with pytest.raises(ndp.NdpError, match=WHO + r" failed \(-2\): " + WHO + ".*use_fd"):
        eng.closed_loop_jvp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["tape"], out[0], out[1], tf=_t(r["tan"]["tf"]))
    eng.synchronize()
    eng.close()
    assert (_np(out[0]) == -7.0).all() and (_np(out[1]) == -7.0).all()


# ---- 6. state, repeats and streams
@pytest.mark.parametrize("N", HORIZONS)
def test_state_repeats_streams_and_the_shared_workspace(ndp, oracle, shared, N):
    """The engine's iterate, kept set and the tape are bit-unchanged by the call; two calls are bit-identical; a reverse call behind the
    forward-mode call gives the gradients of the one in front of it, and a forward-mode call behind that the same tangents (one workspace);
    forward and forward mode on a side stream give the same bits; guard rows are checked in _jvp."""
    import torch
    r = jfull(ndp, oracle, N, shared)
    eng, t, jv = r["eng"], r["t"], r["jv"]
    for x, y in zip(r["after_jvp"], r["after_fwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(r["tape_after_jvp"], r["tape_after"])
    g = _reverse(eng, t, N, r["ups"])
    for n in ("gx0", "gxr", "gur", "gf", "gfp", "gmodel", "status_check"):
        assert np.array_equal(g[n], r["grads"][n], equal_nan=True), n
    again = _jvp(eng, t, N, r["tan"])
    _same(again, jv, OUTS + ("status_check",))
    for x, y in zip(_state(eng), r["after_fwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    side = torch.cuda.Stream(device=_dev())
    eng2 = _engine(ndp, r["a"], N)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t2, v2 = _forward(eng2, r["a"], N, stream=side)
        jv2 = _jvp(eng2, t2, N, r["tan"], stream=side)
    side.synchronize()
    eng2.close()
    _same(jv2, jv, OUTS + ("status_check",))


# ---- 7. a NaN vehicle
def test_a_nan_vehicle_stays_with_itself(ndp, oracle, shared):
    """N = 20, vehicle 1 given a NaN velocity in x_0 (its status is 1 in every tick): its dxs and dus are NaN at every tick and in every
    direction, every other vehicle's outputs are bit-equal to the clean run's, and the recomputed status words are the forward's."""
    N, bad = 20, 1
    r = jfull(ndp, oracle, N, shared)
    a = dict(r["a"], x0=r["a"]["x0"].copy())
    a["x0"][bad, 3] = np.nan
    eng = _engine(ndp, a, N)
    t, v = _forward(eng, a, N)
    jv = _jvp(eng, t, N, r["tan"])
    eng.close()
    rest = np.arange(B) != bad
    assert (v["status"][:, bad] != 0).all() and np.array_equal(jv["status_check"], v["status"])
    assert np.isnan(jv["dxs"][:, bad]).all() and np.isnan(jv["dus"][:, bad]).all()
    assert np.isnan(jv["dXs"][0, bad]).all() and np.isnan(jv["dUs"][0, bad]).all()
    for n in OUTS:
        assert np.array_equal(jv[n][:, rest], r["jv"][n][:, rest], equal_nan=True), n


# ---- 8. refusals
def test_refusals_name_the_call_and_enqueue_nothing(ndp, oracle, shared):
    """Every -1 / -2 case of include/ndp_nmpc.h returns its code with a reason that names the call; the -7-filled outputs, the tape and the
    engine keep their bits."""
    import ctypes as Ct
    import torch
    N = 7
    r = jfull(ndp, oracle, N, shared)
    t = r["t"]
    eng = ndp.BatchedNMPC(B, N=N, disturbance=True)        # (a handle of its own: the sensitivities are switched on and off on it)
    before = _state(eng)
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    dxs, dus, dXs = z(K, B, 2, 10), z(K, B, 2, 4), z(K, B, 2, N + 1, 10)
    tx0 = _t(r["tan"]["tx0"])
    call = lambda e=eng, **kw: e.closed_loop_jvp_device(**{**dict(x0=t["x0"], xr=t["xr"], ur=t["ur"], xs=t["xs"], us=t["us"], tape=t["tape"],  # noqa: E731
                                                                  dxs=dxs, dus=dus, dXs=dXs, f=t["f"], fp=t["fp"], tx0=tx0, n_tan=2), **kw})
    for kw, code in ((dict(x0=None), -1), (dict(ur=None), -1), (dict(us=None), -1), (dict(xs=None), -1)):
        with pytest.raises(ndp.NdpError, match=WHO + r" failed \(%d\)" % code):
            call(**kw)
    for kw, why in ((dict(substeps=0), "substeps"), (dict(substeps=17), "substeps"), (dict(tape=None), "d_tape"),
                    (dict(tx0=None), "no tangent"), (dict(dxs=None), "d_dxs"), (dict(dus=None), "d_dus"),
                    (dict(n_tan=0, tx0=z(B, 0, 10), dxs=z(K, B, 0, 10), dus=z(K, B, 0, 4), dXs=None), "n_tan"),
                    (dict(n_tan=9, tx0=z(B, 9, 10), dxs=z(K, B, 9, 10), dus=z(K, B, 9, 4), dXs=None), "n_tan")):
        with pytest.raises(ndp.NdpError, match=WHO + r" failed \(-2\): " + WHO + ".*" + why):
            call(**kw)
    eng.enable_sensitivity(1)
    with pytest.raises(ndp.NdpError, match=WHO + r" failed \(-2\).*" + WHO + ".*sensitivities"):
        call()
    eng.enable_sensitivity(0)
    args = [0, R.DT, 4] + [Ct.c_void_p(dxs.data_ptr())] * 8 + [1] + [Ct.c_void_p(dxs.data_ptr())] * 11           # ticks < 1, and a NULL handle
    assert eng._lib.ndp_closed_loop_jvp_device(eng._h, *args) == -2 and WHO.encode() in eng._lib.ndp_last_error(eng._h)
    assert eng._lib.ndp_closed_loop_jvp_device(None, *args) == -1
    # a force without use_fd; the derivative's own refusals, N = 28 among them
    two = {k: (v[:2] if k == "x0" else v[:, :2]) for k, v in r["a"].items()}
    for kw, n_hor, why in ((dict(disturbance=False), N, "use_fd"), (dict(n_rti=2), N, "n_rti"), (dict(qp_precision=1), N, "qp_precision"),
                           (dict(), 28, "N <= 27"), (dict(), 30, "N <= 27")):
        e = ndp.BatchedNMPC(2, N=n_hor, **({"disturbance": True, **kw}))
        tt = dict(x0=_t(two["x0"]), xr=z(K, 2, n_hor + 1, 10), ur=z(K, 2, n_hor, 4), f=torch.zeros(K, 2, n_hor + 1, 3, dtype=torch.float32, device=_dev()),
                  fp=_t(two["fp"]), xs=z(K, 2, 10), us=z(K, 2, 4), dxs=z(K, 2, 1, 10), dus=z(K, 2, 1, 4))
        with pytest.raises(ndp.NdpError, match=WHO + r" failed \(-2\): " + WHO + ".*" + why):
            e.closed_loop_jvp_device(tape=e.closed_loop_tape(K), tx0=z(2, 1, 10), **tt)
        e.synchronize()
        assert (_np(tt["dxs"]) == -7.0).all() and (_np(tt["dus"]) == -7.0).all()
        e.close()
    eng.synchronize()
    torch.cuda.synchronize()
    for x, y in zip(_state(eng), before):
        assert np.array_equal(x, y, equal_nan=True)
    eng.close()
    assert (_np(dxs) == -7.0).all() and (_np(dus) == -7.0).all() and (_np(dXs) == -7.0).all()
    assert np.array_equal(_np(t["tape"]), r["tape_after"])


# ---- 9. another model
def test_tangents_at_the_loop_model(ndp, oracle, shared):
    """N = 20 at tests/plant_side_cases.py's LOOP_CASE (distinct weights, mass 0.9, the asymmetric box, g 7.0): dxs, dus, dXs against
    closed_loop_chain_ref.forward with the systems at that model, per referenced vehicle within max(BAR["ext"], 10 x that vehicle's own
    forward / reverse duality gap of the float64 reference) -- one ill-conditioned vehicle's reference sweeps disagree with each other
    beyond the flat bar.  A default handle given set_model(Qd, Rd, mass) before its warm-up step gives the created
    handle's bits."""
    N = 20
    a, cpu, cpu_ok, which, ups = C.loop_record(oracle, N)
    cfg, kw = C.loop_cfg(oracle, N), MC.engine_kw(MC.LOOP_CASE)
    eng = _engine(ndp, a, N, **kw)
    assert (eng.cfg.mass, eng.cfg.gravity) == (0.9, 7.0)
    rec = _loop(eng, a, C.LOOP_K, R.SUBSTEPS)
    eng.close()
    assert R.set_finish(rec)[which].all()
    tan = J.directions(C.LOOP_K, C.B, N, 2)
    eng = _engine(ndp, a, N, **kw)
    t, v = _forward(eng, a, N, ticks=C.LOOP_K)
    jv = _jvp(eng, t, N, tan)
    eng.close()
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(jv["status_check"], rec["st"])
    sys_ = R.systems(oracle, rec, which, cfg=cfg)
    ref = J.reference(sys_, rec, tan)
    gap = J.reference_gap(sys_, rec, tan, ups)
    worst = 0.0
    for j, vh in enumerate(which):
        e = J.errors(tuple(jv[n][:, [vh]] for n in ("dxs", "dus", "dXs")), tuple(x[:, [j]] for x in ref))
        bar = max(BAR["ext"], 10.0 * gap[j])
        print(f"vehicle {vh}: measured " + " ".join(f"{n} {x:.3e}" for n, x in e.items()) + f"; the reference's own gap {gap[j]:.2e}, bar {bar:.2e}")
        worst = max(worst, max(e.values()) / bar)
    assert worst <= 1.0
    q, rd, m = MC.model_of(MC.LOOP_CASE)[:3]
    eng = _engine(ndp, a, N, moved=(q, rd, m), **MC.engine_kw({k: x for k, x in MC.LOOP_CASE.items() if k not in ("Qd", "Rd", "mass")}))
    t2, v2 = _forward(eng, a, N, ticks=C.LOOP_K)
    jv2 = _jvp(eng, t2, N, tan)
    eng.close()
    _same(jv2, jv, OUTS + ("status_check",))


# ---- 10. torch
@pytest.mark.parametrize("N", HORIZONS)
def test_torch_closed_loop_jvp_gives_the_direct_calls_bits(ndp, oracle, shared, N):
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    r = jfull(ndp, oracle, N, shared)
    a, tan = r["a"], r["tan"]
    eng = _engine(ndp, a, N)
    out = TL.closed_loop_jvp(eng, _t(a["x0"]), _t(a["xr"]), _t(a["ur"]), tuple(_t(tan[n]) for n in J.NAMES), f=_t(a["f"], torch.float32),
                             fp=_t(a["fp"]))
    one = TL.closed_loop_jvp(eng, _t(a["x0"]), _t(a["xr"]), _t(a["ur"]), (None, None, None, None, _t(tan["tfp"][:, :, 0])), f=_t(a["f"], torch.float32),
                             fp=_t(a["fp"]))
    torch.cuda.synchronize()
    eng.close()
    for got, want in zip(out, (r["vals"]["xs"], r["vals"]["us"], r["vals"]["Xs"], r["jv"]["dxs"], r["jv"]["dus"], r["jv"]["dXs"])):
        assert np.array_equal(_np(got), want, equal_nan=True)
    assert tuple(one[3].shape) == (K, B, 10) and tuple(one[4].shape) == (K, B, 4) and tuple(one[5].shape) == (K, B, N + 1, 10)
