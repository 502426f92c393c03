"""Forward mode of the closed loop along directions of the cost weights and the mass on the device (run with -m gpu):
ndp_closed_loop_jvp_model_device against the forward sweep of tests/model_jvp_ref.py (closed_loop_chain_ref.forward's recursion with the
model's source term at every tick and the plant's mass share in the link), in duality with ndp_closed_loop_vjp_device's d_gmodel and
with the reference's model_reverse, and end to end: Levenberg-Marquardt on the cost weights with the Jacobian from the call.
CPU side: tests/test_step_model_jvp.py.

Inputs: tests/test_closed_loop_vjp_gpu.py's (`full`: ext_inputs(65, 3, N, 20231516), its record, forward, reverse call and reference
systems, once per horizon), N in closed_loop_jvp_cases.HORIZONS = (20, 7), K = 3 ticks, T = 3 directions with the force on the plant
given, so that column 15 acts: direction 0 and 1 carry model and data directions together, direction 2 is the plant's mass alone.

Bars, none of them from what the code under test gives:
  tangents      BAR["ext"] of tests/test_closed_loop_chain_gpu.py by rel_err with lead 3, as tests/test_closed_loop_jvp_gpu.py holds the
                data directions; the plant link PLANT_BAR against the complex-step Jacobian
  duality       against the device's d_gmodel: K x 1e-10 of the largest term; against the reference's model_reverse:
                sum_j |theta'_j| x the per-column bar tests/test_closed_loop_vjp_gpu.py holds gmodel to (its _model_errors: K x STEP_BAR
                max(1, |g|max) per tick for columns 0..14, BAR["ext"] max(1, |gfp|max) sum_k |fp_k|_1 / m for column 15)
  other model   per vehicle max(BAR["ext"], 10 x the float64 reference's own forward / reverse duality gap along the same directions)"""
import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import closed_loop_jvp_cases as J
from tests import closed_loop_vjp_ref as CV
from tests import model_cases as MC
from tests import model_jvp_ref as MR
from tests import plant_deriv_ref as P
from tests import plant_side_cases as C
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.fixed_set_ref import scale
from tests.test_closed_loop_chain_gpu import BAR, PLANT_BAR, STEP_BAR
from tests.test_closed_loop_vjp_gpu import GUARD, _engine, _forward, _guarded, _loop, _np, _reverse, _state, full

pytestmark = pytest.mark.gpu

K, B, T = J.K, J.B, 3
HORIZONS = list(J.HORIZONS)
OUTS = ("dxs", "dus", "dXs", "dUs")
WHO = "ndp_closed_loop_jvp_model_device"


def directions(ticks, n, N, seed=43):
    """(the data directions of closed_loop_jvp_cases.directions with T = 3, tmodel [n,3,16]): direction 2 is column 15 alone."""
    tan = J.directions(ticks, n, N, T)
    tm = np.random.default_rng(seed).normal(size=(n, T, 16))
    tm[:, 2, :15] = 0.0
    for name, v in tan.items():
        if name == "tx0":
            v[:, 2] = 0.0
        else:
            v[:, :, 2] = 0.0
    return tan, tm


def _mjvp(eng, t, N, tan, tm, stream=None):
    """closed_loop_jvp_device with tmodel into guarded, -7.0-filled outputs on the record t (_forward's); tan: {tx0, txr, tur, tf, tfp}
    numpy arrays or None (the whole dict None: the model direction alone).  Returns {name: numpy} of dxs, dus, dXs, dUs, status_check."""
    import torch
    ticks, n, nt = t["xr"].shape[0], t["x0"].shape[0], tm.shape[1]
    shapes = dict(dxs=(ticks, n, nt, 10), dus=(ticks, n, nt, 4), dXs=(ticks, n, nt, N + 1, 10), dUs=(ticks, n, nt, N, 4))
    o = {k: _guarded(*s) for k, s in shapes.items()}
    st = _guarded(ticks, n, dtype=torch.int32, fill=-7)
    d = {} if tan is None else {name: None if v is None else _t(v if name == "tx0" else v[:ticks]) for name, v in tan.items()}
    torch.cuda.synchronize()
    eng.closed_loop_jvp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["tape"], o["dxs"][0], o["dus"][0], f=t["f"], fp=t["fp"],
                               dXs=o["dXs"][0], dUs=o["dUs"][0], status_check=st[0].view(ticks, n), dt=t.get("dt", R.DT),
                               substeps=t["substeps"], stream=stream, tmodel=_t(tm), n_tan=nt, **d)
    eng.synchronize()
    torch.cuda.synchronize()
    for k, v in list(o.items()) + [("status_check", st)]:
        assert (_np(v[1])[-GUARD:] == -7).all(), k
    out = {k: _np(v[0]) for k, v in o.items()}
    out["status_check"] = _np(st[0]).reshape(ticks, n)
    return out


def _same(a, b, names=OUTS):
    for n in names:
        assert np.array_equal(a[n], b[n], equal_nan=True), n


@pytest.fixture(scope="module")
def shared():
    cache = {}
    yield cache
    for r in cache.values():
        r["eng"].close()


def mfull(ndp, oracle, N, cache):
    """tests/test_closed_loop_vjp_gpu.py's `full` of one horizon plus ONE model forward-mode run along the T = 3 directions and the float64
    forward sweep with the model columns on the device's record: computed once and left unchanged."""
    r = full(ndp, oracle, N, cache)
    if "mj" not in r:
        r["tan"], r["tm"] = directions(K, B, N)
        r["mj"] = _mjvp(r["eng"], r["t"], N, r["tan"], r["tm"])
        r["after_mjvp"], r["tape_after_mjvp"] = _state(r["eng"]), _np(r["t"]["tape"])
        if "sys" in r:
            cfg = R.twin_cfg(oracle, N)
            MR.loop_model_systems(oracle, r["sys"], r["rec"], cfg)
            t = r["tan"]
            r["mref"] = MR.loop_forward(r["sys"], r["rec"], r["tm"], t["tx0"], t["txr"], t["tur"], t["tfp"], t["tf"])
    return r


def _lhs(fwd, ups):
    dx, du, dX = fwd
    G, H, A = ups
    return np.einsum("kvtc,kvc->vt", dx, G) + np.einsum("kvtc,kvc->vt", du, H) + np.einsum("kvtnc,kvnc->vt", dX, A)


def _data_terms(t, g):
    return [np.einsum("vtc,vc->vt", t["tx0"], g["gx0"]), np.einsum("kvtnc,kvnc->vt", t["txr"], g["gxr"]),
            np.einsum("kvtnc,kvnc->vt", t["tur"], g["gur"]), np.einsum("kvtnc,kvnc->vt", t["tf"], g["gf"]),
            np.einsum("kvtc,kvc->vt", t["tfp"], g["gfp"])]


# ---- 1. against the float64 reference
@pytest.mark.parametrize("N", HORIZONS)
def test_tangents_match_the_forward_sweep_with_the_model_columns(ndp, oracle, shared, N):
    r = mfull(ndp, oracle, N, shared)
    mj = r["mj"]
    assert r["ok"][r["which"]].all() and np.array_equal(mj["status_check"], r["vals"]["status"])
    e = J.errors((mj["dxs"], mj["dus"], mj["dXs"]), r["mref"], r["which"])
    print(f"N={N}: model forward mode against the forward sweep, measured " + " ".join(f"{n} {v:.3e}" for n, v in e.items())
          + f"; bar {BAR['ext']:.2e}")
    assert np.isfinite(mj["dxs"][:, r["ok"]]).all() and np.abs(mj["dxs"][:, r["which"]]).max() > 1e-3
    assert max(e.values()) <= BAR["ext"], e
    # dUs[k][.][.][0] is dus[k]; the engine and the tape keep their bits
    assert np.array_equal(mj["dUs"][:, r["ok"]][:, :, :, 0], mj["dus"][:, r["ok"]])
    for x, y in zip(r["after_mjvp"], r["after_fwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(r["tape_after_mjvp"], r["tape_after"])


@pytest.mark.parametrize("N", HORIZONS)
def test_the_plant_link_sees_the_mass_through_the_force(ndp, oracle, shared, N):
    """dxs[k] against the plant's complex-step Jacobian at (x_k, u0_k, fp_k) applied to the call's own (dxs[k-1], dus[k]) and
    tfp[k] - (tmodel[15] / m) fp_k, within PLANT_BAR; direction 2 (column 15 alone) moves the states and leaves tick 0's dus exactly 0."""
    r = mfull(ndp, oracle, N, shared)
    eng, t, mj, tan, tm, ok = r["eng"], r["t"], r["mj"], r["tan"], r["tm"], (r["vals"]["status"] == 0).all(axis=0)
    xs, us, fp = _np(t["xs"]), _np(t["us"]), _np(t["fp"])
    m, worst = float(eng.cfg.mass), 0.0
    for k in range(K):
        xk = _np(t["x0"]) if k == 0 else xs[k - 1]
        txk = tan["tx0"] if k == 0 else mj["dxs"][k - 1]
        Jk = P.jacobian(xk[ok], us[k][ok][None], fp[k][ok][None], R.DT, R.SUBSTEPS, m, float(eng.cfg.gravity))
        tfp = tan["tfp"][k] - tm[:, :, 15:16] / m * fp[k][:, None, :]
        ref = P.jvp(Jk, tx0=txk[ok], tu=mj["dus"][k][ok][None], tf=tfp[ok][None])[0]
        good, ratio = P.within_bar(mj["dxs"][k][ok], ref, PLANT_BAR)
        worst = max(worst, ratio)
    print(f"N={N}: plant link with the mass share against the complex-step Jacobian, worst {worst:.3e} (bar {PLANT_BAR:.0e})")
    assert worst <= PLANT_BAR
    assert not mj["dus"][0][ok][:, 2].any() and not mj["dXs"][0][ok][:, 2].any()
    assert np.abs(mj["dxs"][0][ok][:, 2]).max() > 1e-6
    assert np.abs(mj["dus"][1:][:, ok][:, :, 2]).max() > 1e-9         # (the moved state reaches the later ticks' steps)


# ---- 2. duality
@pytest.mark.parametrize("N", HORIZONS)
def test_duality_with_the_reverse_calls_model_gradient(ndp, oracle, shared, N):
    """<G, dxs> + <H, dus> + <A, dXs> = the data terms + <gmodel[v], tmodel[v]> (all 16 columns) against ndp_closed_loop_vjp_device on the
    same record, per vehicle and direction over all set finishes: the gap over the largest term within K x 1e-10."""
    r = mfull(ndp, oracle, N, shared)
    mj, g, tm = r["mj"], r["grads"], r["tm"]
    lhs = _lhs((mj["dxs"], mj["dus"], mj["dXs"]), r["ups"])
    terms = _data_terms(r["tan"], g) + [g["gmodel"][:, None, j] * tm[:, :, j] for j in range(16)]
    big = np.maximum(np.abs(np.array(terms)).max(axis=0), np.abs(lhs))
    gap = (np.abs(lhs - np.sum(terms, axis=0)) / big)[r["ok"]]
    print(f"N={N}: duality with the reverse call's gmodel over {int(r['ok'].sum())} vehicles, worst gap {gap.max():.3e} of the largest term "
          f"(bar {K * 1e-10:.0e})")
    assert r["ok"].sum() >= B - B // 4 and gap.max() <= K * 1e-10


@pytest.mark.parametrize("N", HORIZONS)
def test_duality_with_the_references_model_reverse(ndp, oracle, shared, N):
    """The model direction alone, every data direction NULL (a run of its own): <G, dxs> + <H, dus> + <A, dXs> of the device against sum_j model_reverse[v][j] theta'_j of the float64 reference on the referenced
    vehicles, within sum_j |theta'_j| x the bar of column j (the module docstring)."""
    r = mfull(ndp, oracle, N, shared)
    which, tm, rec, sys_ = r["which"], r["tm"], r["rec"], r["sys"]
    alone = _mjvp(r["eng"], r["t"], N, None, tm)
    lhs = _lhs((alone["dxs"], alone["dus"], alone["dXs"]), r["ups"])[which]
    tot, per = CV.model_reverse(oracle, sys_, rec, *r["ups"])
    _, gfp = CV.sweep_upstreams(sys_, rec, *r["ups"])
    mass = oracle.default_cfg(N=N, use_fd=True).mass
    worst = 0.0
    for j, v in enumerate(which):
        bar14 = sum(STEP_BAR * scale(per[k, j, :15]) for k in range(K))
        bar15 = BAR["ext"] * scale(gfp[:, j]) * float(np.abs(rec["fp"][:, v]).sum()) / mass
        for d in range(T):
            bar = np.abs(tm[v, d, :15]).sum() * bar14 + abs(tm[v, d, 15]) * bar15
            err = abs(lhs[j, d] - tot[j] @ tm[v, d])
            worst = max(worst, err / bar)
            assert err <= bar, (v, d, err, bar)
    print(f"N={N}: duality with the reference's model_reverse, worst {worst:.3e} of its bar")


# ---- 3. directions, substeps, a NaN vehicle
@pytest.mark.parametrize("N", HORIZONS)
def test_t_directions_in_one_call_are_t_calls_of_one_and_two_calls_agree(ndp, oracle, shared, N):
    r = mfull(ndp, oracle, N, shared)
    eng, t, tan, tm = r["eng"], r["t"], r["tan"], r["tm"]
    again = _mjvp(eng, t, N, tan, tm)
    _same(again, r["mj"], OUTS + ("status_check",))
    for d in range(T):
        one = _mjvp(eng, t, N, {n: np.ascontiguousarray(v[:, d:d + 1] if n == "tx0" else v[:, :, d:d + 1]) for n, v in tan.items()},
                    np.ascontiguousarray(tm[:, d:d + 1]))
        for n in OUTS:
            assert np.array_equal(one[n][:, :, 0], r["mj"][n][:, :, d], equal_nan=True), (n, d)


def test_substeps_1_against_the_forward_sweep_and_the_reverse_call(ndp, oracle, shared):
    """N = 7, K = 3 with one RK4 substep per tick: the tangents of the referenced vehicles against the forward sweep at that substep count
    (BAR["ext"]), and duality with the reverse call's gmodel (K x 1e-10)."""
    N, sub = 7, 1
    r0 = mfull(ndp, oracle, N, shared)
    a, which, tan, tm = r0["a"], r0["which"], r0["tan"], r0["tm"]
    eng = _engine(ndp, a, N)
    rec = _loop(eng, a, K, sub)
    eng.close()
    eng = _engine(ndp, a, N)
    t, v = _forward(eng, a, N, substeps=sub)
    mj = _mjvp(eng, t, N, tan, tm)
    g = _reverse(eng, t, N, r0["ups"])
    eng.close()
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and R.set_finish(rec)[which].all()
    sys_ = MR.loop_model_systems(oracle, R.systems(oracle, rec, which, substeps=sub), rec, R.twin_cfg(oracle, N))
    ref = MR.loop_forward(sys_, rec, tm, tan["tx0"], tan["txr"], tan["tur"], tan["tfp"], tan["tf"])
    e = J.errors((mj["dxs"], mj["dus"], mj["dXs"]), ref, which)
    ok = (v["status"] == 0).all(axis=0)
    lhs = _lhs((mj["dxs"], mj["dus"], mj["dXs"]), r0["ups"])
    terms = _data_terms(tan, g) + [g["gmodel"][:, None, j] * tm[:, :, j] for j in range(16)]
    gap = (np.abs(lhs - np.sum(terms, axis=0)) / np.maximum(np.abs(np.array(terms)).max(axis=0), np.abs(lhs)))[ok]
    print("substeps 1: measured " + " ".join(f"{n} {x:.3e}" for n, x in e.items()) + f" (bar {BAR['ext']:.2e}); duality gap {gap.max():.3e}")
    assert max(e.values()) <= BAR["ext"] and gap.max() <= K * 1e-10


def test_a_nan_vehicle_stays_with_itself(ndp, oracle, shared):
    """N = 20, vehicle 1 given a NaN velocity in x_0: its dxs and dus are NaN at every tick and in every direction, every other vehicle's
    outputs are bit-equal to the clean run's."""
    N, bad = 20, 1
    r = mfull(ndp, oracle, N, shared)
    a = dict(r["a"], x0=r["a"]["x0"].copy())
    a["x0"][bad, 3] = np.nan
    eng = _engine(ndp, a, N)
    t, v = _forward(eng, a, N)
    mj = _mjvp(eng, t, N, r["tan"], r["tm"])
    eng.close()
    rest = np.arange(B) != bad
    assert (v["status"][:, bad] != 0).all() and np.array_equal(mj["status_check"], v["status"])
    assert np.isnan(mj["dxs"][:, bad]).all() and np.isnan(mj["dus"][:, bad]).all()
    for n in OUTS:
        assert np.array_equal(mj[n][:, rest], r["mj"][n][:, rest], equal_nan=True), n


# ---- 4. another model
def test_tangents_at_the_loop_model(ndp, oracle):
    """N = 7 at model_cases.LOOP_CASE (distinct weights, mass 0.9, the asymmetric box, g 7.0), so that a default mass or a default weight
    in the new code shows: dxs, dus, dXs against the forward sweep with the systems and model columns at that model, per referenced
    vehicle within max(BAR["ext"], 10 x the float64 reference's own forward / reverse duality gap along the same model directions)."""
    N = 7
    a, cpu, cpu_ok, which, ups = C.loop_record(oracle, N)
    cfg, kw = C.loop_cfg(oracle, N), MC.engine_kw(MC.LOOP_CASE)
    eng = _engine(ndp, a, N, **kw)
    assert (eng.cfg.mass, eng.cfg.gravity) == (0.9, 7.0)
    rec = _loop(eng, a, C.LOOP_K, R.SUBSTEPS)
    eng.close()
    assert R.set_finish(rec)[which].all()
    tan, tm = directions(C.LOOP_K, C.B, N)
    eng = _engine(ndp, a, N, **kw)
    t, v = _forward(eng, a, N, ticks=C.LOOP_K)
    mj = _mjvp(eng, t, N, tan, tm)
    eng.close()
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(mj["status_check"], rec["st"])
    sys_ = MR.loop_model_systems(oracle, R.systems(oracle, rec, which, cfg=cfg), rec, cfg)
    ref = MR.loop_forward(sys_, rec, tm, tan["tx0"], tan["txr"], tan["tur"], tan["tfp"], tan["tf"])
    only = MR.loop_forward(sys_, rec, tm)
    tot, _ = CV.model_reverse(oracle, sys_, rec, *ups, cfg=cfg)
    own = np.abs(_lhs(only, tuple(u[:, which] for u in ups)) - np.einsum("vj,vtj->vt", tot, tm[which])).max(axis=1)
    worst = 0.0
    for j, vh in enumerate(which):
        e = J.errors(tuple(mj[n][:, [vh]] for n in ("dxs", "dus", "dXs")), tuple(x[:, [j]] for x in ref))
        bar = max(BAR["ext"], 10.0 * own[j])
        print(f"vehicle {vh}: measured " + " ".join(f"{n} {x:.3e}" for n, x in e.items()) + f"; the reference's own gap {own[j]:.2e}, bar {bar:.2e}")
        worst = max(worst, max(e.values()) / bar)
    assert worst <= 1.0


# ---- 5. torch
def test_torch_closed_loop_jvp_gives_the_direct_calls_bits(ndp, oracle, shared):
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    N = 7
    r = mfull(ndp, oracle, N, shared)
    a, tan, tm = r["a"], r["tan"], r["tm"]
    eng = _engine(ndp, a, N)
    out = TL.closed_loop_jvp(eng, _t(a["x0"]), _t(a["xr"]), _t(a["ur"]), tuple(_t(tan[n]) for n in J.NAMES), f=_t(a["f"], torch.float32),
                             fp=_t(a["fp"]), tmodel=_t(tm))
    torch.cuda.synchronize()
    eng.close()
    for got, want in zip(out, (r["vals"]["xs"], r["vals"]["us"], r["vals"]["Xs"], r["mj"]["dxs"], r["mj"]["dus"], r["mj"]["dXs"])):
        assert np.array_equal(_np(got), want, equal_nan=True)
    eng = _engine(ndp, a, N)
    one = TL.closed_loop_jvp(eng, _t(a["x0"]), _t(a["xr"]), _t(a["ur"]), (None,) * 5, f=_t(a["f"], torch.float32), fp=_t(a["fp"]),
                             tmodel=TL.model_tangent(tmass=1.0).to(_dev()))
    torch.cuda.synchronize()
    eng.close()
    assert tuple(one[3].shape) == (K, B, 10) and tuple(one[4].shape) == (K, B, 4) and tuple(one[5].shape) == (K, B, N + 1, 10)
    assert torch.isfinite(one[3][:, r["ok"]]).all() and one[3].abs().max() > 0


# ---- 6. refusals
def test_refusals_name_the_call_and_enqueue_nothing(ndp, oracle, shared):
    import ctypes as Ct
    import torch
    N = 7
    r = mfull(ndp, oracle, N, shared)
    t = r["t"]
    eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    dxs, dus = z(K, B, 2, 10), z(K, B, 2, 4)
    call = lambda **kw: eng.closed_loop_jvp_device(**{**dict(x0=t["x0"], xr=t["xr"], ur=t["ur"], xs=t["xs"], us=t["us"], tape=t["tape"],  # noqa: E731
                                                             dxs=dxs, dus=dus, f=t["f"], fp=t["fp"], tmodel=z(B, 2, 16), n_tan=2), **kw})
    for kw, why in ((dict(substeps=0), "substeps"), (dict(tape=None), "d_tape"), (dict(dxs=None), "d_dxs"),
                    (dict(n_tan=9, tmodel=z(B, 9, 16), dxs=z(K, B, 9, 10), dus=z(K, B, 9, 4)), "n_tan")):
        with pytest.raises(ndp.NdpError, match=WHO + r" failed \(-2\): " + WHO + ".*" + why):
            call(**kw)
    with pytest.raises(ndp.NdpError, match=WHO + r" failed \(-1\)"):
        call(x0=None)
    # d_tmodel NULL at the C entry: the binding routes on tmodel
    p = Ct.c_void_p(dxs.data_ptr())
    args = [K, R.DT, 4] + [p] * 8 + [2] + [None] * 5 + [None] + [p, p, None, None, None, None]
    assert eng._lib.ndp_closed_loop_jvp_model_device(eng._h, *args) == -2
    assert b"without it: ndp_closed_loop_jvp_device" in eng._lib.ndp_last_error(eng._h)
    eng.synchronize()
    torch.cuda.synchronize()
    eng.close()
    assert (_np(dxs) == -7.0).all() and (_np(dus) == -7.0).all()
    assert np.array_equal(_np(t["tape"]), r["tape_after"])


# ---- 7. end to end: Levenberg-Marquardt on the cost weights
def test_levenberg_marquardt_on_the_cost_weights_with_the_jacobian_from_the_call(ndp):
    """B = 64, 3 ticks.  Targets xs* from an engine with Qd*; start from a perturbed Qd; three Levenberg-Marquardt steps on the residuals
    xs - xs* with the Jacobian in the nine weighted entries of Qd from two forward calls (8 + 1 directions), the damping doubled from
    lambda = 1e-3 max diag(J'J) until the loss decreases (at most 30 doublings, the cap of
    test_training_the_cost_weights_by_gradient_descent_with_a_line_search): every step is accepted within the cap and lowers the loss.  No
    rate or final loss is asserted: a wrong sign or scale of the Jacobian fails the search."""
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    n, N, ticks = 64, 20, 3
    a = R.ext_inputs(n, ticks, N, 20231516)
    eng = _engine(ndp, a, N)
    X0, U0 = eng.get_iterate()
    A0 = eng.active_set()[1]
    Qs = np.array(list(eng.cfg.Qd))
    x0, xr, ur, f, fp = _t(a["x0"]), _t(a["xr"]), _t(a["ur"]), _t(a["f"], torch.float32), _t(a["fp"])
    cols = [j for j in range(10) if j != 6]
    eye = torch.eye(16, dtype=torch.float64, device=_dev())

    def run(q, jac):
        """(xs [ticks,n,10], J [ticks,n,10,9] or None) at the weights q, from the same iterate and kept sets."""
        eng.set_model(Qd=q)
        Js = []
        for group in ((cols[:8], cols[8:]) if jac else ()):
            eng.set_iterate(X0, U0)
            eng.set_active_set(A0)
            out = TL.closed_loop_jvp(eng, x0, xr, ur, (None,) * 5, f=f, fp=fp, tmodel=eye[group])
            Js.append(out[3])
        if not jac:
            eng.set_iterate(X0, U0)
            eng.set_active_set(A0)
            xs = torch.empty(ticks, n, 10, dtype=torch.float64, device=_dev())
            us = torch.empty(ticks, n, 4, dtype=torch.float64, device=_dev())
            eng.closed_loop_device(x0, xr, ur, xs, us, f=f, fp=fp)
            eng.synchronize()
            return xs.cpu().numpy(), None
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), torch.cat(Js, dim=2).permute(0, 1, 3, 2).cpu().numpy()

    xs_star, _ = run(Qs, False)
    ok_star = np.isfinite(xs_star).all(axis=(0, 2))
    q = Qs * np.where(np.arange(10) == 6, 1.0, np.random.default_rng(32).uniform(0.4, 2.5, 10))
    losses = []
    for step in range(3):
        xs, Jm = run(q, True)
        ok = ok_star & np.isfinite(xs).all(axis=(0, 2)) & np.isfinite(Jm).all(axis=(0, 2, 3))
        res = (xs - xs_star)[:, ok].reshape(-1)
        Jf = Jm[:, ok].reshape(-1, len(cols))
        loss = float(res @ res)
        JtJ, g = Jf.T @ Jf, Jf.T @ res
        lam = 1e-3 * float(np.diag(JtJ).max())
        for doublings in range(31):
            cand = q.copy()
            cand[cols] -= np.linalg.solve(JtJ + lam * np.eye(len(cols)), g)
            if (cand >= 0).all():
                xs_c, _ = run(cand, False)
                ok_c = ok & np.isfinite(xs_c).all(axis=(0, 2))
                new = float(((xs_c - xs_star)[:, ok_c] ** 2).sum()) if ok_c.sum() == ok.sum() else np.inf
                if new < loss:
                    break
            lam *= 2.0
        else:
            raise AssertionError(f"step {step}: no decrease within 30 doublings (loss {loss:.6e})")
        losses.append((loss, new, doublings))
        q = cand
    eng.close()
    print("Levenberg-Marquardt on Qd (loss before, after, doublings):", [("%.4e" % x, "%.4e" % y, d) for x, y, d in losses])
    assert all(c < b for b, c, _ in losses) and losses[0][0] > 0
