"""The formation's closed loop in one call per direction on the device (run with -m gpu): ndp_closed_loop_formation_config,
ndp_plant_force_scatter_device, ndp_closed_loop_formation_device against the host loop of ndp_plant_force_multi_device, ndp_step_device and
ndp_plant_step_device, bit for bit, and ndp_closed_loop_formation_vjp_device against the float64 reverse sweep of
tests/closed_loop_formation_ref.py on the device's own record.  CPU side: tests/test_closed_loop_formation.py.

Inputs: closed_loop_formation_ref.inputs -- stacked triples (K = 2 slots), 3 ticks: B = 6 at N = 20 (every vehicle referenced; where g_w is
compared), B = 66 at N = 20 (22 triples; triple 0 and triple 21, vehicles 63..65 across the 64-lane workgroup boundary, are referenced) and
B = 6 at N = 7.  The conditions of tests/test_closed_loop_formation.py are asserted again on the device's record; no row is left out.

Bars, both imported from tests/test_closed_loop_chain_gpu.py and none from what the code under test gives (closed_loop_chain_ref.rel_err):
  BAR["ext"]  the leaves the force's adjoint cannot reach: the LAST tick's gxr, gur and gf
  BAR["ndp"]  everything else and g_w: the project's figure for the same fp32 network links composed over three ticks
MEASURED on the first device run (MI355X), the worst over b6 / b66 / n7 (test 3 prints every figure again; DESIGN section 9 has them):
  ext group  1.5e-14 (xr_last 1.5e-14, ur_last 1.5e-14, f_last 9.5e-15)          bar 1.2e-11
  ndp group  6.3e-07 (x0 6.3e-07, xr 1.9e-07, ur 1.5e-07, f 6.0e-08, w 4.0e-07)  bar 6.7e-06
  the one call against the torch chain: every leaf bit-equal but the weights, 8.3e-08"""
import ctypes as Ct

import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import closed_loop_formation_ref as C
from tests import mlp_vjp_ref as MV
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.test_closed_loop_chain_gpu import BAR
from tests.test_closed_loop_formation import referenced

pytestmark = pytest.mark.gpu

K, GUARD = C.K, 2
CASES = {"b6": (2, 20), "b66": (22, 20), "n7": (2, 7)}
OUTS = ("gx0", "gxr", "gur", "gf", "gw", "gmodel")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _engine(ndp, a, N, index="own", load_mlp=True, **kw):
    """A fresh engine: reset to tick 0's window, one warm-up step on tick 0's inputs (a kept set exists), the formation configured
    (index "own": the inputs'; None: not configured).  kw: ndp_cfg overrides (the model, r_horiz)."""
    import torch
    n = a["x0"].shape[0]
    eng = ndp.BatchedNMPC(n, N=N, disturbance=True, load_mlp=load_mlp, **kw)
    eng.reset(a["xr"][0], a["ur"][0])
    u0 = torch.empty(n, 4, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    eng.update_device(_t(a["x0"]), _t(a["xr"][0]), _t(a["ur"][0]), u0, f=_t(a["f"][0], torch.float32))
    eng.synchronize()
    if index is not None:
        eng.closed_loop_formation_config(a["index"] if isinstance(index, str) else index)
    return eng


def _state(eng):
    return [_np(v) for v in eng.device_iterate()] + [eng.active_set()[1]]


def _loop(eng, a, index, ticks=K, gate=True, scale=1.0, dt=R.DT, substeps=R.SUBSTEPS):
    """The host loop of the three existing calls -- plant_force_multi_device, update_device, ndp_plant_step_device -- and its record
    (closed_loop_formation_ref's layout: fp = the forces the device made)."""
    import torch
    n = a["x0"].shape[0]
    x, idx = _t(a["x0"]), _t(np.ascontiguousarray(index, dtype=np.int32))
    rec = {k: [] for k in ("x", "force", "Xpre", "Upre", "act_pre", "act", "u0", "X", "st", "it", "fp")}
    for k in range(ticks):
        tape = eng.record_tape()
        fp, u0 = torch.empty(n, 3, dtype=torch.float64, device=_dev()), torch.empty(n, 4, dtype=torch.float64, device=_dev())
        torch.cuda.synchronize()
        eng.plant_force_multi_device(x, idx, fp, gate=gate, scale=scale)
        eng.update_device(x, _t(a["xr"][k]), _t(a["ur"][k]), u0, f=_t(a["f"][k], torch.float32))
        eng.synchronize()
        X = eng.device_iterate()[0].clone()
        xn = x.clone()
        torch.cuda.synchronize()
        st, it = eng.status()
        eng._check(eng._lib.ndp_plant_step_device(eng._h, Ct.c_void_p(xn.data_ptr()), Ct.c_void_p(u0.data_ptr()), Ct.c_void_p(fp.data_ptr()),
                                                  float(dt), int(substeps), None), "ndp_plant_step_device")
        eng.synchronize()
        for name, v in (("x", _np(x)), ("force", a["f"][k].astype(np.float64)), ("Xpre", _np(tape[0])), ("Upre", _np(tape[1])),
                        ("act_pre", _np(tape[2])), ("act", eng.active_set()[1]), ("u0", _np(u0)), ("X", _np(X)), ("st", st), ("it", it),
                        ("fp", _np(fp))):
            rec[name].append(v)
        x = xn
    rec["x"].append(_np(x))
    rec = {k: np.stack(v) for k, v in rec.items()}
    rec.update(xr=a["xr"][:ticks], ur=a["ur"][:ticks], other=None, idx=None, blob=a["blob"], index=np.asarray(index))
    return rec


def _guarded(*shape, dtype=None, fill=-7.0):
    """(the array, the whole buffer): a contiguous array of `shape` with GUARD rows behind it."""
    import torch
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else shape[0]
    last = shape[-1] if len(shape) > 1 else 1
    whole = torch.full((rows + GUARD, last), fill, dtype=dtype or torch.float64, device=_dev())
    return whole[:rows].view(*shape), whole


def _forward(eng, a, N, ticks=K, optional=True, stream=None, gate=True, scale=1.0, dt=R.DT, substeps=R.SUBSTEPS):
    """closed_loop_formation_device into guarded outputs; optional False: d_Xs, d_status and d_tape NULL."""
    import torch
    n = a["x0"].shape[0]
    t = dict(x0=_t(a["x0"]), xr=_t(a["xr"][:ticks]), ur=_t(a["ur"][:ticks]), f=_t(a["f"][:ticks], torch.float32))
    o = dict(xs=_guarded(ticks, n, 10), us=_guarded(ticks, n, 4), fps=_guarded(ticks, n, 3))
    if optional:
        o.update(Xs=_guarded(ticks, n, N + 1, 10), status=_guarded(ticks, n, dtype=torch.int32, fill=-7))
    tape = eng.closed_loop_tape(ticks) if optional else None
    torch.cuda.synchronize()
    eng.closed_loop_formation_device(t["x0"], t["xr"], t["ur"], o["xs"][0], o["us"][0], o["fps"][0], f=t["f"],
                                     Xs=o["Xs"][0] if optional else None, status=o["status"][0].view(ticks, n) if optional else None,
                                     tape=tape, gate=gate, plant_scale=scale, dt=dt, substeps=substeps, stream=stream)
    eng.synchronize()
    torch.cuda.synchronize()
    t.update(xs=o["xs"][0], us=o["us"][0], fps=o["fps"][0], tape=tape, gate=gate, scale=scale, dt=dt, substeps=substeps)
    vals = {k: _np(v[0]) for k, v in o.items()}
    if optional:
        vals["status"] = vals["status"].reshape(ticks, n)
    for k, v in o.items():
        assert (_np(v[1])[-GUARD:] == -7).all(), k
    return t, vals


def _reverse(eng, t, N, ups, ask=OUTS, stream=None):
    """closed_loop_formation_vjp_device into guarded, -7-filled outputs; ups = (gxs, gus, gXs, gfps), each an array or None."""
    import torch
    ticks, n = t["xr"].shape[0], t["x0"].shape[0]
    shapes = dict(gx0=(n, 10), gxr=(ticks, n, N + 1, 10), gur=(ticks, n, N, 4), gf=(ticks, n, N + 1, 3), gw=(MV.mlp_frag.NPARAM,), gmodel=(n, 16))
    o = {k: _guarded(*shapes[k], dtype=torch.float32 if k == "gw" else None) for k in ask}
    st = _guarded(ticks, n, dtype=torch.int32, fill=-7)
    g = [None if u is None else _t(u[:ticks]) for u in ups]
    torch.cuda.synchronize()
    eng.closed_loop_formation_vjp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["fps"], t["tape"], f=t["f"], gxs=g[0], gus=g[1],
                                         gXs=g[2], gfps=g[3], status_check=st[0].view(ticks, n), gate=t["gate"], plant_scale=t["scale"],
                                         dt=t["dt"], substeps=t["substeps"], stream=stream, **{k: v[0] for k, v in o.items()})
    eng.synchronize()
    torch.cuda.synchronize()
    for k, v in list(o.items()) + [("status_check", st)]:
        assert (_np(v[1])[-GUARD:] == -7).all(), k
    out = {k: _np(v[0]) for k, v in o.items()}
    out["status_check"] = _np(st[0]).reshape(ticks, n)
    return out


def _ups(n, N, seed=31, ticks=K):
    G, H, A = R.upstreams(ticks, n, N, seed=seed)
    return G, H, A, np.random.default_rng(seed + 1).normal(size=(ticks, n, 3))


@pytest.fixture(scope="module")
def shared():
    cache = {}
    yield cache
    for r in cache.values():
        r["eng"].close()


def full(ndp, oracle, name, cache):
    """Everything the tests of one case share, computed once and left unchanged: the inputs, the device's record from the host loop, ONE
    run of the one call and of its reverse call with every output, and the reference sweep on the device's record."""
    if name in cache:
        return cache[name]
    triples, N = CASES[name]
    a = C.inputs(triples, N)
    n = a["x0"].shape[0]
    which = referenced(triples)
    eng = _engine(ndp, a, N, index=None)
    rec = _loop(eng, a, a["index"])
    after_loop = _state(eng)
    eng.close()
    eng = _engine(ndp, a, N)
    t, vals = _forward(eng, a, N)
    after_fwd = _state(eng)
    ups = _ups(n, N)
    grads = _reverse(eng, t, N, ups)
    r = dict(a=a, n=n, N=N, which=which, rec=rec, ok=R.set_finish(rec), after_loop=after_loop, eng=eng, t=t, vals=vals, after_fwd=after_fwd,
             ups=ups, grads=grads, after_bwd=_state(eng), tape_after=_np(t["tape"]))
    if r["ok"][which].all():
        r["sys"] = R.systems(oracle, rec, which)
        r["ref"] = C.reverse(r["sys"], rec, *ups)
    cache[name] = r
    return r


def _errors(g, ref, which, with_w):
    """{bar: {leaf: rel_err}}: the last tick's gxr, gur, gf under "ext", everything else (and g_w) under "ndp"; the ticks are the
    reference's (one tick: there are no earlier ticks' leaves)."""
    last = ref["xr"].shape[0] - 1
    ext = dict(xr_last=R.rel_err(g["gxr"][last][which], ref["xr"][last], 1), ur_last=R.rel_err(g["gur"][last][which], ref["ur"][last], 1),
               f_last=R.rel_err(g["gf"][last][which], ref["f"][last], 1))
    net = dict(x0=R.rel_err(g["gx0"][which], ref["x0"], 1))
    if last:
        net.update(xr=R.rel_err(g["gxr"][:last, which], ref["xr"][:last], 2), ur=R.rel_err(g["gur"][:last, which], ref["ur"][:last], 2),
                   f=R.rel_err(g["gf"][:last, which], ref["f"][:last], 2))
    if with_w:
        net["w"] = R.rel_err(g["gw"], ref["w"], 0)
    return dict(ext=ext, ndp=net)


# ---- 1. the scatter
def test_scatter_is_bit_equal_to_the_ordered_sums(ndp):
    """plant_force_scatter_device against numpy float64 sums formed in the stated order, bit for bit (signed zeros included), on the
    hand-made index at B = 65, K = 3 (a hub heard by all, a vehicle heard by none, self slots, -1 and >= B entries, the same index twice
    in one row) and at B = 1, K = 1 with an empty slot; columns 6..9 exactly 0; a sentinel row past B untouched."""
    import torch
    rng = np.random.default_rng(4)
    for n, Kn, idx in ((65, 3, C.hand_index(65, 3)), (1, 1, np.array([[-1]], dtype=np.int32))):
        eng = ndp.BatchedNMPC(n, N=7)
        eng.closed_loop_formation_config(idx)
        gz = rng.normal(size=(n, Kn, 6)) * 10.0 ** rng.integers(-8, 8, size=(n, Kn, 1))
        gz[0, 0] = -0.0
        gx, whole = _guarded(n, 10)
        torch.cuda.synchronize()
        eng.plant_force_scatter_device(_t(gz), gx)
        eng.synchronize()
        got, want = _np(gx), C.scatter_ordered(gz, idx)
        eng.close()
        assert np.array_equal(_bits(got[:, :6]), _bits(want[:, :6])), (n, np.abs(got - want).max())
        assert np.array_equal(_bits(got[:, 6:]), np.zeros((n, 4), dtype=np.int64))
        assert (_np(whole)[-GUARD:] == -7).all()
        if n == 65:
            assert np.abs(want[0, :6]).max() > 0 and np.array_equal(_bits(got[1, :6]), _bits(-gz[1, 0] - gz[1, 1]))   # heard by none: 0 - own


# ---- 2. the forward
@pytest.mark.parametrize("name", ["b6", "b66", "n7"])
def test_forward_is_the_host_loops_bits(ndp, oracle, shared, name):
    """xs, us, fps, Xs, the status words, the tape slots and the engine's iterate and kept set afterwards are bit-equal to the host loop of
    plant_force_multi_device, update_device and ndp_plant_step_device; with d_Xs, d_status and d_tape NULL the same xs, us, fps and state."""
    r = full(ndp, oracle, name, shared)
    rec, v, eng, a, N = r["rec"], r["vals"], r["eng"], r["a"], r["N"]
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(v["us"], rec["u0"], equal_nan=True)
    assert np.array_equal(_bits(v["fps"]), _bits(rec["fp"])) and np.abs(v["fps"][:, r["which"]]).max() > 1.0
    assert np.array_equal(v["Xs"], rec["X"], equal_nan=True) and np.array_equal(v["status"], rec["st"])
    for x, y in zip(r["after_fwd"], r["after_loop"]):
        assert np.array_equal(x, y, equal_nan=True)
    for k in range(K):
        X, U, A = (_np(s) for s in eng.closed_loop_tape_slot(r["t"]["tape"], k))
        assert np.array_equal(X, rec["Xpre"][k], equal_nan=True) and np.array_equal(U, rec["Upre"][k], equal_nan=True)
        assert np.array_equal(A, rec["act_pre"][k])
    assert np.array_equal(r["grads"]["status_check"], rec["st"])
    eng2 = _engine(ndp, a, N)
    t2, v2 = _forward(eng2, a, N, optional=False)
    for n_ in ("xs", "us", "fps"):
        assert np.array_equal(v2[n_], v[n_], equal_nan=True), n_
    for x, y in zip(_state(eng2), r["after_loop"]):
        assert np.array_equal(x, y, equal_nan=True)
    eng2.close()


def test_the_devices_record_meets_the_conditions(ndp, oracle, shared):
    """The conditions of tests/test_closed_loop_formation.py on the DEVICE's record, every case: open margins >= MARGIN, no failing slot,
    an open slot per referenced triple at every tick, every referenced vehicle a status-0 set finish."""
    for name in CASES:
        r = full(ndp, oracle, name, shared)
        c = C.conditions(r["rec"], r["which"])
        print(f"{name}: smallest open margin {c['margin']:.2e}; {int((~r['ok']).sum())} of {r['n']} vehicles are no set finishes")
        assert c["margin"] >= MV.MARGIN and c["failing"] == 0 and (c["open_per"] >= 1).all() and c["set_finish"].all(), (name, c)


# ---- 3. gradients against the reference
@pytest.mark.parametrize("name", ["b6", "b66", "n7"])
def test_gradients_match_the_reference_sweep(ndp, oracle, shared, name):
    """Every output of the reverse call on the device's record against closed_loop_formation_ref.reverse, by rel_err: the last tick's
    gxr, gur, gf at BAR["ext"]; gx0, the earlier ticks' gxr, gur, gf and (B = 6) g_w at BAR["ndp"].  The coupling is live: the reference
    without the scatter differs from the device by far more than the bar."""
    r = full(ndp, oracle, name, shared)
    e = _errors(r["grads"], r["ref"], r["which"], with_w=name != "b66")
    for bar, errs in e.items():
        print(f"{name}, held to BAR[{bar!r}] = {BAR[bar]:.1e}: measured " + " ".join(f"{n} {v:.3e}" for n, v in errs.items()))
    for bar, errs in e.items():
        assert max(errs.values()) <= BAR[bar], (bar, errs)
    assert np.abs(r["ref"]["gz"]).max() > 1e3 * BAR["ndp"]
    if name != "b66":
        ge = MV.group_errors(r["grads"]["gw"], r["ref"]["w"])
        print(f"{name}: weights by parameter group " + " ".join(f"{n} {v:.2e}" for n, v in ge.items()))


# ---- 4. the torch layer against the per-tick chain
def test_torch_closed_loop_formation_against_the_chain(ndp, oracle, shared):
    """closed_loop_formation against the per-tick torch chain plant_force -> control_step_trajectory -> plant_step on the same inputs
    (B = 6): values bit-equal; the chain's gradients in x_0, xr, ur, f and the weights within the bars of test 3; the Function's own
    gradients are the direct call's bits (f: its float32 rounding)."""
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    r = full(ndp, oracle, "b6", shared)
    a, N, g = r["a"], r["N"], r["grads"]
    G, H, A, Fu = (_t(u) for u in r["ups"])
    idx = _t(a["index"])

    def leaves():
        return dict(x0=_t(a["x0"]).requires_grad_(True), xr=_t(a["xr"]).requires_grad_(True), ur=_t(a["ur"]).requires_grad_(True),
                    f=_t(a["f"], torch.float32).requires_grad_(True), w=_t(a["blob"], torch.float32).requires_grad_(True))
    names = ("x0", "xr", "ur", "f", "w")
    eng = _engine(ndp, a, N, index=None)
    lv = leaves()
    xs, us, Xs, fps = TL.closed_loop_formation(eng, lv["x0"], lv["xr"], lv["ur"], idx, f=lv["f"], weights=lv["w"])
    one = dict(zip(names, torch.autograd.grad((G * xs).sum() + (H * us).sum() + (A * Xs).sum() + (Fu * fps).sum(), [lv[n_] for n_ in names])))
    torch.cuda.synchronize()
    eng.synchronize()
    eng.close()
    for got, want in ((xs, "xs"), (us, "us"), (Xs, "Xs"), (fps, "fps")):
        assert np.array_equal(_np(got), r["vals"][want], equal_nan=True), want
    for n_, m in (("x0", "gx0"), ("xr", "gxr"), ("ur", "gur"), ("w", "gw")):
        assert np.array_equal(_np(one[n_]), g[m], equal_nan=True), n_
    assert one["f"].dtype == torch.float32 and np.array_equal(_np(one["f"]), g["gf"].astype(np.float32))
    eng = _engine(ndp, a, N, index=None)
    lv = leaves()
    x, L, cx, cu, cX, cf = lv["x0"], 0.0, [], [], [], []
    for k in range(K):
        fp = TL.plant_force(eng, x, idx, weights=lv["w"])
        u0, X, U = TL.control_step_trajectory(eng, x, lv["xr"][k], lv["ur"][k], f=lv["f"][k])
        x = TL.plant_step(eng, x, u0, fp)
        L = L + (G[k] * x).sum() + (H[k] * u0).sum() + (A[k] * X).sum() + (Fu[k] * fp).sum()
        cx.append(_np(x)); cu.append(_np(u0)); cX.append(_np(X)); cf.append(_np(fp))
    chain = dict(zip(names, torch.autograd.grad(L, [lv[n_] for n_ in names])))
    torch.cuda.synchronize()
    eng.synchronize()
    eng.close()
    for got, want in ((cx, "xs"), (cu, "us"), (cX, "Xs"), (cf, "fps")):
        assert np.array_equal(np.stack(got), r["vals"][want], equal_nan=True), want
    c = {n_: _np(v).astype(np.float64) for n_, v in chain.items()}
    which = r["which"]
    e = _errors(dict(gx0=g["gx0"], gxr=g["gxr"], gur=g["gur"], gf=g["gf"].astype(np.float32).astype(np.float64), gw=g["gw"]),
                dict(x0=c["x0"][which], xr=c["xr"][:, which], ur=c["ur"][:, which], f=c["f"][:, which], w=c["w"]), which, with_w=True)
    for bar, errs in e.items():
        print(f"one call against the torch chain, held to BAR[{bar!r}] = {BAR[bar]:.1e}: " + " ".join(f"{n_} {v:.3e}" for n_, v in errs.items()))
    # the chain's gradient of f is float32: the last tick's is a rounding of a float64 value within BAR["ext"] of the one call's, one
    # float32 ulp of the row's largest entry more (tests/test_closed_loop_vjp_gpu.py's allowance); xr and ur are float64 on both routes
    f_last = e["ext"].pop("f_last")
    assert f_last <= BAR["ext"] + 2.0 ** -23, f_last
    for bar, errs in e.items():
        assert max(errs.values()) <= BAR[bar], (bar, errs)


# ---- 5. degenerate equalities
def test_all_slots_empty_is_the_ext_form_bit_for_bit(ndp, oracle, shared):
    """Every slot -1: the forward is closed_loop_device with d_fp NULL and fps exact zeros; every output of the reverse call is
    closed_loop_vjp_device's with d_fp = zeros, bit for bit, and g_w is exact zeros."""
    import torch
    r = full(ndp, oracle, "b6", shared)
    a, N, n = r["a"], r["N"], r["n"]
    eng = _engine(ndp, a, N, index=np.full((n, 2), -1, dtype=np.int32))
    t, v = _forward(eng, a, N)
    g = _reverse(eng, t, N, r["ups"][:3] + (None,))
    eng.close()
    eng = _engine(ndp, a, N, index=None)
    o = dict(xs=torch.empty(K, n, 10, dtype=torch.float64, device=_dev()), us=torch.empty(K, n, 4, dtype=torch.float64, device=_dev()),
             Xs=torch.empty(K, n, N + 1, 10, dtype=torch.float64, device=_dev()))
    tape = eng.closed_loop_tape(K)
    torch.cuda.synchronize()
    eng.closed_loop_device(t["x0"], t["xr"], t["ur"], o["xs"], o["us"], f=t["f"], fp=None, Xs=o["Xs"], tape=tape)
    eng.synchronize()
    for n_ in ("xs", "us", "Xs"):
        assert np.array_equal(_np(o[n_]), v[n_], equal_nan=True), n_
    assert np.array_equal(_bits(v["fps"]), np.zeros((K, n, 3), dtype=np.int64))
    for k in range(K):                     # (slot by slot: the padding behind a slot's three arrays is nobody's)
        for x, y in zip(eng.closed_loop_tape_slot(tape, k), eng.closed_loop_tape_slot(t["tape"], k)):
            assert np.array_equal(_np(x), _np(y), equal_nan=True), k
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    e = dict(gx0=z(n, 10), gxr=z(K, n, N + 1, 10), gur=z(K, n, N, 4), gf=z(K, n, N + 1, 3), gmodel=z(n, 16))
    ups = [_t(u) for u in r["ups"][:3]]
    torch.cuda.synchronize()
    eng.closed_loop_vjp_device(t["x0"], t["xr"], t["ur"], o["xs"], o["us"], tape, f=t["f"], fp=torch.zeros(K, n, 3, dtype=torch.float64, device=_dev()),
                               gxs=ups[0], gus=ups[1], gXs=ups[2], **e)
    eng.synchronize()
    eng.close()
    for n_, want in e.items():
        assert np.array_equal(g[n_], _np(want), equal_nan=True), n_
    assert np.array_equal(_bits(g["gw"]), np.zeros(MV.mlp_frag.NPARAM, dtype=np.int32))


def test_pairs_with_one_slot_equal_two_slots_with_an_empty_second(ndp, oracle, shared):
    """K = 1 pairs (index i ^ 1) against K = 2 with the second slot empty: every output of both calls bit-equal."""
    r = full(ndp, oracle, "b6", shared)
    a, N, n = r["a"], r["N"], r["n"]
    one = (np.arange(n, dtype=np.int32) ^ 1)[:, None]
    two = np.concatenate([one, np.full((n, 1), -1, dtype=np.int32)], axis=1)
    out = []
    for idx in (one, two):
        eng = _engine(ndp, a, N, index=idx)
        t, v = _forward(eng, a, N)
        out.append((v, _reverse(eng, t, N, r["ups"])))
        eng.close()
    assert np.abs(out[0][0]["fps"]).max() > 1.0 and np.abs(out[0][1]["gw"]).max() > 0
    for n_ in out[0][0]:
        assert np.array_equal(out[0][0][n_], out[1][0][n_], equal_nan=True), n_
    for n_ in out[0][1]:
        assert np.array_equal(out[0][1][n_], out[1][1][n_], equal_nan=True), n_


# ---- 6. determinism and independence
def test_repeats_single_outputs_state_and_streams(ndp, oracle, shared):
    """Two reverse calls are bit-identical; each output asked for alone (and with one upstream alone: gfps) is what it is when all are
    asked for; the engine's iterate and kept set and the tape are not written; forward and reverse on a side stream give the same bits."""
    import torch
    r = full(ndp, oracle, "b66", shared)
    eng, t, g, N = r["eng"], r["t"], r["grads"], r["N"]
    for x, y in zip(r["after_fwd"], r["after_bwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    again = _reverse(eng, t, N, r["ups"])
    for n_ in OUTS + ("status_check",):
        assert np.array_equal(again[n_], g[n_], equal_nan=True), n_
    for n_ in OUTS:
        assert np.array_equal(_reverse(eng, t, N, r["ups"], ask=(n_,))[n_], g[n_], equal_nan=True), n_
    only_f = _reverse(eng, t, N, (None, None, None, r["ups"][3]))
    assert np.isfinite(only_f["gx0"][r["which"]]).all() and np.abs(only_f["gw"]).max() > 0
    assert np.array_equal(_np(t["tape"]), r["tape_after"])
    for x, y in zip(_state(eng), r["after_fwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    side = torch.cuda.Stream(device=_dev())
    eng2 = _engine(ndp, r["a"], N)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t2, v2 = _forward(eng2, r["a"], N, stream=side)
        g2 = _reverse(eng2, t2, N, r["ups"], stream=side)
    side.synchronize()
    eng2.close()
    for n_ in ("xs", "us", "fps", "Xs", "status"):
        assert np.array_equal(v2[n_], r["vals"][n_], equal_nan=True), n_
    for n_ in OUTS:
        assert np.array_equal(g2[n_], g[n_], equal_nan=True), n_


# ---- 7. a failed vehicle
def test_a_failed_vehicle_takes_its_triple_and_nobody_else(ndp, oracle, shared):
    """B = 6, gate off (a NaN state closes a gate: with it on the neighbours would simply stop hearing the vehicle after tick 0), vehicle 1
    given a NaN velocity in x_0 as tests/test_closed_loop_vjp_gpu.py does: its status words are nonzero and d_status_check tells; its own
    outputs are NaN at every tick; its triple-mates hear a non-finite state at every tick, so their g_x0, their outputs of every tick but
    the last and their d_gmodel rows are NaN; the other triple is bit-equal to the clean run; d_gw is finite and equals the clean run's
    with that triple's upstreams zeroed.  Then the same failure with the gate on: what holds there (see the second half)."""
    r = full(ndp, oracle, "b6", shared)
    a, N, bad, triple, rest = r["a"], r["N"], 1, [0, 1, 2], [3, 4, 5]
    eng = _engine(ndp, a, N)
    t0, v0 = _forward(eng, a, N, gate=False)
    clean = _reverse(eng, t0, N, r["ups"])
    zeroed = tuple(np.where(np.isin(np.arange(6), triple).reshape((1, 6) + (1,) * (u.ndim - 2)), 0.0, u) for u in r["ups"])
    gw_zeroed = _reverse(eng, t0, N, zeroed, ask=("gw",))["gw"]
    eng.close()
    b = dict(a, x0=a["x0"].copy())
    b["x0"][bad, 3] = np.nan
    eng = _engine(ndp, b, N)
    t, v = _forward(eng, b, N, gate=False)
    g = _reverse(eng, t, N, r["ups"])
    eng.close()
    assert (v["status"][:, bad] != 0).all() and np.array_equal(g["status_check"], v["status"])
    assert np.array_equal(v["status"][:, rest], v0["status"][:, rest])
    for n_ in ("gxr", "gur", "gf"):
        assert np.isnan(g[n_][:, bad]).all(), n_
        for m in (0, 2):                   # (a mate's own steps have status 0: rows their adjoint writes as exact 0 stay 0)
            assert all(np.isnan(g[n_][k, m]).any() for k in range(K - 1)), (n_, m)
        assert np.array_equal(g[n_][:, rest], clean[n_][:, rest]), n_
    assert np.isnan(g["gx0"][bad]).all() and np.isnan(g["gx0"][triple]).any(axis=1).all() and np.isnan(g["gmodel"][triple]).any(axis=1).all()
    assert np.array_equal(g["gx0"][rest], clean["gx0"][rest]) and np.array_equal(g["gmodel"][rest], clean["gmodel"][rest])
    for n_ in ("xs", "us", "Xs", "fps"):
        assert np.array_equal(v[n_][:, rest], v0[n_][:, rest]), n_
    assert np.isfinite(g["gw"]).all() and np.abs(g["gw"]).max() > 0
    assert np.array_equal(g["gw"], gw_zeroed), float(np.abs(g["gw"] - gw_zeroed).max())
    assert not np.array_equal(clean["gw"], gw_zeroed)                  # (the triple's share was there to leave out)
    # gate on (the layer's default): from tick 1 the failed vehicle's NaN position closes every slot that names it, so its mates fly on
    # without hearing it and keep feeding d_gw -- that equality is not promised there.  What is: d_status_check tells, the vehicle's own
    # outputs are NaN, and the other triple is the clean gate-on run's, bit for bit, values and gradients
    eng = _engine(ndp, b, N)
    t, v = _forward(eng, b, N)
    g = _reverse(eng, t, N, r["ups"])
    eng.close()
    assert (v["status"][:, bad] != 0).all() and np.array_equal(g["status_check"], v["status"])
    assert np.isnan(g["gx0"][bad]).all() and np.isfinite(g["gw"]).all()
    for n_ in ("gxr", "gur", "gf"):
        assert np.isnan(g[n_][:, bad]).all(), n_
        assert np.array_equal(g[n_][:, rest], r["grads"][n_][:, rest]), n_
    assert np.array_equal(g["gx0"][rest], r["grads"]["gx0"][rest]) and np.array_equal(g["gmodel"][rest], r["grads"]["gmodel"][rest])
    for n_ in ("xs", "us", "Xs", "fps", "status"):
        assert np.array_equal(v[n_][:, rest], r["vals"][n_][:, rest]), n_


# ---- 8. refusals
def test_refusals_name_the_call_and_enqueue_nothing(ndp, oracle, shared):
    """Every new entry: not configured, K out of range, a missing tape, no upstream, no output, weights never set, d_fps NULL -- the
    return code, the whole ndp_last_error text, and the outputs keep their fill."""
    import torch
    r = full(ndp, oracle, "n7", shared)
    a, N, n, t = r["a"], r["N"], r["n"], r["t"]
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    xs, us, fps, gx0, gxs = z(K, n, 10), z(K, n, 4), z(K, n, 3), z(n, 10), _t(r["ups"][0])
    gz = z(n, 2, 6)

    def refused(eng, call, code, text):
        with pytest.raises(ndp.NdpError) as ei:
            call()
        assert "failed (%d)" % code in str(ei.value), str(ei.value)
        if text is not None:
            assert eng._lib.ndp_last_error(eng._h).decode() == text

    fwd = lambda e, **kw: e.closed_loop_formation_device(**{**dict(x0=t["x0"], xr=t["xr"], ur=t["ur"], xs=xs, us=us, fps=fps, f=t["f"]), **kw})  # noqa: E731
    bwd = lambda e, **kw: e.closed_loop_formation_vjp_device(**{**dict(x0=t["x0"], xr=t["xr"], ur=t["ur"], xs=t["xs"], us=t["us"],  # noqa: E731
                                                                       fps=t["fps"], tape=t["tape"], f=t["f"], gxs=gxs, gx0=gx0), **kw})
    F, V, S, CFG = ("ndp_closed_loop_formation_device", "ndp_closed_loop_formation_vjp_device", "ndp_plant_force_scatter_device",
                    "ndp_closed_loop_formation_config")
    none = ": no formation configured (ndp_closed_loop_formation_config)"
    eng = ndp.BatchedNMPC(n, N=N, disturbance=True)
    refused(eng, lambda: fwd(eng), -2, F + none)
    refused(eng, lambda: bwd(eng), -2, V + none)
    refused(eng, lambda: eng.plant_force_scatter_device(gz, gx0), -2, S + none)
    idx = np.ascontiguousarray(a["index"], dtype=np.int32)
    for Kn in (0, 9, -1):
        assert eng._lib.ndp_closed_loop_formation_config(eng._h, idx.ctypes.data_as(Ct.c_void_p), Kn) == -2
        assert eng._lib.ndp_last_error(eng._h).decode() == CFG + ": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle), got %d" % Kn
    refused(eng, lambda: fwd(eng), -2, F + none)                      # (a refused configuration configures nothing)
    eng.closed_loop_formation_config(a["index"])
    refused(eng, lambda: fwd(eng, fps=None), -1, None)
    refused(eng, lambda: bwd(eng, fps=None), -1, None)
    refused(eng, lambda: eng.plant_force_scatter_device(None, gx0), -1, None)
    refused(eng, lambda: fwd(eng, substeps=0), -2, F + ": substeps must be 1..16 (NDP_PLANT_MAX_SUBSTEPS), got 0")
    refused(eng, lambda: bwd(eng, tape=None), -2, V + ": d_tape is required (the forward's, recorded by ndp_closed_loop_formation_device)")
    refused(eng, lambda: bwd(eng, gxs=None), -2, V + ": no upstream gradient (d_gxs, d_gus, d_gXs and d_gfps all NULL)")
    refused(eng, lambda: bwd(eng, gx0=None), -2, V + ": no output asked for (d_gx0, d_gxr, d_gur, d_gf, d_gw and d_gmodel all NULL)")
    eng.closed_loop_formation_config(None)
    refused(eng, lambda: fwd(eng), -2, F + none)                      # NULL clears
    eng.synchronize()
    eng.close()
    eng = ndp.BatchedNMPC(n, N=N, disturbance=True, load_mlp=False)
    eng.closed_loop_formation_config(a["index"])
    refused(eng, lambda: fwd(eng), -6, F + ": ndp_set_mlp_weights was never called")
    refused(eng, lambda: bwd(eng), -6, V + ": ndp_set_mlp_weights was never called")
    eng.synchronize()
    torch.cuda.synchronize()
    eng.close()
    for buf in (xs, us, fps, gx0):
        assert (_np(buf) == -7.0).all()
