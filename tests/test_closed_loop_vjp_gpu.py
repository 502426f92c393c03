"""The one-call closed loop and its reverse mode on the device (run with -m gpu): ndp_closed_loop_device against the plain loop of
update_device and ndp_plant_step_device, bit for bit, and ndp_closed_loop_vjp_device against the composed float64 reference of
tests/closed_loop_chain_ref.py (every leaf) and tests/closed_loop_vjp_ref.py (the model gradient), at N = 20 (the compile-time kernels)
and N = 7 (the run-time-horizon kernels), K = 3 ticks, B = 65 (one vehicle past a full 64-lane workgroup of the link kernels).
CPU side: tests/test_closed_loop_vjp.py.

Inputs: closed_loop_chain_ref.ext_inputs(65, K, N, 20231516), the inputs of tests/test_closed_loop_chain_gpu.py.  On the CPU oracle all 65
vehicles finish every tick on a set at both horizons, 13-16 of them with a pinned input, and all 65 keep their sets under test 4's
perturbations.  The referenced six are picked by that file's _pick on the oracle's record.

Bars, none of them from what the code under test gives:
  leaf gradients   BAR["ext"] of tests/test_closed_loop_chain_gpu.py (ten times what the chain through the same links measured), by its
                   rel_err: |dev - ref| / max(1, |ref|max of the leaf's row)
  model gradient   per tick the step link's STEP_BAR = 1e-9 max(1, |g|max) (tests/test_model_grad_gpu.py writes the same figure as a
                   literal; the named one is imported from the chain's test), K of them for the sum over the ticks; column 15 is linear
                   in gfp, which is held to BAR["ext"]: BAR["ext"] max(1, |gfp|max) sum_k |fp_k|_1 / m
  finite differences  FD_BAR = 1e-6 of max(1, |g|) on the vehicles whose sets and iteration words move in no run, at least 40 of the 65
Measured on the first device run (MI355X), all 65 vehicles set finishes on the device at both horizons:
  leaf gradients   N = 20: x0 2.2e-13, xr 6.4e-14, ur 1.8e-13, f 5.1e-14, fp 1.1e-14; N = 7: x0 8.1e-13, xr 3.3e-13, ur 3.2e-13, f 1.4e-13,
                   fp 2.5e-14; substeps 1 / 16 (K = 2): 6.2e-13 / 6.3e-13; against the layer's chain 5.6e-15 (f as float32: 2.8e-8)
  model gradient   5.6e-5 of its bar (columns 0..14), 5.8e-4 (column 15)
  finite differences  9.9e-9, 65 of 65 stable"""
import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import closed_loop_vjp_ref as M
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.fixed_set_ref import scale
from tests.test_closed_loop_chain_gpu import BAR, FD_BAR, STEP_BAR, _chain, _grads, _leaves, _pick, _plain_loop

pytestmark = pytest.mark.gpu

K, B, SEED = 3, 65, 20231516
HORIZONS = [20, 7]
GUARD = 2
OUTS = ("gx0", "gxr", "gur", "gf", "gfp")


def _np(t):
    return t.detach().cpu().numpy()


def _engine(ndp, a, N, force=True, moved=None, **kw):
    """A fresh engine: reset to tick 0's window and one warm-up step on tick 0's inputs, so that a kept set exists.  kw: ndp_cfg
    overrides (the model); moved: (Qd, Rd, mass) installed by set_model before the reset and the warm-up step."""
    import torch
    n = a["x0"].shape[0]
    eng = ndp.BatchedNMPC(n, N=N, disturbance=force, **kw)
    if moved is not None:
        eng.set_model(Qd=moved[0], Rd=moved[1], mass=moved[2])
    eng.reset(a["xr"][0], a["ur"][0])
    u0 = torch.empty(n, 4, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    eng.update_device(_t(a["x0"]), _t(a["xr"][0]), _t(a["ur"][0]), u0, f=_t(a["f"][0], torch.float32) if force else None)
    eng.synchronize()
    return eng


def _state(eng):
    return [_np(v) for v in eng.device_iterate()] + [eng.active_set()[1]]


def _loop(eng, a, ticks, substeps, force=True, dt=R.DT):
    """_plain_loop's record for any number of ticks, substeps and plant tick dt, with or without the two forces (ext form only)."""
    import ctypes as C
    import torch
    n = a["x0"].shape[0]
    x = _t(a["x0"])
    rec = {k: [] for k in ("x", "force", "Xpre", "Upre", "act_pre", "act", "u0", "X", "st", "it")}
    for k in range(ticks):
        tape = eng.record_tape()
        f = _t(a["f"][k], torch.float32) if force else None
        fp = _t(a["fp"][k]) if force else None
        u0 = torch.empty(n, 4, dtype=torch.float64, device=_dev())
        torch.cuda.synchronize()
        eng.update_device(x, _t(a["xr"][k]), _t(a["ur"][k]), u0, f=f)
        eng.synchronize()
        X = eng.device_iterate()[0].clone()
        xn = x.clone()
        torch.cuda.synchronize()
        st, it = eng.status()
        eng._check(eng._lib.ndp_plant_step_device(eng._h, C.c_void_p(xn.data_ptr()), C.c_void_p(u0.data_ptr()),
                                                  None if fp is None else C.c_void_p(fp.data_ptr()), float(dt), int(substeps), None), "ndp_plant_step_device")
        eng.synchronize()
        for name, v in (("x", _np(x)), ("force", a["f"][k].astype(np.float64)), ("Xpre", _np(tape[0])), ("Upre", _np(tape[1])),
                        ("act_pre", _np(tape[2])), ("act", eng.active_set()[1]), ("u0", _np(u0)), ("X", _np(X)), ("st", st), ("it", it)):
            rec[name].append(v)
        x = xn
    rec["x"].append(_np(x))
    rec = {k: np.stack(v) for k, v in rec.items()}
    rec.update(xr=a["xr"][:ticks], ur=a["ur"][:ticks], fp=a["fp"][:ticks], other=None, idx=None, blob=None)
    return rec


def _guarded(*shape, dtype=None, fill=-7.0):
    """(the array, the whole buffer): a contiguous array of `shape` with GUARD rows of its last-but-leading layout behind it."""
    import torch
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else shape[0]
    last = shape[-1] if len(shape) > 1 else 1
    whole = torch.full((rows + GUARD, last), fill, dtype=dtype or torch.float64, device=_dev())
    return whole[:rows].view(*shape), whole


def _forward(eng, a, N, ticks=K, substeps=R.SUBSTEPS, force=True, stream=None, dt=R.DT, tape=True):
    """closed_loop_device into guarded outputs; returns the tensors the reverse call needs and the numpy values.  tape False: the call
    is given no tape (the reverse call cannot follow)."""
    import torch
    n = a["x0"].shape[0]
    t = dict(x0=_t(a["x0"]), xr=_t(a["xr"][:ticks]), ur=_t(a["ur"][:ticks]), f=_t(a["f"][:ticks], torch.float32) if force else None,
             fp=_t(a["fp"][:ticks]) if force else None)
    o = dict(xs=_guarded(ticks, n, 10), us=_guarded(ticks, n, 4), Xs=_guarded(ticks, n, N + 1, 10),
             status=_guarded(ticks, n, dtype=torch.int32, fill=-7))
    tape = eng.closed_loop_tape(ticks) if tape else None
    torch.cuda.synchronize()
    eng.closed_loop_device(t["x0"], t["xr"], t["ur"], o["xs"][0], o["us"][0], f=t["f"], fp=t["fp"], Xs=o["Xs"][0],
                           status=o["status"][0].view(ticks, n), tape=tape, dt=dt, substeps=substeps, stream=stream)
    eng.synchronize()
    torch.cuda.synchronize()
    t.update(xs=o["xs"][0], us=o["us"][0], tape=tape, substeps=substeps, dt=dt)
    vals = {k: _np(v[0]) for k, v in o.items()}
    vals["status"] = vals["status"].reshape(ticks, n)
    for k, v in o.items():
        assert (_np(v[1])[-GUARD:] == -7).all(), k
    return t, vals


def _reverse(eng, t, N, ups, ask=OUTS + ("gmodel",), stream=None):
    """closed_loop_vjp_device into guarded, -7.0-filled outputs; returns {name: numpy} of what was asked for, plus status_check."""
    import torch
    ticks, n = t["xr"].shape[0], t["x0"].shape[0]
    shapes = dict(gx0=(n, 10), gxr=(ticks, n, N + 1, 10), gur=(ticks, n, N, 4), gf=(ticks, n, N + 1, 3), gfp=(ticks, n, 3), gmodel=(n, 16))
    o = {k: _guarded(*shapes[k]) for k in ask}
    st = _guarded(ticks, n, dtype=torch.int32, fill=-7)
    g = [None if u is None else _t(u[:ticks]) for u in ups]
    torch.cuda.synchronize()
    eng.closed_loop_vjp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["tape"], f=t["f"], fp=t["fp"], gxs=g[0], gus=g[1], gXs=g[2],
                               status_check=st[0].view(ticks, n), dt=t.get("dt", R.DT), substeps=t["substeps"], stream=stream,
                               **{k: v[0] for k, v in o.items()})
    eng.synchronize()
    torch.cuda.synchronize()
    for k, v in list(o.items()) + [("status_check", st)]:
        assert (_np(v[1])[-GUARD:] == -7).all(), k
    out = {k: _np(v[0]) for k, v in o.items()}
    out["status_check"] = _np(st[0]).reshape(ticks, n)
    return out


@pytest.fixture(scope="module")
def shared():
    cache = {}
    yield cache
    for r in cache.values():
        r["eng"].close()


def full(ndp, oracle, N, cache):
    """Everything the tests of one horizon share, computed once and left unchanged: the inputs, the oracle's record (the referenced
    vehicles), the device's record from the plain loop, ONE run of the one call and of its reverse call with every output, and the
    reference on the device's record.  The engine of the one call stays open (its state: after the forward)."""
    if N in cache:
        return cache[N]
    a = R.ext_inputs(B, K, N, SEED)
    cpu = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], f=a["f"])
    which = _pick(cpu, R.set_finish(cpu))
    eng = _engine(ndp, a, N)
    rec = _plain_loop(eng, a, "ext")
    after_loop = _state(eng)
    eng.close()
    eng = _engine(ndp, a, N)
    t, vals = _forward(eng, a, N)
    after_fwd = _state(eng)
    ups = R.upstreams(K, B, N, seed=31)
    grads = _reverse(eng, t, N, ups)
    r = dict(a=a, cpu=cpu, which=which, rec=rec, ok=R.set_finish(rec), after_loop=after_loop, eng=eng, t=t, vals=vals, after_fwd=after_fwd,
             ups=ups, grads=grads, after_bwd=_state(eng), tape_after=_np(t["tape"]))
    if r["ok"][which].all():
        r["sys"] = R.systems(oracle, rec, which)
        r["ref"] = R.reverse(r["sys"], rec, *ups)
    cache[N] = r
    return r


def _leaf_errors(g, ref, which):
    return dict(x0=R.rel_err(g["gx0"][which], ref["x0"], 1), xr=R.rel_err(g["gxr"][:, which], ref["xr"], 2),
                ur=R.rel_err(g["gur"][:, which], ref["ur"], 2), f=R.rel_err(g["gf"][:, which], ref["f"], 2),
                fp=R.rel_err(g["gfp"][:, which], ref["fp"], 2))


def _model_errors(oracle, sys_, rec, ups, gm, which):
    """(worst |dev - ref| over its bar for columns 0..14, the same for column 15): the bars of the module docstring."""
    tot, per = M.model_reverse(oracle, sys_, rec, *ups)
    cfg = oracle.default_cfg(N=sys_["N"], use_fd=True)
    _, gfp = M.sweep_upstreams(sys_, rec, *ups)
    e14 = e15 = 0.0
    for j, v in enumerate(which):
        bar = sum(STEP_BAR * scale(per[k, j, :15]) for k in range(sys_["K"]))
        e14 = max(e14, float(np.abs(gm[v, :15] - tot[j, :15]).max()) / bar)
        bar15 = BAR["ext"] * scale(gfp[:, j]) * float(np.abs(rec["fp"][:, v]).sum()) / cfg.mass
        e15 = max(e15, abs(gm[v, 15] - tot[j, 15]) / bar15)
    return e14, e15


# ---- 0. the conditions on the inputs
@pytest.mark.parametrize("N", HORIZONS)
def test_the_inputs_meet_their_conditions(ndp, oracle, shared, N):
    """Six referenced vehicles, set finishes on the oracle and on the device with the oracle's sets, one of them with a stage-0 input on its
    bound in one tick and free in a later one; at most a quarter of the 65 miss a set finish on the device (reported, and left out of the
    batch-wide checks)."""
    r = full(ndp, oracle, N, shared)
    rec, which, ok = r["rec"], r["which"], r["ok"]
    print(f"N={N}: {int((~ok).sum())} of {B} vehicles are no set finishes on the device: {np.flatnonzero(~ok).tolist()}; referenced {which}")
    assert len(which) == 6 and R.set_finish(r["cpu"])[which].all() and ok[which].all() and (~ok).sum() <= B // 4
    assert np.array_equal(rec["act"][:, which], r["cpu"]["act"][:, which])
    pin0 = rec["act"][:, :, 0, :].any(axis=2)
    assert any(pin0[k, v] and (~pin0[k + 1:, v]).any() for v in which for k in range(K - 1))


# ---- 1. values
@pytest.mark.parametrize("N", HORIZONS)
def test_values_are_the_plain_loops_bits(ndp, oracle, shared, N):
    """xs, us, Xs, the status words and the engine's iterate and kept set afterwards are bit-equal to the plain loop's from an identically
    prepared engine; tape slot k is record_tape() taken before tick k of that loop; the recomputed status words are the forward's."""
    r = full(ndp, oracle, N, shared)
    rec, v, eng = r["rec"], r["vals"], r["eng"]
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(v["us"], rec["u0"], equal_nan=True)
    assert np.array_equal(v["Xs"], rec["X"], equal_nan=True) and np.array_equal(v["status"], rec["st"])
    for x, y in zip(r["after_fwd"], r["after_loop"]):
        assert np.array_equal(x, y, equal_nan=True)
    for k in range(K):
        X, U, A = (_np(s) for s in eng.closed_loop_tape_slot(r["t"]["tape"], k))
        assert np.array_equal(X, rec["Xpre"][k], equal_nan=True) and np.array_equal(U, rec["Upre"][k], equal_nan=True)
        assert np.array_equal(A, rec["act_pre"][k])
    assert np.array_equal(r["grads"]["status_check"], rec["st"])


@pytest.mark.parametrize("N", HORIZONS)
def test_values_without_forces_and_for_one_vehicle_one_tick(ndp, oracle, shared, N):
    """d_f = d_fp = NULL on a use_fd = 0 engine, and ticks = 1 with B = 1: the plain loop's bits."""
    a = full(ndp, oracle, N, shared)["a"]
    one = {k: (v[:1] if k == "x0" else v[:, :1]) for k, v in a.items()}
    for inputs, ticks, force in ((a, K, False), (one, 1, True)):
        eng = _engine(ndp, inputs, N, force=force)
        rec = _loop(eng, inputs, ticks, R.SUBSTEPS, force=force)
        after = _state(eng)
        eng.close()
        eng = _engine(ndp, inputs, N, force=force)
        t, v = _forward(eng, inputs, N, ticks=ticks, force=force)
        assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(v["us"], rec["u0"], equal_nan=True)
        assert np.array_equal(v["Xs"], rec["X"], equal_nan=True) and np.array_equal(v["status"], rec["st"])
        for x, y in zip(_state(eng), after):
            assert np.array_equal(x, y, equal_nan=True)
        for k in range(ticks):
            X, U, A = (_np(s) for s in eng.closed_loop_tape_slot(t["tape"], k))
            assert np.array_equal(X, rec["Xpre"][k], equal_nan=True) and np.array_equal(A, rec["act_pre"][k])
        eng.close()


# ---- 2. gradients against the float64 reference
@pytest.mark.parametrize("N", HORIZONS)
def test_every_leaf_gradient_matches_the_reverse_sweep(ndp, oracle, shared, N):
    """gx0, gxr, gur, gf, gfp against closed_loop_chain_ref.reverse on the device's own record, by rel_err, held to BAR["ext"]."""
    r = full(ndp, oracle, N, shared)
    e = _leaf_errors(r["grads"], r["ref"], r["which"])
    print(f"N={N}: one call against the reference, measured " + " ".join(f"{n} {v:.3e}" for n, v in e.items())
          + f"; worst {max(e.values()):.3e}, bar {BAR['ext']:.1e}")
    assert max(e.values()) <= BAR["ext"], e


@pytest.mark.parametrize("N", HORIZONS)
def test_the_layers_chain_agrees_with_the_one_call(ndp, oracle, shared, N):
    """control_step_trajectory -> plant_step, tick by tick, and its backward on the same inputs: values bit-equal, gradients within
    BAR["ext"] by rel_err on the device's set finishes (not bit-equal: the plant's adjoint may round differently from one kernel to the
    next).  The chain's float32 gradient of f is a rounding of a float64 value within that bar of the one call's: one float32 ulp of the
    row's largest entry more, 2^-23."""
    import torch
    r = full(ndp, oracle, N, shared)
    eng = _engine(ndp, r["a"], N)
    lv = _leaves(r["a"], "ext")
    xs, u0s, Xs, L = _chain(eng, lv, "ext", tuple(_t(u) for u in r["ups"]))
    L.backward()
    torch.cuda.synchronize()
    eng.synchronize()
    eng.close()
    assert np.array_equal(np.stack([_np(x) for x in xs]), r["vals"]["xs"], equal_nan=True)
    assert np.array_equal(np.stack([_np(x) for x in Xs]), r["vals"]["Xs"], equal_nan=True)
    c, g, ok = _grads(lv, "ext"), r["grads"], r["ok"]
    e = dict(x0=R.rel_err(g["gx0"][ok], c["x0"][ok], 1), xr=R.rel_err(g["gxr"][:, ok], c["xr"][:, ok], 2),
             ur=R.rel_err(g["gur"][:, ok], c["ur"][:, ok], 2), fp=R.rel_err(g["gfp"][:, ok], c["fp"][:, ok], 2))
    ef = R.rel_err(g["gf"][:, ok], c["f"][:, ok], 2)
    print(f"N={N}: one call against the layer's chain, measured " + " ".join(f"{n} {v:.3e}" for n, v in e.items()) + f"; f (float32) {ef:.3e}")
    assert max(e.values()) <= BAR["ext"], e
    assert ef <= BAR["ext"] + 2.0 ** -23


# ---- 3. the model gradient
@pytest.mark.parametrize("N", HORIZONS)
def test_model_gradient_matches_the_composed_reference(ndp, oracle, shared, N):
    """Columns 0..14 against sum_k model_grad_ref with the reference sweep's upstreams, K step bars; column 15 against the closed form;
    column 6 exactly 0; with d_gmodel NULL the other five outputs are bit-equal."""
    r = full(ndp, oracle, N, shared)
    gm, which = r["grads"]["gmodel"], r["which"]
    e14, e15 = _model_errors(oracle, r["sys"], r["rec"], r["ups"], gm, which)
    print(f"N={N}: model gradient, worst share of its bar: columns 0..14 {e14:.3e}, column 15 {e15:.3e}")
    assert e14 <= 1.0 and e15 <= 1.0
    assert np.isfinite(gm[r["ok"]]).all() and not gm[r["ok"]][:, 6].any() and np.abs(gm[which, 15]).max() > 1e-3
    plain = _reverse(r["eng"], r["t"], N, r["ups"], ask=OUTS)
    for n in OUTS:
        assert np.array_equal(plain[n], r["grads"][n], equal_nan=True), n
    nof = _reverse(r["eng"], dict(r["t"], fp=None), N, r["ups"], ask=("gmodel",))
    assert not nof["gmodel"][:, 15].any()                     # exactly 0 with d_fp NULL


# ---- 4. device finite differences
@pytest.mark.parametrize("N", HORIZONS)
def test_device_finite_differences(ndp, oracle, shared, N):
    """Central differences of L over the device's own closed loop in Qd[0], Rd[3] (set_model, steps 1e-5 of the value) and x_0's entries 2
    and 8 (steps 1e-6), every tick of every perturbed run restarted from the recorded iterate and kept set: within FD_BAR of max(1, |g|)
    on the vehicles whose sets and iteration words move in no run, at least 40 of the 65."""
    r = full(ndp, oracle, N, shared)
    a, rec, g = r["a"], r["rec"], r["grads"]
    G, H, A = r["ups"]
    eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
    eng.reset(a["xr"][0], a["ur"][0])
    Qd0, Rd0 = np.array(list(eng.cfg.Qd)), np.array(list(eng.cfg.Rd))
    cases = [("Qd", 0, 1e-5 * Qd0[0], g["gmodel"][:, 0]), ("Rd", 3, 1e-5 * Rd0[3], g["gmodel"][:, 13]), ("x0", 2, 1e-6, g["gx0"][:, 2]),
             ("x0", 8, 1e-6, g["gx0"][:, 8])]
    stable, fds = r["ok"].copy(), []
    for name, j, h, _ in cases:
        L = []
        for sgn in (1.0, -1.0):
            q, rd, x = Qd0.copy(), Rd0.copy(), a["x0"].copy()
            {"Qd": q, "Rd": rd}.get(name, x)[(slice(None), j) if name == "x0" else j] += sgn * h
            eng.set_model(Qd=q, Rd=rd)
            tot = np.zeros(B)
            for k in range(K):
                eng.set_iterate(rec["Xpre"][k], rec["Upre"][k])
                eng.set_active_set(rec["act_pre"][k])
                u, X, U, st, it = eng.update(x, a["xr"][k], a["ur"][k], f=a["f"][k], raise_on_status=False, full=True)
                stable &= (st == 0) & ((it & 0xffff) == 0) & (eng.active_set()[1] == rec["act"][k]).all(axis=(1, 2))
                x = eng.plant_step(x, u, a["fp"][k], dt=R.DT, substeps=R.SUBSTEPS)
                tot += (G[k] * x).sum(axis=1) + (H[k] * u).sum(axis=1) + (A[k] * X).sum(axis=(1, 2))
            L.append(tot)
        fds.append((L[0] - L[1]) / (2 * h))
    eng.close()
    print(f"N={N}: {int(stable.sum())} of {B} vehicles keep their sets and iteration words in every run")
    assert stable.sum() >= 40
    for (name, j, h, got), fd in zip(cases, fds):
        err = float((np.abs(fd - got)[stable] / np.maximum(1.0, np.abs(got[stable]))).max())
        print(f"N={N}: {name}[{j}] worst |fd - g| / max(1, |g|) = {err:.2e}, |g|max {np.abs(got[stable]).max():.2e}")
        assert err <= FD_BAR, (name, j, err)


# ---- 5. the contract
@pytest.mark.parametrize("N", HORIZONS)
def test_repeats_single_outputs_state_and_streams(ndp, oracle, shared, N):
    """Two reverse calls are bit-identical; each output asked for alone equals its value when all are asked for; the engine's iterate and
    kept set, and the tape, are bit-unchanged by the reverse call; forward and reverse on a side stream give the default stream's bits;
    the guard rows behind every output keep their -7.0 (checked in _forward and _reverse)."""
    import torch
    r = full(ndp, oracle, N, shared)
    eng, t, g = r["eng"], r["t"], r["grads"]
    for x, y in zip(r["after_fwd"], r["after_bwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    again = _reverse(eng, t, N, r["ups"])
    for n in OUTS + ("gmodel", "status_check"):
        assert np.array_equal(again[n], g[n], equal_nan=True), n
    for n in OUTS + ("gmodel",):
        assert np.array_equal(_reverse(eng, t, N, r["ups"], ask=(n,))[n], g[n], equal_nan=True), n
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
    for n in ("xs", "us", "Xs", "status"):
        assert np.array_equal(v2[n], r["vals"][n], equal_nan=True), n
    for n in OUTS + ("gmodel",):
        assert np.array_equal(g2[n], g[n], equal_nan=True), n


# ---- 6. substeps 1 and 16
@pytest.mark.parametrize("substeps", [1, 16])
def test_substeps_1_and_16(ndp, oracle, shared, substeps):
    """K = 2 at N = 20: values the plain loop's bits, leaf gradients and the model gradient held to the same bars (the plant adjoint
    recomputes O(substeps^2) substeps per tick)."""
    N, ticks = 20, 2
    r0 = full(ndp, oracle, N, shared)
    a, which = r0["a"], r0["which"]
    eng = _engine(ndp, a, N)
    rec = _loop(eng, a, ticks, substeps)
    eng.close()
    eng = _engine(ndp, a, N)
    t, v = _forward(eng, a, N, ticks=ticks, substeps=substeps)
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(v["us"], rec["u0"], equal_nan=True)
    ups = tuple(u[:ticks] for u in r0["ups"])
    g = _reverse(eng, t, N, ups)
    eng.close()
    assert R.set_finish(rec)[which].all()
    sys_ = R.systems(oracle, rec, which, substeps=substeps)
    e = _leaf_errors(g, R.reverse(sys_, rec, *ups), which)
    tot, per = M.model_reverse(oracle, sys_, rec, *ups)
    e14 = max(float(np.abs(g["gmodel"][v_, :15] - tot[j, :15]).max()) / sum(STEP_BAR * scale(per[k, j, :15]) for k in range(ticks))
              for j, v_ in enumerate(which))
    print(f"substeps {substeps}: measured " + " ".join(f"{n} {x:.3e}" for n, x in e.items()) + f"; bar {BAR['ext']:.1e}; "
          f"model gradient's worst share of its bar {e14:.3e}")
    assert max(e.values()) <= BAR["ext"], e
    assert e14 <= 1.0


# ---- 7. a NaN vehicle
def test_a_nan_vehicle_stays_with_itself(ndp, oracle, shared):
    """N = 20, vehicle 1 given a NaN velocity in x_0: its gradients and its gmodel row are NaN; every other vehicle's values and
    gradients are bit-unchanged."""
    N, bad = 20, 1
    r = full(ndp, oracle, N, shared)
    a = dict(r["a"], x0=r["a"]["x0"].copy())
    a["x0"][bad, 3] = np.nan
    eng = _engine(ndp, a, N)
    t, v = _forward(eng, a, N)
    g = _reverse(eng, t, N, r["ups"])
    eng.close()
    rest = np.arange(B) != bad
    assert (v["status"][:, bad] != 0).all() and np.array_equal(v["status"][:, rest], r["vals"]["status"][:, rest])
    assert np.array_equal(g["status_check"], v["status"])
    assert np.isnan(g["gx0"][bad]).all() and np.isnan(g["gmodel"][bad]).all()
    for n in ("gxr", "gur", "gf", "gfp"):
        assert np.isnan(g[n][:, bad]).all(), n
        assert np.array_equal(g[n][:, rest], r["grads"][n][:, rest], equal_nan=True), n
    assert np.array_equal(g["gx0"][rest], r["grads"]["gx0"][rest], equal_nan=True)
    assert np.array_equal(g["gmodel"][rest], r["grads"]["gmodel"][rest], equal_nan=True)
    for n in ("xs", "us", "Xs"):
        assert np.array_equal(v[n][:, rest], r["vals"][n][:, rest], equal_nan=True), n


# ---- 8. refusals
def test_refusals_name_the_call_and_enqueue_nothing(ndp, oracle, shared):
    """Every -1 / -2 case of include/ndp_nmpc.h returns its code with a reason that names the call, and the outputs keep their fill."""
    import torch
    N = 7
    r = full(ndp, oracle, N, shared)
    t = r["t"]
    eng = ndp.BatchedNMPC(B, N=N, disturbance=True)        # (a handle of its own: the sensitivities are switched on and off on it)
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    xs, us, gx0 = z(K, B, 10), z(K, B, 4), z(B, 10)
    gxs = _t(r["ups"][0])
    fwd = lambda e=eng, **kw: e.closed_loop_device(**{**dict(x0=t["x0"], xr=t["xr"], ur=t["ur"], xs=xs, us=us, f=t["f"], fp=t["fp"]), **kw})  # noqa: E731
    bwd = lambda e=eng, **kw: e.closed_loop_vjp_device(**{**dict(x0=t["x0"], xr=t["xr"], ur=t["ur"], xs=t["xs"], us=t["us"], tape=t["tape"],  # noqa: E731
                                                                 f=t["f"], fp=t["fp"], gxs=gxs, gx0=gx0), **kw})
    for call, who in ((fwd, "ndp_closed_loop_device"), (bwd, "ndp_closed_loop_vjp_device")):
        for kw, code in ((dict(x0=None), -1), (dict(ur=None), -1), (dict(us=None), -1), (dict(substeps=0), -2), (dict(substeps=17), -2)):
            with pytest.raises(ndp.NdpError, match=who + r" failed \(%d\)" % code + ("" if code == -1 else ".*" + who)):
                call(**kw)
        eng.enable_sensitivity(1)
        with pytest.raises(ndp.NdpError, match=who + r" failed \(-2\).*" + who + ".*sensitivities"):
            call()
        eng.enable_sensitivity(0)
    for kw, why in ((dict(tape=None), "d_tape"), (dict(gxs=None), "no upstream"), (dict(gx0=None), "no output")):
        with pytest.raises(ndp.NdpError, match=r"ndp_closed_loop_vjp_device failed \(-2\): ndp_closed_loop_vjp_device.*" + why):
            bwd(**kw)
    import ctypes as C
    for name in ("ndp_closed_loop_device", "ndp_closed_loop_vjp_device"):           # ticks < 1, and a NULL handle
        args = [0, R.DT, 4] + [C.c_void_p(xs.data_ptr())] * (11 if name.endswith("loop_device") else 19)
        assert getattr(eng._lib, name)(eng._h, *args) == -2 and name.encode() in eng._lib.ndp_last_error(eng._h)
        assert getattr(eng._lib, name)(None, *args) == -1
    # a force without use_fd; the adjoint's own refusals
    two = {k: (v[:2] if k == "x0" else v[:, :2]) for k, v in r["a"].items()}
    for kw, n_hor, why, both in ((dict(disturbance=False), N, "use_fd", True), (dict(n_rti=2), N, "n_rti", False),
                                 (dict(qp_precision=1), N, "qp_precision", False), (dict(), 30, "N <= 27", False)):
        e = ndp.BatchedNMPC(2, N=n_hor, **({"disturbance": True, **kw}))
        tt = dict(x0=_t(two["x0"]), xr=z(K, 2, n_hor + 1, 10), ur=z(K, 2, n_hor, 4), f=torch.zeros(K, 2, n_hor + 1, 3, dtype=torch.float32, device=_dev()),
                  fp=_t(two["fp"]), xs=z(K, 2, 10), us=z(K, 2, 4))
        if both:
            with pytest.raises(ndp.NdpError, match=r"ndp_closed_loop_device failed \(-2\): ndp_closed_loop_device.*" + why):
                e.closed_loop_device(**tt)
        with pytest.raises(ndp.NdpError, match=r"ndp_closed_loop_vjp_device failed \(-2\): ndp_closed_loop_vjp_device.*" + why):
            e.closed_loop_vjp_device(tape=e.closed_loop_tape(K), gxs=z(K, 2, 10), gx0=z(2, 10), **tt)
        e.synchronize()
        assert (_np(tt["xs"]) == -7.0).all() and (_np(tt["us"]) == -7.0).all()
        e.close()
    eng.synchronize()
    torch.cuda.synchronize()
    eng.close()
    assert (_np(xs) == -7.0).all() and (_np(us) == -7.0).all() and (_np(gx0) == -7.0).all()


# ---- 9. torch
@pytest.mark.parametrize("N", HORIZONS)
def test_torch_closed_loop_gives_the_direct_calls_bits(ndp, oracle, shared, N):
    """closed_loop(...) with a loss over xs, us and Xs: autograd.grad in x_0, xr, ur, f, fp, Qd, Rd and the mass gives the direct call's
    bits (f: its float32 rounding; Qd, Rd: the sum over the finite rows; the mass: column 14 + column 15); with only x_0 and Qd requiring
    a gradient the same two come out and nothing else is computed."""
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    r = full(ndp, oracle, N, shared)
    a, g = r["a"], r["grads"]
    G, H, A = (_t(u) for u in r["ups"])
    gm = _t(g["gmodel"])
    tot = torch.where(torch.isfinite(gm).all(dim=1, keepdim=True), gm, torch.zeros_like(gm)).sum(dim=0)
    for only in (None, ("x0", "Qd")):
        eng = _engine(ndp, a, N)
        mk = lambda n, v, dt=None: _t(v, dt).requires_grad_(only is None or n in only)  # noqa: E731
        lv = dict(x0=mk("x0", a["x0"]), xr=mk("xr", a["xr"]), ur=mk("ur", a["ur"]), f=mk("f", a["f"], torch.float32), fp=mk("fp", a["fp"]),
                  Qd=mk("Qd", list(eng.cfg.Qd), torch.float64), Rd=mk("Rd", list(eng.cfg.Rd), torch.float64),
                  mass=mk("mass", float(eng.cfg.mass), torch.float64))
        xs, us, Xs = TL.closed_loop(eng, lv["x0"], lv["xr"], lv["ur"], f=lv["f"], fp=lv["fp"], Qd=lv["Qd"], Rd=lv["Rd"], mass=lv["mass"])
        assert np.array_equal(_np(xs), r["vals"]["xs"], equal_nan=True) and np.array_equal(_np(Xs), r["vals"]["Xs"], equal_nan=True)
        names = list(lv) if only is None else list(only)
        seen = []
        real = eng.closed_loop_vjp_device
        eng.closed_loop_vjp_device = lambda *p, **kw: (seen.append({n for n in OUTS + ("gmodel",) if kw.get(n) is not None}), real(*p, **kw))[1]
        got = dict(zip(names, torch.autograd.grad((G * xs).sum() + (H * us).sum() + (A * Xs).sum(), [lv[n] for n in names])))
        torch.cuda.synchronize()
        eng.synchronize()
        eng.close()
        assert len(seen) == 1 and seen[0] == (set(OUTS + ("gmodel",)) if only is None else {"gx0", "gmodel"})
        assert np.array_equal(_np(got["x0"]), g["gx0"], equal_nan=True) and torch.equal(got["Qd"], tot[0:10])
        if only is None:
            for n, m in (("xr", "gxr"), ("ur", "gur"), ("fp", "gfp")):
                assert np.array_equal(_np(got[n]), g[m], equal_nan=True), n
            assert got["f"].dtype == torch.float32 and np.array_equal(_np(got["f"]), g["gf"].astype(np.float32), equal_nan=True)
            assert torch.equal(got["Rd"], tot[10:14]) and torch.equal(got["mass"], (tot[14:15] + tot[15:16]).reshape(got["mass"].shape))
