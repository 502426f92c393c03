"""The closed loop chained through the torch layer, tick by tick, on the device (run with -m gpu): control_step_trajectory (ext form) or
control_step_ndp (ndp form) -> plant_step -> the next tick's x0, K = 3 ticks at N = 20, differentiated through all three ticks in ONE
graph and held to the composed float64 reference of tests/closed_loop_chain_ref.py.  CPU side: tests/test_closed_loop_chain.py.

A PARTIAL derivative, by the layer's contract: every tick's linearisation point (its pre-step iterate), final active set and gate are held
fixed.  The reference is therefore evaluated on the RECORD of the device's own nominal run (the same loop from update_device and
ndp_plant_step_device without autograd), and the finite differences of test 7 restore the recorded iterate and set before every tick.

    L = sum_k <G_k, x_{k+1}> + <H_k, u0_k> + <A_k, X_k>     (seeded normal G, H, A: every upstream of the step is live)

ext form: B = 65 (one vehicle past a full 64-lane plant workgroup), the mixed workload sliding along its figure-eights, a float32 force leaf
per tick; the reference is evaluated on six vehicles.  ndp form: B = 4, two stacked pairs, other_k = xr_k read through idx = i ^ 1, the
shipped weights as the leaf w; the reference on all four (the weights' gradient sums over them).  x_0 was chosen on the CPU with
closed_loop_chain_ref.nominal_cpu so that the conditions the tests assert hold: the referenced vehicles finish every tick on a set, one of
them has a stage-0 input on its bound in one tick and none in a later one, every gate is open and no network row is under the margin.

Link bars are the project's own: step 1e-9 max(1, |g|max) (tests/test_step_vjp_gpu.py), plant 1e-13 (plant_deriv_ref.within_bar), network
1e-5 (tests/test_downwash_vjp_gpu.py).  End to end the bar is ten times what the first device run measured (the POS_BAR convention; it
covers run-to-run differences in which instances round differently), as |dev - ref| / max(1, |ref|max of the leaf's row): MEASURED and
BAR below, and DESIGN section 9."""
import ctypes as C

import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import mlp_vjp_ref as MV
from tests import plant_deriv_ref as P
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.fixed_set_ref import scale

pytestmark = pytest.mark.gpu

# Measured on the first device run (MI355X), the worst per form over every leaf gradient (test 3) and every tangent (test 4):
#   ext  gradients x0 2.2e-13, xr 6.4e-14, ur 1.8e-13, f 5.1e-14, fp 1.1e-14; tangents dx 1.1e-13, du0 8.8e-13, dX 1.2e-12
#   ndp  gradients xr 5.1e-07, other 6.7e-07, w 4.3e-07 (the fp32 network's error, as its link shows it: g_z 6.7e-07); tangents 3.1e-07
# Both lie far under what the issue expected of the ext form (K step links at their OBSERVED 1e-10): the step link itself measures 1e-12
# of its scale on these inputs, not 1e-10.  The ndp leaves the network's backward does not reach (x_0, ur_k, fp_k: the network is a sink
# of the backward) go through the ext form's links alone, measured 4.5e-14, and are held to the ext bar -- tighter than the form's.
MEASURED = dict(ext=1.24e-12, ndp=6.72e-07)
BAR = {k: 10.0 * v for k, v in MEASURED.items()}

K, N, T = 3, 20, 2
B_EXT, SEED_EXT, SEED_NDP = 65, 20231516, 1
STEP_BAR, PLANT_BAR, NET_BAR, FD_BAR, VALUE_ATOL = 1e-9, 1e-13, 1e-5, 1e-6, 1e-6
LEAVES = dict(ext=("x0", "xr", "ur", "fp", "f"), ndp=("x0", "xr", "ur", "fp", "other", "w"))


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(form):
    return R.ext_inputs(B_EXT, K, N, SEED_EXT) if form == "ext" else R.ndp_inputs(K, SEED_NDP)


def _leaves(a, form, only=None):
    """The chain's leaves on the device.  only: the set of (name, tick) that require grad (None: all of them)."""
    import torch
    mk = lambda v, name, k=None, dt=None: _t(v, dt).requires_grad_(only is None or (name, k) in only)  # noqa: E731
    lv = dict(x0=mk(a["x0"], "x0"), xr=[mk(a["xr"][k], "xr", k) for k in range(K)], ur=[mk(a["ur"][k], "ur", k) for k in range(K)],
              fp=[mk(a["fp"][k], "fp", k) for k in range(K)])
    if form == "ext":
        lv["f"] = [mk(a["f"][k], "f", k, torch.float32) for k in range(K)]
    else:
        lv["other"] = [mk(a["other"][k], "other", k) for k in range(K)]
        lv["w"] = mk(a["blob"], "w", None, torch.float32)
        lv["idx"] = _t(a["idx"])
    return lv


def _engine(ndp, a, form):
    """A fresh engine: reset to tick 0's window and one warm-up step on tick 0's inputs, so that a kept set exists."""
    import torch
    B = a["x0"].shape[0]
    eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
    eng.reset(a["xr"][0], a["ur"][0])
    x0, xr, ur, u0 = _t(a["x0"]), _t(a["xr"][0]), _t(a["ur"][0]), torch.empty(B, 4, dtype=torch.float64, device=_dev())
    extra = dict(f=_t(a["f"][0], torch.float32)) if form == "ext" else dict(other=_t(a["other"][0]), ego_xy=x0[:, :2].contiguous(),
                                                                           other_index=_t(a["idx"]))
    torch.cuda.synchronize()
    eng.update_device(x0, xr, ur, u0, **extra)
    eng.synchronize()
    return eng


def _plain_loop(eng, a, form):
    """The chain without autograd, from update_device and ndp_plant_step_device: the device's record (closed_loop_chain_ref's layout)."""
    import torch
    B = a["x0"].shape[0]
    x = _t(a["x0"])
    idx = None if form == "ext" else _t(a["idx"])
    rec = {k: [] for k in ("x", "force", "Xpre", "Upre", "act_pre", "act", "u0", "X", "st", "it", "open")}
    for k in range(K):
        tape = eng.record_tape()
        xr, ur, fp, u0 = _t(a["xr"][k]), _t(a["ur"][k]), _t(a["fp"][k]), torch.empty(B, 4, dtype=torch.float64, device=_dev())
        extra = dict(f=_t(a["f"][k], torch.float32)) if form == "ext" else dict(other=_t(a["other"][k]), ego_xy=x[:, :2].contiguous(),
                                                                               other_index=idx)
        torch.cuda.synchronize()
        eng.update_device(x, xr, ur, u0, **extra)
        eng.synchronize()
        force = extra["f"] if form == "ext" else eng.device_force().clone()
        X = eng.device_iterate()[0].clone()
        xn = x.clone()
        torch.cuda.synchronize()
        st, it = eng.status()
        eng._check(eng._lib.ndp_plant_step_device(eng._h, C.c_void_p(xn.data_ptr()), C.c_void_p(u0.data_ptr()), C.c_void_p(fp.data_ptr()),
                                                  R.DT, R.SUBSTEPS, None), "ndp_plant_step_device")
        eng.synchronize()
        for name, v in (("x", _np(x)), ("force", _np(force).astype(np.float64)), ("Xpre", _np(tape[0])), ("Upre", _np(tape[1])),
                        ("act_pre", _np(tape[2])), ("act", eng.active_set()[1]), ("u0", _np(u0)), ("X", _np(X)), ("st", st), ("it", it),
                        ("open", np.ones(B, dtype=bool) if form == "ext" else R.gate_open(a["other"][k], a["idx"], _np(x)))):
            rec[name].append(v)
        x = xn
    rec["x"].append(_np(x))
    rec = {k: np.stack(v) for k, v in rec.items()}
    rec.update(xr=a["xr"], ur=a["ur"], fp=a["fp"], other=a.get("other"), idx=a.get("idx"), blob=a.get("blob"))
    return rec


def _chain(eng, lv, form, ups=None, hooks=None):
    """K ticks through the layer.  Returns (xs [K] of x_{k+1}, u0s, Xs, L or None); hooks: a dict that receives the upstream of every
    x_k ('x'), x_{k+1} ('xn'), u0_k and X_k, keyed (name, tick)."""
    from ndp_nmpc_qd_amd import torch_layer as TL
    x, xs, u0s, Xs = lv["x0"], [], [], []
    for k in range(K):
        if form == "ext":
            u0, X, U = TL.control_step_trajectory(eng, x, lv["xr"][k], lv["ur"][k], f=lv["f"][k])
        else:
            u0, X, U = TL.control_step_ndp(eng, x, lv["xr"][k], lv["ur"][k], lv["other"][k], ego_xy=x[:, :2].detach().contiguous(),
                                           weights=lv["w"], other_index=lv["idx"])
        xn = TL.plant_step(eng, x, u0, lv["fp"][k])
        if hooks is not None:
            for name, t in (("x", x), ("xn", xn), ("u0", u0), ("X", X)):
                t.register_hook(lambda g, key=(name, k): hooks.__setitem__(key, g.clone()))
        xs.append(xn); u0s.append(u0); Xs.append(X)
        x = xn
    L = None
    if ups is not None:
        G, H, A = ups
        L = sum((G[k] * xs[k]).sum() + (H[k] * u0s[k]).sum() + (A[k] * Xs[k]).sum() for k in range(K))
    return xs, u0s, Xs, L


def _grads(lv, form):
    """{leaf: numpy gradient, ticks stacked} of a chain's leaves (None where a leaf has none)."""
    g = lambda t: None if t.grad is None else _np(t.grad)  # noqa: E731
    out = {}
    for name in LEAVES[form]:
        v = lv[name]
        out[name] = g(v) if not isinstance(v, list) else [g(t) for t in v]
        if isinstance(v, list) and all(x is not None for x in out[name]):
            out[name] = np.stack(out[name])
    return out


def _instrument(eng, caught, drop_t):
    """The wrapper trick of test_control_step_ndp_end_to_end, on both derivative calls of the layer's backward: every step_vjp_device
    call's inputs and float64 outputs are kept (the layer hands f's gradient on in float32), and between the step's adjoint and the
    network's backward the gf is caught and the margin rule applied to it.  Calls arrive last tick first."""
    import torch
    real_step, real_net = eng.step_vjp_device, eng.downwash_vjp_device

    def step(x0, xr, ur, tape, **kw):
        real_step(x0, xr, ur, tape, **kw)
        eng.synchronize()
        caught["step"].append(dict({n: None if v is None or n == "stream" else v.clone() for n, v in kw.items()}, x0=x0, xr=xr, ur=ur, tape=tape))

    def net(other, ego_ref, gf, **kw):
        k = K - 1 - len(caught["net"]) % K
        raw = gf.clone()
        gf[drop_t[k] & torch.isfinite(gf).all(dim=2)] = 0.0
        real_net(other, ego_ref, gf, **kw)
        eng.synchronize()
        caught["net"].append(dict(raw=raw, gf=gf.clone(), gz=None if kw.get("gz") is None else kw["gz"].clone(),
                                  gw=None if kw.get("gw") is None else kw["gw"].clone()))
    eng.step_vjp_device, eng.downwash_vjp_device = step, net
    return real_step


@pytest.fixture(scope="module")
def shared():
    """The cache of `full`, one entry per form; its instrumented engines stay open for test 2's direct calls and are closed at the end."""
    cache = {}
    yield cache
    for r in cache.values():
        r["eng"].close()


def _pick(rec, ok, n=6):
    """The referenced vehicles: up to two set finishes with a stage-0 input on its bound in one tick and none in a later one, then free
    ones, then the first others."""
    pin0 = rec["act"][:, :, 0, :].any(axis=2)
    first = [v for v in np.flatnonzero(ok) if any(pin0[k, v] and (~pin0[k + 1:, v]).any() for k in range(K - 1))][:2]
    free = [v for v in np.flatnonzero(ok) if not rec["act"][:, v].any()]
    rest = [v for v in np.flatnonzero(ok) if v not in first and v not in free]
    return sorted(int(v) for v in (first + free + rest)[:n])


def full(ndp, oracle, form, cache):
    """Everything the tests of one form share, computed once and left unchanged: the inputs, the CPU nominal run, the device's record from
    the plain loop, the referenced vehicles and their reference systems, and ONE instrumented run of the chain and its backward on torch's
    default stream (outputs, caught upstreams, leaf gradients)."""
    if form in cache:
        return cache[form]
    import torch
    a = _inputs(form)
    B = a["x0"].shape[0]
    kw = dict(f=a["f"]) if form == "ext" else dict(other=a["other"], idx=a["idx"], blob=a["blob"])
    cpu = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], **kw)
    eng = _engine(ndp, a, form)
    rec = _plain_loop(eng, a, form)
    eng.close()
    ok = R.set_finish(rec)
    which = list(range(B)) if form == "ndp" else _pick(cpu, R.set_finish(cpu))
    drop = None if form == "ext" else R.margins(a["blob"], a["other"], a["xr"], a["idx"]) < MV.MARGIN
    ups_np = R.upstreams(K, B, N, seed=31)
    ups = tuple(_t(v) for v in ups_np)
    eng = _engine(ndp, a, form)
    lv = _leaves(a, form)
    caught, hooks = dict(step=[], net=[]), {}
    real_step = _instrument(eng, caught, None if drop is None else _t(drop))
    xs, u0s, Xs, L = _chain(eng, lv, form, ups, hooks)
    after_fwd = [_np(v) for v in eng.device_iterate()] + [eng.active_set()[1]]
    L.backward(retain_graph=True)
    torch.cuda.synchronize()
    eng.synchronize()
    after_bwd = [_np(v) for v in eng.device_iterate()] + [eng.active_set()[1]]
    r = dict(a=a, B=B, cpu=cpu, rec=rec, ok=ok, which=which, drop=drop, ups=ups_np, ups_t=ups, lv=lv, eng=eng, real_step=real_step, L=L,
             xs=np.stack([_np(v) for v in xs]), u0s=np.stack([_np(v) for v in u0s]), Xs=np.stack([_np(v) for v in Xs]),
             caught=caught, hooks={k: _np(v) for k, v in hooks.items()}, grads=_grads(lv, form), after_fwd=after_fwd, after_bwd=after_bwd)
    if ok[which].all():                 # (otherwise test_the_inputs_meet_their_conditions fails, and says why)
        r["sys"] = R.systems(oracle, rec, which)
        r["ref"] = R.reverse(r["sys"], rec, *ups_np, drop=drop)
    cache[form] = r
    return r


def _f64_gf(r):
    """[K,B,N+1,3]: the step's float64 gf of every tick, as caught (ext: what the layer rounds to the float32 leaf's gradient)."""
    return np.stack([_np(r["caught"]["step"][K - 1 - k]["gf"]) for k in range(K)])


FORMS = ["ext", "ndp"]


# ---- 0. the conditions on the inputs
@pytest.mark.parametrize("form", FORMS)
def test_the_inputs_meet_their_conditions(ndp, oracle, shared, form):
    """Conditions on the inputs, none of which loosens a bar: every referenced (vehicle, tick) is a status-0 set finish without an
    interior-point iteration, on the CPU and on the device; ext: a referenced vehicle has a stage-0 input on its bound in one tick and a
    later tick with none, and at most a quarter of the 65 are no set finishes on the device (they are reported and left out of the
    batch-wide checks); ndp: all four gates open at every tick, at most MAX_DROPPED of the network rows under MARGIN."""
    r = full(ndp, oracle, form, shared)
    rec, which, ok = r["rec"], r["which"], r["ok"]
    print(f"{form}: {int((~ok).sum())} of {r['B']} vehicles are no set finishes on the device: {np.flatnonzero(~ok).tolist()}; referenced {which}")
    assert R.set_finish(r["cpu"])[which].all() and ok[which].all()
    assert np.array_equal(rec["act"][:, which], r["cpu"]["act"][:, which])
    if form == "ext":
        assert len(which) == 6 and (~ok).sum() <= B_EXT // 4
        pin0 = rec["act"][:, :, 0, :].any(axis=2)
        assert any(pin0[k, v] and (~pin0[k + 1:, v]).any() for v in which for k in range(K - 1))
    else:
        assert rec["open"].all() and r["cpu"]["open"].all()
        assert float(r["drop"].mean()) <= MV.MAX_DROPPED


# ---- 1. values
@pytest.mark.parametrize("form", FORMS)
def test_values_are_the_plain_loops_bits_and_the_oracles_closed_loop(ndp, oracle, shared, form):
    """x_{k+1}, u0_k, X_k of the chain are bit-equal to the same loop from update_device and ndp_plant_step_device without autograd on a
    fresh engine, and within atol 1e-6 (test_gpu_closed_loop_matches_oracle_closed_loop's) of the oracle's loop on the set finishes."""
    r = full(ndp, oracle, form, shared)
    rec, cpu = r["rec"], r["cpu"]
    assert np.array_equal(r["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(r["u0s"], rec["u0"], equal_nan=True)
    assert np.array_equal(r["Xs"], rec["X"], equal_nan=True)
    both = r["ok"] & R.set_finish(cpu)
    for name, dev, ref in (("x", rec["x"][1:], cpu["x"][1:]), ("u0", rec["u0"], cpu["u0"]), ("X", rec["X"], cpu["X"])):
        err = float(np.abs(dev[:, both] - ref[:, both]).max())
        print(f"{form}: {name} against the oracle's loop, worst absolute difference {err:.2e} on {int(both.sum())} vehicles")
        assert err <= VALUE_ATOL, (name, err)


# ---- 2. link by link
@pytest.mark.parametrize("form", FORMS)
def test_every_link_meets_its_own_bar_on_the_chains_upstream(ndp, oracle, shared, form):
    """The upstream of every link is caught on the way (register_hook on every x_k, u0_k, X_k; the wrappers of _instrument for the
    float64 gf), the reference link is fed the device's own upstream, and the link's output must meet that link's project bar: step
    1e-9 max(1, |g|max), plant 1e-13 (within_bar), network 1e-5.  A stage-0 input on its bound passes exactly 0 upstream: an upstream on
    that component alone gives exact zeros in every output of the step's adjoint, and its ur entry's gradient is exactly 0."""
    import torch
    r = full(ndp, oracle, form, shared)
    rec, which, sys_, hooks, eng, a = r["rec"], r["which"], r["sys"], r["hooks"], r["eng"], r["a"]
    G, H, A = r["ups"]
    B = r["B"]
    worst = dict(step=0.0, plant=0.0, gz=0.0, gw=0.0)
    n_pinned = 0
    for k in range(K):
        c = r["caught"]["step"][K - 1 - k]
        gu0, gX = _np(c["gu0"]), _np(c["gX"])
        assert np.array_equal(gu0, hooks[("u0", k)], equal_nan=True) and np.array_equal(gX, hooks[("X", k)]) and np.array_equal(gX, A[k])
        assert np.array_equal(_np(c["x0"]), rec["x"][k], equal_nan=True) and np.array_equal(_np(c["tape"][0]), rec["Xpre"][k], equal_nan=True)
        assert np.array_equal(_np(c["tape"][2]), rec["act_pre"][k])
        # the plant link, by a direct call on the device's own upstream of x_{k+1}
        x, u0, xn, fp = (_t(v) for v in (rec["x"][k], rec["u0"][k][None], rec["x"][k + 1][None], a["fp"][k][None]))
        out = [torch.full(s, -7.0, dtype=torch.float64, device=_dev()) for s in ((B, 10), (1, B, 4), (1, B, 3))]
        torch.cuda.synchronize()
        eng.plant_rollout_vjp_device(x, u0, xn, _t(hooks[("xn", k)][None]), f=fp, gx0=out[0], gu=out[1], gf=out[2], dt=R.DT, substeps=R.SUBSTEPS)
        eng.synchronize()
        gx_p, gu_p, gfp = _np(out[0]), _np(out[1])[0], _np(out[2])[0]
        assert np.array_equal(gfp, r["grads"]["fp"][k], equal_nan=True)                       # the leaf's gradient IS this call's
        for dev, ref in zip((gx_p, gu_p, gfp), R.plant_link(sys_, k, hooks[("xn", k)][which])):
            okb, ratio = P.within_bar(dev[which], ref, PLANT_BAR)
            worst["plant"] = max(worst["plant"], ratio)
            assert okb, ("plant", k, ratio)
        assert np.array_equal(hooks[("u0", k)][r["ok"]], (H[k] + gu_p)[r["ok"]])                # g_u0 = H_k + the plant's gu, nothing else
        # the step link
        ref = R.step_link(sys_, k, gu0[which], gX[which])
        got = [_np(c[n])[which] for n in ("gx0", "gxr", "gur", "gf")]
        if form == "ndp":                                                                      # (kept before xr's share of the network)
            assert np.array_equal(_np(r["caught"]["net"][K - 1 - k]["raw"]), _np(c["gf"]), equal_nan=True)
        for j in range(len(which)):
            s = max(scale(x[j]) for x in ref)
            for dev, x in zip(got, ref):
                e = float(np.max(np.abs(dev[j] - x[j]))) / s
                worst["step"] = max(worst["step"], e)
                assert e <= STEP_BAR, ("step", k, which[j], e)
        if form == "ext":
            assert np.array_equal(r["grads"]["f"][k], _np(c["gf"]).astype(np.float32), equal_nan=True)
            assert np.array_equal(r["grads"]["xr"][k], _np(c["gxr"]), equal_nan=True)
        assert np.array_equal(r["grads"]["ur"][k], _np(c["gur"]), equal_nan=True)
        # a pinned stage-0 input passes exactly 0 upstream
        act = rec["act"][k]
        assert not r["grads"]["ur"][k][r["ok"]][act[r["ok"]] != 0].any()
        pin0 = (act[:, 0, :] != 0) & r["ok"][:, None]
        if pin0.any():
            only = np.where(pin0, np.where(gu0 == 0.0, 1.0, gu0), 0.0)
            o = [torch.full(s, -7.0, dtype=torch.float64, device=_dev()) for s in ((B, 10), (B, N + 1, 10), (B, N, 4), (B, N + 1, 3))]
            torch.cuda.synchronize()
            r["real_step"](c["x0"], c["xr"], c["ur"], c["tape"], gu0=_t(only), f=c["f"], gx0=o[0], gxr=o[1], gur=o[2], gf=o[3])
            eng.synchronize()
            rows = pin0.any(axis=1)
            n_pinned += int(rows.sum())
            for t in o:
                assert (_np(t)[rows] == 0.0).all()
        # the network link
        if form == "ndp":
            nrec = r["caught"]["net"][K - 1 - k]
            gf = _np(nrec["gf"]) * rec["open"][k][:, None, None]
            z = R.net_rows(a["other"][k], a["xr"][k], a["idx"])
            rz, rw, _, _ = MV.vjp64(a["blob"], z.reshape(-1, 6), gf.reshape(-1, 3))
            rz = rz.reshape(B, N + 1, 6)
            e = float((np.abs(_np(nrec["gz"]) - rz).max(axis=2) / np.maximum(1.0, np.abs(rz).max(axis=2))).max())
            ge = max(MV.group_errors(_np(nrec["gw"]), rw).values())
            worst["gz"], worst["gw"] = max(worst["gz"], e), max(worst["gw"], ge)
            assert e <= NET_BAR and ge <= NET_BAR, ("network", k, e, ge)
            assert np.array_equal(_np(c["gxr"])[:, :, 6:], r["grads"]["xr"][k][:, :, 6:])
    print(f"{form}: worst link errors (share of each link's bar's scale) " + " ".join(f"{n} {v:.2e}" for n, v in worst.items())
          + f"; {n_pinned} (vehicle, tick) with a stage-0 input on its bound")
    if form == "ext":
        assert n_pinned >= 1


# ---- 3. end to end
@pytest.mark.parametrize("form", FORMS)
def test_every_leaf_gradient_matches_the_independent_reverse_sweep(ndp, oracle, shared, form):
    """Every leaf's gradient against closed_loop_chain_ref.reverse on the device's record, as |dev - ref| / max(1, |ref|max of the leaf's
    row) (a row: one vehicle's share of one tick's leaf; the weights: the whole vector).  ext's float32 leaf f is compared through the
    float64 gf the layer rounds (test 2 holds the leaf to its rounding, bit for bit).  Bars: BAR at the top of this file."""
    r = full(ndp, oracle, form, shared)
    which, ref, g = r["which"], r["ref"], r["grads"]
    e = dict(x0=R.rel_err(g["x0"][which], ref["x0"], 1), ur=R.rel_err(g["ur"][:, which], ref["ur"], 2), fp=R.rel_err(g["fp"][:, which], ref["fp"], 2))
    if form == "ext":
        e["xr"] = R.rel_err(g["xr"][:, which], ref["xr"], 2)
        e["f"] = R.rel_err(_f64_gf(r)[:, which], ref["f"], 2)
        groups = dict(ext=e)
    else:
        net = dict(xr=R.rel_err(g["xr"][:, which], ref["xr"], 2), other=R.rel_err(g["other"], ref["other"], 2), w=R.rel_err(g["w"], ref["w"], 0))
        groups = dict(ext=e, ndp=net)       # (x_0, ur_k, fp_k: the ext form's links alone, held to its bar)
        ge = MV.group_errors(g["w"], ref["w"])
        print("ndp: weights by parameter group " + " ".join(f"{n} {v:.2e}" for n, v in ge.items()))
        assert max(ge.values()) <= NET_BAR
        assert not g["other"][:, :, :, 6:].any()
    for name, errs in groups.items():
        print(f"{form}, held to the {name} bar: measured " + " ".join(f"{n} {v:.3e}" for n, v in errs.items())
              + f"; worst {max(errs.values()):.3e}, bar {BAR[name]:.1e}")
    for name, errs in groups.items():
        assert max(errs.values()) <= BAR[name], (name, errs)


# ---- 4. forward mode chained by hand
@pytest.mark.parametrize("form", FORMS)
def test_forward_mode_chained_by_hand(ndp, oracle, shared, form):
    """control_step_jvp (ext) / control_step_ndp_jvp (ndp) into plant_rollout_jvp with ticks = 1, tick by tick, T = 2 seeded directions of
    every leaf: values bit-equal to the reverse-mode chain's forward; tangents held to closed_loop_chain_ref.forward at test 3's bars,
    measured the same way; duality with the device's reverse chain within K x 1e-10 of the largest term for the ext form (one step-link
    gap of test_duality_with_the_adjoint_on_the_device per tick; the plant's 1e-12 is negligible), and within 2e-5 for the ndp form (both
    network passes are held to one float64 network at 1e-5)."""
    from ndp_nmpc_qd_amd import torch_layer as TL
    r = full(ndp, oracle, form, shared)
    a, B, which, rec = r["a"], r["B"], r["which"], r["rec"]
    t = R.tangents(K, B, N, T, seed=41, rows=None if form == "ext" else a["other"].shape[1])
    if form == "ndp":
        assert not r["drop"].any()          # (forward mode has no place for the margin rule: the inputs leave no row under the margin)
    eng = _engine(ndp, a, form)
    lv = _leaves(a, form, only=set())
    x, tx = lv["x0"], _t(t["t_x0"])
    dx, du0s, dXs, vals = [], [], [], []
    for k in range(K):
        if form == "ext":
            u0, X, U, du0, dX, dU = TL.control_step_jvp(eng, x, lv["xr"][k], lv["ur"][k], (tx, _t(t["t_xr"][k]), _t(t["t_ur"][k]), _t(t["t_f"][k])),
                                                        f=lv["f"][k])
        else:
            u0, X, U, du0, dX, dU = TL.control_step_ndp_jvp(eng, x, lv["xr"][k], lv["ur"][k], lv["other"][k],
                                                            (tx, _t(t["t_xr"][k]), _t(t["t_ur"][k]), _t(t["t_other"][k]), _t(t["t_w"])),
                                                            ego_xy=x[:, :2].contiguous(), weights=lv["w"], other_index=lv["idx"])
        xs, dxs = TL.plant_rollout_jvp(eng, x, u0[None], (tx, du0[None].contiguous(), _t(t["t_fp"][k][None])), f=lv["fp"][k][None])
        x, tx = xs[0], dxs[0].contiguous()
        vals.append((_np(x), _np(u0), _np(X)))
        dx.append(_np(tx)); du0s.append(_np(du0)); dXs.append(_np(dX))
    eng.close()
    for k in range(K):
        for got, want in zip(vals[k], (r["xs"][k], r["u0s"][k], r["Xs"][k])):
            assert np.array_equal(got, want, equal_nan=True)
    dx, du0s, dXs = np.stack(dx), np.stack(du0s), np.stack(dXs)
    kw = dict(t_f=t["t_f"]) if form == "ext" else dict(t_other=t["t_other"], t_w=t["t_w"])
    rx, ru, rX = R.forward(r["sys"], rec, t["t_x0"], t["t_xr"], t["t_ur"], t["t_fp"], **kw)
    errs = dict(dx=R.rel_err(dx[:, which], rx, 3), du0=R.rel_err(du0s[:, which], ru, 3), dX=R.rel_err(dXs[:, which], rX, 3))
    bar = BAR[form]
    print(f"{form}: tangents, measured " + " ".join(f"{n} {v:.3e}" for n, v in errs.items()) + f"; bar {bar:.1e}")
    # duality with the reverse chain, per vehicle and direction
    G, H, A = r["ups"]
    g = r["grads"]
    lhs = np.einsum("kvtc,kvc->vt", dx, G) + np.einsum("kvtc,kvc->vt", du0s, H) + np.einsum("kvtnc,kvnc->vt", dXs, A)
    terms = [np.einsum("vtc,vc->vt", t["t_x0"], g["x0"]), np.einsum("kvtnc,kvnc->vt", t["t_xr"], g["xr"]),
             np.einsum("kvtnc,kvnc->vt", t["t_ur"], g["ur"]), np.einsum("kvtc,kvc->vt", t["t_fp"], g["fp"])]
    if form == "ext":
        terms.append(np.einsum("kvtnc,kvnc->vt", t["t_f"], _f64_gf(r)))
        rhs = np.sum(terms, axis=0)
        big = np.maximum(np.abs(np.array(terms)).max(axis=0), np.abs(lhs))
        gap = (np.abs(lhs - rhs) / big)[r["ok"]]
        lim = K * 1e-10
    else:                                   # other_k and w couple the vehicles: one sum over all four
        tot = [float(x.sum(axis=0)[0]) for x in terms], [float(x.sum(axis=0)[1]) for x in terms]
        extra = [np.einsum("krtnc,krnc->t", t["t_other"], g["other"]), t["t_w"].astype(np.float64) @ g["w"].astype(np.float64)]
        rhs = np.array([sum(tot[i]) + extra[0][i] + extra[1][i] for i in range(T)])
        big = np.array([max(np.abs(tot[i] + [extra[0][i], extra[1][i], lhs.sum(axis=0)[i]])) for i in range(T)])
        gap = np.abs(lhs.sum(axis=0) - rhs) / big
        lim = 2e-5
    print(f"{form}: duality of the hand-chained forward mode with the reverse chain, worst gap {gap.max():.3e} of the largest term (bar {lim:.0e})")
    assert max(errs.values()) <= bar, errs
    assert gap.max() <= lim


# ---- 5. order, streams, state
@pytest.mark.parametrize("form", FORMS)
def test_streams_repeats_and_engine_state(ndp, oracle, shared, form):
    """The whole chain and its backward on a side stream (a stream the C-ABI can name) give the default-stream run's gradients bit for
    bit; a second backward over the retained graph is bit-identical; the engine's iterate and kept set after the backward are those after
    the forward."""
    import torch
    r = full(ndp, oracle, form, shared)
    for x, y in zip(r["after_fwd"], r["after_bwd"]):
        assert np.array_equal(x, y, equal_nan=True)
    lv = r["lv"]
    for name in LEAVES[form]:
        for t in (lv[name] if isinstance(lv[name], list) else [lv[name]]):
            t.grad = None
    r["L"].backward(retain_graph=True)                       # (the instrumented engine: same calls, same order)
    torch.cuda.synchronize()
    again = _grads(lv, form)
    for name in LEAVES[form]:
        assert np.array_equal(again[name], r["grads"][name], equal_nan=True), name
    a = r["a"]
    eng = _engine(ndp, a, form)
    lv2 = _leaves(a, form)
    side = torch.cuda.Stream(device=_dev())
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        xs, u0s, Xs, L = _chain(eng, lv2, form, r["ups_t"])
        L.backward()
    side.synchronize()
    torch.cuda.synchronize()
    for k in range(K):
        assert np.array_equal(_np(xs[k]), r["xs"][k], equal_nan=True) and np.array_equal(_np(Xs[k]), r["Xs"][k], equal_nan=True)
    got = _grads(lv2, form)
    eng.close()
    for name in LEAVES[form]:
        assert np.array_equal(got[name], r["grads"][name], equal_nan=True), name


def test_tapes_survive_later_steps_and_other_weights_are_refused(ndp, oracle, shared):
    """ndp form: one more forward step with the same weights tensor between the chain's forward and its backward leaves the chain's
    gradients bit-unchanged (the tapes are the chain's own; the installed weights are still these); the same with another weights tensor
    makes the backward raise _check_installed's error."""
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    r = full(ndp, oracle, "ndp", shared)
    a = r["a"]
    for other_w in (False, True):
        eng = _engine(ndp, a, "ndp")
        lv = _leaves(a, "ndp")
        xs, u0s, Xs, L = _chain(eng, lv, "ndp", r["ups_t"])
        w = _t(a["blob"] * np.float32(1.01), torch.float32) if other_w else lv["w"]
        with torch.no_grad():
            TL.control_step_ndp(eng, xs[-1].detach(), lv["xr"][K - 1].detach(), lv["ur"][K - 1].detach(), lv["other"][K - 1].detach(),
                                ego_xy=xs[-1][:, :2].detach().contiguous(), weights=w, other_index=lv["idx"])
        if other_w:
            with pytest.raises(RuntimeError, match="network weights were replaced"):
                L.backward()
        else:
            L.backward()
            torch.cuda.synchronize()
            got = _grads(lv, "ndp")
            for name in LEAVES["ndp"]:
                assert np.array_equal(got[name], r["grads"][name], equal_nan=True), name
        torch.cuda.synchronize()
        eng.close()


# ---- 6. which leaves need a gradient
@pytest.mark.parametrize("form", FORMS)
def test_only_two_leaves_require_grad(ndp, oracle, shared, form):
    """Only x_0 and tick 1's ur_1 require grad, everything else is detached (needs_input_grad differs from tick to tick: tick 0 owes x_0
    alone, tick 1 x_1 and ur_1, tick 2 x_2 alone): their gradients are the full run's, bit for bit."""
    import torch
    r = full(ndp, oracle, form, shared)
    a = r["a"]
    eng = _engine(ndp, a, form)
    lv = _leaves(a, form, only={("x0", None), ("ur", 1)})
    xs, u0s, Xs, L = _chain(eng, lv, form, r["ups_t"])
    L.backward()
    torch.cuda.synchronize()
    eng.synchronize()
    eng.close()
    assert np.array_equal(_np(lv["x0"].grad), r["grads"]["x0"], equal_nan=True)
    assert np.array_equal(_np(lv["ur"][1].grad), r["grads"]["ur"][1], equal_nan=True)
    for name in LEAVES[form]:
        for k, t in enumerate(lv[name] if isinstance(lv[name], list) else [lv[name]]):
            assert t.grad is None or (name, k) in (("x0", 0), ("ur", 1))


def test_a_nan_state_stays_with_its_vehicle(ndp, oracle, shared):
    """ndp form, vehicle 1 given a NaN velocity entry at tick 0: its own gradients are NaN, it contributes nothing to the weights'
    gradient (finite, and the float64 reverse sweep over the other three vehicles within the network's bar), and every other vehicle's
    gradients are bit-unchanged.  (The neighbour row vehicle 1 reads, other_k[0], hears its NaN.)"""
    import torch
    r = full(ndp, oracle, "ndp", shared)
    a = dict(r["a"])
    bad, rest = 1, [0, 2, 3]
    a["x0"] = a["x0"].copy()
    a["x0"][bad, 3] = np.nan
    eng = _engine(ndp, a, "ndp")
    lv = _leaves(a, "ndp")
    real, drop_t = eng.downwash_vjp_device, _t(r["drop"])
    seen = []

    def margin_rule(other_, ego_ref_, gf_, **kw):
        gf_[drop_t[K - 1 - len(seen)] & torch.isfinite(gf_).all(dim=2)] = 0.0
        seen.append(1)
        return real(other_, ego_ref_, gf_, **kw)
    eng.downwash_vjp_device = margin_rule
    xs, u0s, Xs, L = _chain(eng, lv, "ndp", r["ups_t"])
    L.backward()
    torch.cuda.synchronize()
    eng.synchronize()
    st = eng.status()[0]
    eng.close()
    g, full_g = _grads(lv, "ndp"), r["grads"]
    assert st[bad] != 0 and not st[rest].any()
    assert np.isnan(g["x0"][bad]).all() and np.isnan(g["xr"][:, bad]).all() and np.isnan(g["ur"][:, bad]).all()
    for name in ("x0",):
        assert np.array_equal(g[name][rest], full_g[name][rest])
    for name in ("xr", "ur", "fp"):
        assert np.array_equal(g[name][:, rest], full_g[name][:, rest]), name
    assert np.array_equal(g["other"][:, [1, 2, 3]], full_g["other"][:, [1, 2, 3]])           # rows read by vehicles 0, 3, 2
    assert np.isfinite(g["w"]).all()
    sub = dict(r["sys"], which=rest, J=[J[rest] for J in r["sys"]["J"]], S=[[S[v] for v in rest] for S in r["sys"]["S"]])
    ref_w = R.reverse(sub, r["rec"], *r["ups"], drop=r["drop"])["w"]
    ge = MV.group_errors(g["w"], ref_w)
    print("weights' gradient without the NaN vehicle, by group " + " ".join(f"{n} {v:.2e}" for n, v in ge.items()))
    assert max(ge.values()) <= NET_BAR
    assert max(MV.group_errors(full_g["w"], ref_w).values()) > 1e-3                          # (vehicle 1's share was not small)


# ---- 7. device finite differences
def test_device_finite_differences_of_the_chained_loss(ndp, oracle, shared):
    """ext form: central differences of L over the device's own closed loop in two entries each of x_0, xr_1, ur_2, f_0 and fp_1 (steps
    1e-6; 2^-14 on the float32 f), every tick of every perturbed run restarted from the recorded iterate and kept set (set_iterate,
    set_active_set), against the chain's gradients: within 1e-6 of max(1, |g|) on the vehicles whose sets and iteration words do not move
    in any run, at least 40 of the 65."""
    r = full(ndp, oracle, "ext", shared)
    a, rec, g = r["a"], r["rec"], r["grads"]
    G, H, A = r["ups"]
    eng = ndp.BatchedNMPC(B_EXT, N=N, disturbance=True)
    eng.reset(a["xr"][0], a["ur"][0])
    cases = [("x0", None, (2,), 1e-6), ("x0", None, (8,), 1e-6), ("xr", 1, (5, 1), 1e-6), ("xr", 1, (12, 7), 1e-6), ("ur", 2, (0, 3), 1e-6),
             ("ur", 2, (9, 0), 1e-6), ("f", 0, (0, 2), 2.0 ** -14), ("f", 0, (11, 0), 2.0 ** -14), ("fp", 1, (0,), 1e-6), ("fp", 1, (2,), 1e-6)]
    stable = r["ok"].copy()
    fds = []
    for name, k, at, h in cases:
        L = []
        for sgn in (1.0, -1.0):
            p = {n: np.array(a[n]) for n in ("x0", "xr", "ur", "f", "fp")}
            (p[name] if k is None else p[name][k])[(slice(None),) + at] += (np.float32 if name == "f" else np.float64)(sgn * h)
            x, tot = p["x0"], np.zeros(B_EXT)
            for j in range(K):
                eng.set_iterate(rec["Xpre"][j], rec["Upre"][j])
                eng.set_active_set(rec["act_pre"][j])
                u, X, U, st, it = eng.update(x, p["xr"][j], p["ur"][j], f=p["f"][j], raise_on_status=False, full=True)
                stable &= (st == 0) & ((it & 0xffff) == 0) & (eng.active_set()[1] == rec["act"][j]).all(axis=(1, 2))
                x = eng.plant_step(x, u, p["fp"][j], dt=R.DT, substeps=R.SUBSTEPS)
                tot += (G[j] * x).sum(axis=1) + (H[j] * u).sum(axis=1) + (A[j] * X).sum(axis=(1, 2))
            L.append(tot)
        fds.append((L[0] - L[1]) / (2 * h))
    eng.close()
    print(f"{int(stable.sum())} of {B_EXT} vehicles keep their sets and iteration words in every run")
    assert stable.sum() >= 40
    worst = 0.0
    for (name, k, at, h), fd in zip(cases, fds):
        got = (g[name] if k is None else g[name][k])[(slice(None),) + at].astype(np.float64)
        err = float((np.abs(fd - got)[stable] / np.maximum(1.0, np.abs(got[stable]))).max())
        worst = max(worst, err)
        assert err <= FD_BAR, (name, k, at, err)
    print(f"worst |fd - g| / max(1, |g|) = {worst:.2e}")
