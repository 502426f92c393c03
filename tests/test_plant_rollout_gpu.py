"""ndp_plant_rollout_device, ndp_plant_rollout_vjp_device, ndp_plant_rollout_jvp_device and their torch layer on the device, against
ndp_plant_step_device (bits) and the float64 complex-step reference of tests/plant_deriv_ref.py (the project's plant bar, 1e-13 of
max(1, the row's largest reference entry), no row left out).

Shapes: B in {1, 64, 257} (one lane; one full wave; a last workgroup that holds a single lane), ticks in {1, 3}, substeps in {1, 4, 16}
(the bounds of NDP_PLANT_MAX_SUBSTEPS and the default), with a force and without -- CASES touches every value, not the whole product."""
import ctypes as C

import numpy as np
import pytest

from ndp_nmpc_qd_amd.params import nmpc_params as CP
from tests import plant_deriv_ref as P

pytestmark = pytest.mark.gpu

DT = CP.ts_nmpc
CASES = [(1, 1, 1, True), (64, 3, 4, False), (257, 3, 16, True), (257, 1, 4, False)]       # (B, ticks, substeps, force)
_ENG, _REF = {}, {}


def engine(B):
    import ndp_nmpc_qd_amd as ndp
    if B not in _ENG:
        _ENG[B] = ndp.BatchedNMPC(B, load_mlp=False)
    return _ENG[B]


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64, order="C", copy=True)).cuda()


def filled(*shape):
    import torch
    return torch.full(shape, -7.0, dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy()


def run(eng, call):
    """The engine's own stream (stream=None) behind everything torch has enqueued, and the host behind it."""
    import torch
    torch.cuda.synchronize()
    call()
    eng.synchronize()


def reference(case):
    """Inputs, the reference Jacobian and upstream / tangent draws of a case: computed once, shared, never written."""
    if case not in _REF:
        B, ticks, sub, force = case
        eng = engine(B)
        x0, u, f = P.inputs(B, ticks, seed=100 + B + ticks + sub, force=force)
        J = P.jacobian(x0, u, f, DT, sub, eng.cfg.mass, eng.cfg.gravity)
        rng = np.random.default_rng(7)
        T = 8
        r = dict(x0=x0, u=u, f=f, J=J, g=rng.normal(size=(ticks, B, 10)), tx0=rng.normal(size=(B, T, 10)),
                 tu=rng.normal(size=(ticks, B, T, 4)), tf=rng.normal(size=(ticks, B, T, 3)))
        for v in r.values():
            if v is not None:
                v.setflags(write=False)
        _REF[case] = r
    return _REF[case]


def forward(eng, x0, u, f, sub):
    xs = filled(u.shape[0], eng.B, 10)
    run(eng, lambda: eng.plant_rollout_device(x0, u, xs, f=f, dt=DT, substeps=sub))
    return xs


def vjp(eng, x0, u, f, xs, g, sub, want=(True, True, True)):
    K, B = u.shape[0], eng.B
    out = [filled(*s) if w else None for w, s in zip(want, ((B, 10), (K, B, 4), (K, B, 3)))]
    run(eng, lambda: eng.plant_rollout_vjp_device(x0, u, xs, g, f=f, gx0=out[0], gu=out[1], gf=out[2], dt=DT, substeps=sub))
    return out


def jvp(eng, x0, u, f, sub, tx0=None, tu=None, tf=None, check=False):
    K, B = u.shape[0], eng.B
    T = next(t.shape[-2] for t in (tx0, tu, tf) if t is not None)
    dxs, xc = filled(K, B, T, 10), filled(K, B, 10) if check else None
    run(eng, lambda: eng.plant_rollout_jvp_device(x0, u, dxs, f=f, tx0=tx0, tu=tu, tf=tf, xs_check=xc, dt=DT, substeps=sub))
    return dxs, xc


# ---- 1. the forward's bits
@pytest.mark.parametrize("case", [(64, 3, 4, False), (257, 3, 16, True), (1, 3, 1, True), (257, 3, 4, False)])
def test_log_rows_are_successive_plant_steps_bit_for_bit(case):
    B, ticks, sub, force = case
    eng = engine(B)
    x0, u, f = P.inputs(B, ticks, seed=11 + B, force=force)
    dx0, du, df = dev(x0), dev(u), dev(f)
    xs = host(forward(eng, dx0, du, df, sub))
    x = dx0.clone()
    for k in range(ticks):
        fk = None if df is None else C.c_void_p(df[k].data_ptr())
        run(eng, lambda: eng._check(eng._lib.ndp_plant_step_device(eng._h, C.c_void_p(x.data_ptr()), C.c_void_p(du[k].data_ptr()), fk,
                                                                   DT, sub, None), "ndp_plant_step_device"))
        assert np.array_equal(xs[k], host(x)), k
    assert np.isfinite(xs).all() and np.abs(np.linalg.norm(xs[..., 6:], axis=-1) - 1).max() < 1e-14
    # once more with d_x0 = the last tick's slot of the log
    log = filled(ticks, B, 10)
    log[ticks - 1].copy_(dx0)
    run(eng, lambda: eng.plant_rollout_device(log[ticks - 1], du, log, f=df, dt=DT, substeps=sub))
    assert np.array_equal(host(log), xs)


# ---- 2. reverse and forward mode against the reference
@pytest.mark.parametrize("case", CASES)
def test_vjp_and_jvp_against_the_complex_step_reference(case):
    B, ticks, sub, force = case
    eng, r = engine(B), reference(case)
    x0, u, f = dev(r["x0"]), dev(r["u"]), dev(r["f"])
    xs = forward(eng, x0, u, f, sub)
    got = vjp(eng, x0, u, f, xs, dev(r["g"]), sub)
    for name, dv, rf in zip(("gx0", "gu", "gf"), got, P.vjp(r["J"], r["g"])):
        ok, ratio = P.within_bar(host(dv), rf)
        print(case, name, "worst |dev - ref| / max(1, row max):", ratio)
        assert ok, (name, ratio)
    dxs, _ = jvp(eng, x0, u, f, sub, dev(r["tx0"]), dev(r["tu"]), dev(r["tf"]))
    ok, ratio = P.within_bar(host(dxs), P.jvp(r["J"], r["tx0"], r["tu"], r["tf"]))
    print(case, "dxs worst:", ratio)
    assert ok, ratio
    # one kind of direction at a time (the others NULL = 0)
    for kw in ("tx0", "tu", "tf"):
        dxs, _ = jvp(eng, x0, u, f, sub, **{kw: dev(r[kw][..., :2, :])})
        ok, ratio = P.within_bar(host(dxs), P.jvp(r["J"], **{kw: r[kw][..., :2, :]}))
        assert ok, (kw, ratio)


# ---- 3. duality
@pytest.mark.parametrize("case", [(64, 3, 4, False), (257, 3, 16, True)])
def test_forward_and_reverse_mode_are_dual_on_the_device(case):
    """<JVP(t), g> = <t, VJP(g)> per vehicle and direction, to 1e-12 of max(1, either side): each side is a sum of at most a few hundred
    products of O(1..30) terms in fp64, whose rounding is a few 1e-16 of the terms' size -- so the scale is floored at 1 rather than left
    to a sum that happens to cancel."""
    B, ticks, sub, force = case
    eng, r = engine(B), reference(case)
    x0, u, f = dev(r["x0"]), dev(r["u"]), dev(r["f"])
    xs = forward(eng, x0, u, f, sub)
    gx0, gu, gf = (host(t) for t in vjp(eng, x0, u, f, xs, dev(r["g"]), sub))
    dxs = host(jvp(eng, x0, u, f, sub, dev(r["tx0"]), dev(r["tu"]), dev(r["tf"]))[0])
    lhs = np.einsum("kbtc,kbc->bt", dxs, r["g"])
    rhs = np.einsum("btc,bc->bt", r["tx0"], gx0) + np.einsum("kbtc,kbc->bt", r["tu"], gu) + np.einsum("kbtc,kbc->bt", r["tf"], gf)
    rel = np.abs(lhs - rhs) / np.maximum(1.0, np.maximum(np.abs(lhs), np.abs(rhs)))
    print(case, "duality, worst relative:", rel.max())
    assert rel.max() <= 1e-12


# ---- 4. bit-level properties
def test_bit_level_promises():
    case = (257, 3, 4, True)
    B, ticks, sub, _ = case
    eng = engine(B)
    x0n, un, fn = P.inputs(B, ticks, seed=21)
    rng = np.random.default_rng(22)
    x0, u, f = dev(x0n), dev(un), dev(fn)
    tx0, tu, tf = dev(rng.normal(size=(B, 8, 10))), dev(rng.normal(size=(ticks, B, 8, 4))), dev(rng.normal(size=(ticks, B, 8, 3)))
    g = dev(rng.normal(size=(ticks, B, 10)))
    xs = forward(eng, x0, u, f, sub)
    # T = 8 directions in one call = 8 calls; the recomputed primal = the forward's log
    d8, xc = jvp(eng, x0, u, f, sub, tx0, tu, tf, check=True)
    assert np.array_equal(host(xc), host(xs))
    for t in range(8):
        d1, _ = jvp(eng, x0, u, f, sub, tx0[:, t:t + 1].contiguous(), tu[:, :, t:t + 1].contiguous(), tf[:, :, t:t + 1].contiguous())
        assert np.array_equal(host(d1[:, :, 0]), host(d8[:, :, t])), t
    # two reverse calls are identical; an output does not depend on which others are asked for
    a, b = vjp(eng, x0, u, f, xs, g, sub), vjp(eng, x0, u, f, xs, g, sub)
    for s, t in zip(a, b):
        assert np.array_equal(host(s), host(t)) and not (host(s) == -7.0).all()
    only = vjp(eng, x0, u, f, xs, g, sub, want=(False, True, False))
    assert only[0] is None and only[2] is None and np.array_equal(host(only[1]), host(a[1]))
    # d_f NULL with d_gf asked for = an all-zero d_f
    xs0 = forward(eng, x0, u, None, sub)
    zero = dev(np.zeros((ticks, B, 3)))
    assert np.array_equal(host(forward(eng, x0, u, zero, sub)), host(xs0))
    for s, t in zip(vjp(eng, x0, u, None, xs0, g, sub), vjp(eng, x0, u, zero, xs0, g, sub)):
        assert np.array_equal(host(s), host(t))


# ---- 5. structure
def test_structure_of_the_adjoint():
    case = (64, 3, 4, True)
    B, ticks, sub, _ = case
    eng = engine(B)
    x0n, un, fn = P.inputs(B, ticks, seed=31)
    x0, u, f = dev(x0n), dev(un), dev(fn)
    xs = forward(eng, x0, u, f, sub)
    rng = np.random.default_rng(32)
    last = np.zeros((ticks, B, 10))
    last[-1] = rng.normal(size=(B, 10))
    gx0, gu, gf = (host(t) for t in vjp(eng, x0, u, f, xs, dev(last), sub))
    assert (np.abs(gu).max(axis=-1) > 0).all() and (np.abs(gf).max(axis=-1) > 0).all()      # a terminal loss reaches every tick's input
    first = np.zeros((ticks, B, 10))
    first[0] = rng.normal(size=(B, 10))
    gx0, gu, gf = (host(t) for t in vjp(eng, x0, u, f, xs, dev(first), sub))
    assert not gu[1:].any() and not gf[1:].any() and gu[0].any() and gf[0].any()           # ... and the first state hears only tick 0
    # q / |q| has no component along q: an upstream gradient parallel to the output quaternion moves nothing
    along = np.zeros((ticks, B, 10))
    along[..., 6:] = host(xs)[..., 6:] * rng.uniform(0.5, 2.0, (ticks, B, 1))
    for t in vjp(eng, x0, u, f, xs, dev(along), sub):
        assert np.abs(host(t)).max() < 1e-13


# ---- 6. refusals
def test_refusals_enqueue_nothing_and_leave_the_handle_usable():
    B, ticks, sub = 64, 3, 4
    eng = engine(B)
    lib, h = eng._lib, eng._h
    x0n, un, fn = P.inputs(B, ticks, seed=41)
    x0, u, f = dev(x0n), dev(un), dev(fn)
    xs = forward(eng, x0, u, f, sub)
    g, tu = dev(np.ones((ticks, B, 10))), dev(np.ones((ticks, B, 1, 4)))
    o_xs, o_gx0, o_gu, o_gf, o_dxs, o_xc = (filled(ticks, B, 10), filled(B, 10), filled(ticks, B, 4), filled(ticks, B, 3),
                                            filled(ticks, B, 1, 10), filled(ticks, B, 10))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    import torch
    torch.cuda.synchronize()

    def fwd(hh=h, k=ticks, s=sub, a=x0, b=u, o=o_xs):
        return lib.ndp_plant_rollout_device(hh, k, DT, s, p(a), p(b), p(f), p(o), None)

    def rev(hh=h, k=ticks, s=sub, a=x0, b=u, log=xs, gg=g, outs=(o_gx0, o_gu, o_gf)):
        return lib.ndp_plant_rollout_vjp_device(hh, k, DT, s, p(a), p(b), p(f), p(log), p(gg), p(outs[0]), p(outs[1]), p(outs[2]), None)

    def fwdmode(hh=h, k=ticks, s=sub, a=x0, b=u, T=1, tans=(None, tu, None), o=o_dxs):
        return lib.ndp_plant_rollout_jvp_device(hh, k, DT, s, p(a), p(b), p(f), T, p(tans[0]), p(tans[1]), p(tans[2]), p(o), p(o_xc), None)

    for call in (fwd, rev, fwdmode):
        assert call(hh=None) == -1
        assert call(a=None) == -1 and call(b=None) == -1
        for bad in (dict(k=0), dict(k=-3), dict(s=0), dict(s=17)):
            assert call(**bad) == -2, (call.__name__, bad)
            assert b"must be" in lib.ndp_last_error(h)
    assert fwd(o=None) == -1
    assert rev(log=None) == -1 and rev(gg=None) == -1
    assert rev(outs=(None, None, None)) == -2 and b"no output" in lib.ndp_last_error(h)
    assert fwdmode(T=0) == -2 and fwdmode(T=9) == -2
    assert fwdmode(tans=(None, None, None)) == -2 and b"no tangent" in lib.ndp_last_error(h)
    assert fwdmode(o=None) == -2 and b"d_dxs" in lib.ndp_last_error(h)
    eng.synchronize()
    for t in (o_xs, o_gx0, o_gu, o_gf, o_dxs, o_xc):
        assert (host(t) == -7.0).all()
    assert fwd() == 0 and rev() == 0 and fwdmode() == 0              # the handle stays usable
    eng.synchronize()
    assert np.array_equal(host(o_xs), host(xs)) and np.array_equal(host(o_xc), host(xs))
    for t in (o_gx0, o_gu, o_gf, o_dxs):
        assert np.isfinite(host(t)).all() and not (host(t) == -7.0).any()


# ---- 7. the torch layer
def test_torch_layer_values_gradients_and_chaining():
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    case = (64, 3, 4, False)
    B, ticks, sub, _ = case
    eng, r = engine(B), reference((64, 3, 4, False))
    fn = np.random.default_rng(51).normal(0, 4, (ticks, B, 3))
    J = P.jacobian(r["x0"], r["u"], fn, DT, sub, eng.cfg.mass, eng.cfg.gravity)
    x0, u, f = (dev(a).requires_grad_(True) for a in (r["x0"], r["u"], fn))
    xs = TL.plant_rollout(eng, x0, u, f, dt=DT, substeps=sub)
    assert xs.shape == (ticks, B, 10) and xs.dtype == torch.float64
    assert np.array_equal(host(xs.detach()), host(forward(eng, x0.detach(), u.detach(), f.detach(), sub)))
    (xs * dev(r["g"])).sum().backward()
    for name, t, rf in zip(("x0", "u", "f"), (x0, u, f), P.vjp(J, r["g"])):
        ok, ratio = P.within_bar(host(t.grad), rf)
        assert ok, (name, ratio)
    # plant_step chained twice = plant_rollout with ticks = 2: values bit for bit, gradients to the bar
    a = [dev(v).requires_grad_(True) for v in (r["x0"], r["u"][:2], fn[:2])]
    b = [dev(v).requires_grad_(True) for v in (r["x0"], r["u"][:2], fn[:2])]
    two = TL.plant_rollout(eng, *a, dt=DT, substeps=sub)
    x1 = TL.plant_step(eng, b[0], b[1][0], b[2][0], dt=DT, substeps=sub)
    x2 = TL.plant_step(eng, x1, b[1][1], b[2][1], dt=DT, substeps=sub)
    assert x1.shape == (B, 10)
    assert np.array_equal(host(two.detach()), host(torch.stack([x1, x2]).detach()))
    w = dev(r["g"][:2])
    (two * w).sum().backward()
    (torch.stack([x1, x2]) * w).sum().backward()
    for s, t in zip(a, b):
        ok, ratio = P.within_bar(host(t.grad), host(s.grad))
        assert ok, ratio
    # forward mode through the layer: T axis kept when given, dropped when not
    xs_j, dxs = TL.plant_rollout_jvp(eng, x0, u, (dev(r["tx0"][:, :2]), None, dev(np.ascontiguousarray(r["tf"][:, :, :2]))), f=f, dt=DT,
                                     substeps=sub)
    assert np.array_equal(host(xs_j), host(xs.detach())) and dxs.shape == (ticks, B, 2, 10)
    ok, ratio = P.within_bar(host(dxs), P.jvp(J, tx0=r["tx0"][:, :2], tf=r["tf"][:, :, :2]))
    assert ok, ratio
    _, d1 = TL.plant_rollout_jvp(eng, x0, u, (None, dev(np.ascontiguousarray(r["tu"][:, :, 0])), None), f=f, dt=DT, substeps=sub)
    assert d1.shape == (ticks, B, 10)


def test_torch_gradcheck():
    import torch
    from ndp_nmpc_qd_amd import torch_layer as TL
    eng = engine(2)
    x0n, un, fn = P.inputs(2, 2, seed=61)
    args = [dev(a).requires_grad_(True) for a in (x0n, un, fn)]
    assert torch.autograd.gradcheck(lambda a, b, c: TL.plant_rollout(eng, a, b, c, dt=DT, substeps=2), args)
    assert torch.autograd.gradcheck(lambda a, b: TL.plant_rollout(eng, a, b, None, dt=DT, substeps=2), args[:2])


# ---- 8. one use: a held force identified from a logged flight by one Gauss-Newton step
def test_one_gauss_newton_step_recovers_a_held_force():
    """The state is exactly affine in a force held over the whole flight, so the three forward-mode columns for the unit force directions
    (d_tf = e_i at every tick, T = 3, taken at f = 0) and the residual to the f = 0 rollout give f* by one 3 x 3 solve per vehicle.  Bar
    1e-11 absolute: the same computation in float64 numpy recovered f* to 1.3e-14 over 50 draws."""
    B, ticks, sub = 4, 10, 4
    eng = engine(B)
    x0n, un, _ = P.inputs(B, ticks, seed=71, force=False)
    fstar = np.random.default_rng(72).normal(0, 4, (B, 3))
    x0, u = dev(x0n), dev(un)
    logged = host(forward(eng, x0, u, dev(np.broadcast_to(fstar, (ticks, B, 3))), sub))
    zero = dev(np.zeros((ticks, B, 3)))
    base = host(forward(eng, x0, u, zero, sub))
    tf = dev(np.broadcast_to(np.eye(3), (ticks, B, 3, 3)))
    dxs = host(jvp(eng, x0, u, zero, sub, tf=tf)[0])                           # [ticks, B, 3, 10]
    for v in range(B):
        A = dxs[:, v].transpose(0, 2, 1).reshape(ticks * 10, 3)
        res = (logged[:, v] - base[:, v]).reshape(ticks * 10)
        est = np.linalg.solve(A.T @ A, A.T @ res)
        print("vehicle", v, "|f_est - f*| max:", np.abs(est - fstar[v]).max())
        assert np.abs(est - fstar[v]).max() < 1e-11
