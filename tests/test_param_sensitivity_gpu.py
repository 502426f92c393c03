"""Parameter sensitivities on the device (run with -m gpu): rti_psens_kernel's du0/dxr, du0/dur, du0/df against the fixed-set reference
(tests/fixed_set_ref.py), against device finite differences, the torch layer's gradients, the translation identity, and the step's other
outputs against a handle with them off.  CPU side: tests/test_param_sensitivity.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.deriv_gpu import MIXED, ndp  # noqa: F401
from tests.fixed_set_ref import psens_ref, scale

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _step(ndp, b, level, params, fused=False, f=None, **kw):
    """One step of a fresh engine from xr / ur; returns (u0, X, U, st, it, act, sens, psens, Xp, Up, f)."""
    B, N = b["x0"].shape[0], b["xr"].shape[1] - 1
    eng = ndp.BatchedNMPC(B, N=N, disturbance=fused or f is not None, **kw)
    eng.reset(b["xr"], b["ur"])
    Xp, Up = eng.get_iterate()
    if level:
        eng.enable_sensitivity(level)
    if params:
        eng.enable_param_sensitivity()
    extra = dict(other=b["other"], ego_xy=b["ego_xy"]) if fused else dict(f=f) if f is not None else {}
    u0, X, U, st, it = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False, full=True, **extra)
    _, act = eng.active_set()
    sens = eng.sensitivity() if level else None
    ps = eng.param_sensitivity() if params else None
    fo = eng.device_force().cpu().numpy().copy() if fused else f
    eng.close()
    return u0, X, U, st, it, act, sens, ps, Xp, Up, fo


def _worst(oracle, b, out, idx):
    u0, X, U, st, it, act, sens, (dxr, dur, df), Xp, Up, f = out
    N = b["xr"].shape[1] - 1
    cfg = oracle.default_cfg(N=N, use_fd=f is not None)
    worst = 0.0
    for i in idx:
        ref = psens_ref(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], None if f is None else np.asarray(f[i], dtype=np.float64),
                        Xp[i], Up[i], act[i])
        s = max(scale(r) for r in ref)
        worst = max(worst, *(np.max(np.abs(g[i] - r)) / s for g, r in zip((dxr, dur, df), ref)))
    return worst


@pytest.mark.parametrize("form", [dict(fused=True), dict(work_queue=1), dict(fused=True, N=13)])
def test_mixed_batch_matches_the_fixed_set_reference(ndp, oracle, form):
    """B = 1024 mixed (about a fifth of the instances on input bounds): in place fused, the work list's producer / consumer (unfused,
    N = 20), and the run-time horizon N = 13 (fused).  48 seeded status-0 active-set instances, pinned ones among them, within 1e-9 of
    max(1, |J|max) of psens_ref; stage 0's reference rows, f_N and pinned stage-0 rows exactly 0 everywhere."""
    form = dict(form)
    N = form.pop("N", 20)
    b = synth.make_batch(1024, N=N, seed=synth.SEED0 + 50, downwash=form.get("fused", False), **MIXED)
    out = _step(ndp, b, 1, True, **form)
    st, it, act, (dxr, dur, df) = out[3], out[4], out[5], out[7]
    idx = np.flatnonzero((st == 0) & (it == 0))
    assert idx.size >= 900 and act.any()
    rng = np.random.default_rng(3)
    pin = [i for i in idx if act[i].any()]
    pick = sorted(set(rng.choice(idx, 40, replace=False).tolist()) | set(pin[:8]))
    assert _worst(oracle, b, out, pick) <= BAR
    ok = st == 0
    assert not dxr[ok][:, :, 0].any() and not df[ok][:, :, N].any()
    p0 = act[ok][:, 0] != 0
    assert not dxr[ok][p0].any() and not dur[ok][p0].any() and not df[ok][p0].any()


@pytest.fixture(scope="module")
def fd_case(ndp):
    """B = 256, N = 20, a supplied fp32 force: the step through the torch layer with x0, xr, ur and f requiring grad, and device central
    differences of u0 in a few entries of xr, ur and f from the same iterate and kept set (restored in that order)."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import ControlStep
    B, N = 256, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 52, **MIXED)
    f = np.random.default_rng(5).normal(0.0, 0.4, (B, N + 1, 3)).astype(np.float32)
    eng = ndp.BatchedNMPC(B, disturbance=True)
    eng.reset(b["xr"], b["ur"])
    eng.update(b["x0"], b["xr"], b["ur"], f=f, raise_on_status=False)      # a kept set to start from
    X0, U0 = eng.get_iterate()
    _, A0 = eng.active_set()
    layer = ControlStep(eng, params=True)
    dev = torch.device("cuda", 0)
    x0 = torch.tensor(b["x0"], device=dev, requires_grad=True)
    xr = torch.tensor(b["xr"], device=dev, requires_grad=True)
    ur = torch.tensor(b["ur"], device=dev, requires_grad=True)
    ft = torch.tensor(f, device=dev, requires_grad=True)
    u0 = layer(x0, xr, ur, f=ft)
    g = torch.randn(B, 4, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    gxr, gur, gf = (t.cpu().numpy() for t in torch.autograd.grad(u0, (xr, ur, ft), g))
    st0, it0 = eng.status()
    J = eng.param_sensitivity()
    _, Ab = eng.active_set()
    stable = (st0 == 0) & (it0 == 0)
    fds = []
    cases = [("xr", (k, j), 1e-6) for k, j in ((1, 0), (6, 4), (10, 7), (20, 9))] + \
            [("ur", (k, j), 1e-6) for k, j in ((0, 3), (8, 1))] + [("f", (k, j), 2.0 ** -10) for k, j in ((0, 2), (12, 0))]
    for which, (k, j), h in cases:
        us = []
        for sgn in (1.0, -1.0):
            eng.set_iterate(X0, U0)
            eng.set_active_set(A0)
            a = dict(xr=b["xr"].copy(), ur=b["ur"].copy(), f=f.copy())
            a[which][:, k, j] += sgn * h
            u, _, _, st, it = eng.update(b["x0"], a["xr"], a["ur"], f=a["f"], raise_on_status=False, full=True)
            _, A = eng.active_set()
            stable &= (st == 0) & (it == 0) & (A == Ab).all(axis=(1, 2))
            us.append(u)
        fds.append((which, k, j, (us[0] - us[1]) / (2 * h)))
    eng.close()
    return dict(J=dict(zip(("xr", "ur", "f"), J)), fds=fds, stable=stable, grads=dict(xr=gxr, ur=gur, f=gf), g=g.cpu().numpy())


def test_device_finite_differences_match_the_parameter_sensitivities(fd_case):
    c = fd_case
    s = c["stable"]
    assert s.sum() >= 200
    for which, k, j, fd in c["fds"]:
        J = c["J"][which][s]
        err = np.max(np.abs(fd[s] - J[:, :, k, j]), axis=1) / np.maximum(1.0, np.max(np.abs(J), axis=(1, 2, 3)))
        assert err.max() <= 1e-6, (which, k, j, err.max())


def test_torch_layer_gradients_match_device_finite_differences(fd_case):
    c = fd_case
    s = c["stable"]
    for which, k, j, fd in c["fds"]:
        ref = np.einsum("bi,bi->b", fd[s], c["g"][s])
        got = c["grads"][which][s][:, k, j]
        assert np.max(np.abs(got - ref)) <= 1e-6 * max(1.0, np.max(np.abs(ref))), (which, k, j)
    for which in ("xr", "ur", "f"):
        ref = np.einsum("bi,bi...->b...", c["g"], c["J"][which])
        tol = 1e-5 if which == "f" else 1e-13
        assert c["grads"][which].dtype == (np.float32 if which == "f" else np.float64)
        assert np.allclose(c["grads"][which], ref, rtol=tol, atol=tol, equal_nan=True)


def test_translation_identity_under_interior_point_always(ndp):
    """qp_mode 1 (the last Newton system; the fixed-set reference does not apply): du0/dx0[:, 0:3] + sum_k du0/dxr[:, k, 0:3] = 0 to 1e-9."""
    b = synth.make_batch(512, seed=synth.SEED0 + 53, downwash=True, **MIXED)
    out = _step(ndp, b, 1, True, fused=True, qp_mode=1)
    st, (du0, _, _), (dxr, _, _) = out[3], out[6], out[7]
    ok = st == 0
    assert ok.sum() >= 500 and out[4][ok].min() > 0
    res = np.abs(du0[ok][:, :, 0:3] + dxr[ok][:, :, :, 0:3].sum(axis=2)).max(axis=(1, 2))
    assert (res / np.maximum(1.0, np.abs(du0[ok]).max(axis=(1, 2)))).max() <= BAR


@pytest.mark.parametrize("form", [dict(fused=True), dict(work_queue=1), dict(fused=True, N=13)])
def test_parameter_sensitivities_do_not_change_the_step(ndp, form):
    """u0, iterate, status, iteration words, kept sets and the level-1 / level-2 outputs are bit-identical with them on and off."""
    form = dict(form)
    N = form.pop("N", 20)
    b = synth.make_batch(1024, N=N, seed=synth.SEED0 + 54, downwash=form.get("fused", False), **MIXED)
    for level in (1, 2):
        a = _step(ndp, b, level, False, **form)
        s = _step(ndp, b, level, True, **form)
        for x, y in zip(a[:6], s[:6]):
            assert np.array_equal(x, y)
        for x, y in zip(a[6], s[6]):
            assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True)


def test_nan_state_gives_nan_only_for_its_instance(ndp):
    b = synth.make_batch(256, seed=synth.SEED0 + 55, **MIXED)
    clean = _step(ndp, b, 1, True)
    b["x0"][5, 3] = np.nan
    bad = _step(ndp, b, 1, True)
    assert bad[3][5] != 0
    keep = np.arange(256) != 5
    for a, c in zip(bad[7], clean[7]):
        assert np.isnan(a[5]).all() and np.array_equal(a[keep], c[keep])


def test_refusals_name_their_reason_and_launch_nothing(ndp):
    B = 64
    b = synth.make_batch(B, N=13, seed=synth.SEED0 + 56, **MIXED)
    eng = ndp.BatchedNMPC(B, N=13)
    eng.reset(b["xr"], b["ur"])
    with pytest.raises(ndp.NdpError, match=r"\(-2\).*ndp_sens_enable"):
        eng.enable_param_sensitivity()
    assert not eng.param_sensitivity_enabled
    eng.enable_sensitivity(1)
    eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)      # level 1 alone: the unfused run-time horizon is served
    eng.enable_param_sensitivity()
    X, U = eng.get_iterate()
    K = eng.sensitivity()[0]
    with pytest.raises(ndp.NdpError, match=r"\(-2\).*need the fused step"):
        eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)
    X2, U2 = eng.get_iterate()
    assert np.array_equal(X, X2) and np.array_equal(U, U2) and np.array_equal(eng.sensitivity()[0], K)
    assert np.isnan(eng.param_sensitivity()[0]).all()                  # nothing was written
    with pytest.raises(ndp.NdpError, match=r"\(-2\).*sensitivities are enabled"):
        eng.tick_config(None)
    eng.enable_sensitivity(0)                                           # frees them too
    assert not eng.param_sensitivity_enabled and eng._lib.ndp_device_sens_xr(eng._h) is None
    with pytest.raises(ndp.NdpError, match=r"\(-2\).*not enabled"):
        eng._check(eng._lib.ndp_get_sens_params(eng._h, None, None, None), "ndp_get_sens_params")
    eng.close()


def test_training_a_force_offset_through_the_layer(ndp):
    """Twenty gradient steps (Adam, decaying step) on a per-instance constant force offset, through ControlStep(params=True), bring u0 towards the u0 of
    the force 0.5 everywhere: |u0 - u_target|^2 falls below a tenth.  The iterate is restored before every step (set_iterate also empties
    the kept sets), so each forward pass solves the same QP but for the force."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import ControlStep
    B, N = 64, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 57)
    eng = ndp.BatchedNMPC(B, disturbance=True)
    eng.reset(b["xr"], b["ur"])
    X0, U0 = eng.get_iterate()
    layer = ControlStep(eng, params=True)
    dev = torch.device("cuda", 0)
    x0, xr, ur = (torch.tensor(b[k], device=dev) for k in ("x0", "xr", "ur"))
    off = torch.zeros(B, 1, 3, dtype=torch.float32, device=dev, requires_grad=True)
    with torch.no_grad():
        eng.set_iterate(X0, U0)
        u_target = layer(x0, xr, ur, f=torch.full((B, N + 1, 3), 0.5, dtype=torch.float32, device=dev))
    opt = torch.optim.Adam([off], lr=0.1)         # (per-element steps: the instances' offsets are independent)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.85)
    losses = []
    for _ in range(20):
        eng.set_iterate(X0, U0)
        u0 = layer(x0, xr, ur, f=off.expand(B, N + 1, 3).contiguous())
        loss = ((u0 - u_target) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(loss.item())
    eng.close()
    print("force-offset training losses:", ["%.3e" % v for v in losses])
    assert losses[-1] < 0.1 * losses[0] and np.isfinite(losses).all()
