"""Initial-state sensitivities on the device (run with -m gpu): rti_sens_kernel against the fixed-set reference (tests/fixed_set_ref.py: the
oracle's QP at the pre-step iterate, dense KKT), against device finite differences, and the step's other outputs against a handle with
sensitivities off.  CPU side: tests/test_sensitivity.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.deriv_gpu import MIXED, ndp  # noqa: F401
from tests.fixed_set_ref import scale, sens_ref

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _step(ndp, b, level, fused=False, **kw):
    """One step of a fresh engine from xr / ur; returns (u0, X, U, st, it, act, sens, Xp, Up, f)."""
    B, N = b["x0"].shape[0], b["xr"].shape[1] - 1
    eng = ndp.BatchedNMPC(B, N=N, disturbance=fused, **kw)
    eng.reset(b["xr"], b["ur"])
    Xp, Up = eng.get_iterate()
    if level:
        eng.enable_sensitivity(level)
    extra = dict(other=b["other"], ego_xy=b["ego_xy"]) if fused else {}
    u0, X, U, st, it = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False, full=True, **extra)
    _, act = eng.active_set()
    sens = eng.sensitivity() if level else None
    f = eng.device_force().cpu().numpy().copy() if fused else None
    eng.close()
    return u0, X, U, st, it, act, sens, Xp, Up, f


def _ref(oracle, b, i, Xp, Up, act, f=None):
    N = b["xr"].shape[1] - 1
    cfg = oracle.default_cfg(N=N, use_fd=f is not None)
    qp = oracle.linearize(cfg, b["x0"][i], b["xr"][i], b["ur"][i], None if f is None else f[i], Xp[i], Up[i])
    return sens_ref(qp, act[i])


def _check_against_ref(oracle, b, out, idx, level2_idx):
    u0, X, U, st, it, act, (du0, dU, dX), Xp, Up, f = out
    worst = 0.0
    for i in idx:
        r0, rU, rX = _ref(oracle, b, i, Xp, Up, act, f)
        s = scale(rU)
        worst = max(worst, np.max(np.abs(du0[i] - r0)) / s)
        if i in level2_idx:
            worst = max(worst, np.max(np.abs(dU[i] - rU)) / s, np.max(np.abs(dX[i] - rX)) / max(1.0, np.max(np.abs(rX))))
    return worst


def test_mixed_fused_batch_matches_the_fixed_set_reference(ndp, oracle):
    """B = 1024, N = 20, fused downwash, default mode, level 2: du0 of every status-0 instance the active set finished within 1e-9 of
    max(1, |K|max); dU and dX on 64 seeded instances; rows of pinned inputs exactly 0, dX_0 = I."""
    b = synth.make_batch(1024, seed=synth.SEED0 + 40, downwash=True, **MIXED)
    out = _step(ndp, b, 2, fused=True)
    u0, X, U, st, it, act, (du0, dU, dX), *_ = out
    idx = np.flatnonzero((st == 0) & (it == 0))
    assert idx.size >= 1000 and act.any()
    l2 = set(np.random.default_rng(7).choice(idx, 64, replace=False).tolist())
    assert _check_against_ref(oracle, b, out, idx, l2) <= BAR
    ok = st == 0
    assert not dU[ok][act[ok] != 0].any() and not du0[ok][act[ok][:, 0] != 0].any()
    assert np.array_equal(dX[ok][:, 0], np.broadcast_to(np.eye(10), (int(ok.sum()), 10, 10)))


def test_work_list_and_in_place_forms_agree(ndp, oracle):
    """The same batch with the work list forced on (its consumer solves the listed instances) and off: sensitivities agree to 1e-12,
    and the work-list form meets the reference."""
    b = synth.make_batch(1024, seed=synth.SEED0 + 41, **MIXED)
    on = _step(ndp, b, 2, work_queue=1)
    off = _step(ndp, b, 2, work_queue=2)
    assert np.array_equal(on[3], off[3]) and not on[3].any()
    for a, c in zip(on[6], off[6]):
        assert np.max(np.abs(a - c)) <= 1e-12 * max(1.0, np.max(np.abs(c)))
    idx = np.flatnonzero(on[4] == 0)
    assert _check_against_ref(oracle, b, on, idx[:128], set(idx[:32].tolist())) <= BAR


@pytest.fixture(scope="module")
def fd_case(ndp):
    """B = 256, level 1: the step at x0 through the torch layer (u0, K0, grad_x0 of a random upstream gradient) and device central
    differences at x0 +- 1e-6 e_j from the same iterate and kept set (restored in that order: set_iterate empties the sets)."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import ControlStep
    B, h = 256, 1e-6
    b = synth.make_batch(B, seed=synth.SEED0 + 42, **MIXED)
    eng = ndp.BatchedNMPC(B)
    eng.reset(b["xr"], b["ur"])
    eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)       # a kept set to start from
    X0, U0 = eng.get_iterate()
    _, A0 = eng.active_set()
    layer = ControlStep(eng)
    dev = torch.device("cuda", 0)
    x0 = torch.tensor(b["x0"], device=dev, requires_grad=True)
    xr, ur = torch.tensor(b["xr"], device=dev), torch.tensor(b["ur"], device=dev)
    u0 = layer(x0, xr, ur)
    g = torch.randn(B, 4, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    (gx,) = torch.autograd.grad(u0, x0, g)
    st0, it0 = eng.status()
    K0 = eng.sensitivity()[0]
    _, Ab = eng.active_set()
    fd = np.zeros((B, 4, 10))
    stable = (st0 == 0) & (it0 == 0)
    for j in range(10):
        us = []
        for sgn in (1.0, -1.0):
            eng.set_iterate(X0, U0)
            eng.set_active_set(A0)
            x = b["x0"].copy()
            x[:, j] += sgn * h
            u, _, _, st, it = eng.update(x, b["xr"], b["ur"], raise_on_status=False, full=True)
            _, A = eng.active_set()
            stable &= (st == 0) & (it == 0) & (A == Ab).all(axis=(1, 2))
            us.append(u)
        fd[:, :, j] = (us[0] - us[1]) / (2 * h)
    eng.close()
    return dict(K0=K0, fd=fd, stable=stable, gx=gx.cpu().numpy(), g=g.cpu().numpy())


def test_device_finite_differences_match_du0_dx0(fd_case):
    c = fd_case
    s = c["stable"]
    assert s.sum() >= 200
    K, fd = c["K0"][s], c["fd"][s]
    err = np.max(np.abs(fd - K), axis=(1, 2)) / np.maximum(1.0, np.max(np.abs(K), axis=(1, 2)))
    assert err.max() <= 1e-6, err.max()


def test_torch_layer_gradient_matches_device_finite_differences(fd_case):
    c = fd_case
    s = c["stable"]
    ref = np.einsum("bij,bi->bj", c["fd"][s], c["g"][s])
    assert np.max(np.abs(c["gx"][s] - ref)) <= 1e-6 * max(1.0, np.max(np.abs(ref)))
    assert np.allclose(c["gx"], np.einsum("bij,bi->bj", c["K0"], c["g"]), rtol=1e-13, atol=1e-13, equal_nan=True)


@pytest.mark.parametrize("form", [dict(fused=True), dict(fused=True, work_queue=1), dict(N=13)])
def test_sensitivities_do_not_change_the_step(ndp, form):
    """A handle with sensitivities on (level 2) returns u0, iterate, status and iteration words bit-identical to one with them off."""
    form = dict(form)
    N = form.pop("N", 20)
    b = synth.make_batch(1024, N=N, seed=synth.SEED0 + 43, downwash=form.get("fused", False), **MIXED)
    a = _step(ndp, b, 0, **form)
    s = _step(ndp, b, 2, **form)
    for x, y in zip(a[:6], s[:6]):
        assert np.array_equal(x, y)


def test_interior_point_always(ndp, oracle):
    """qp_mode 1: the derivative of the last Newton system, which carries the barrier's weights mu / t^2 on every bound.  Instances with
    no input within 1e-2 of a bound stay within 5e-2 of the empty-set reference (at t = 1e-2 the weight of the last Newton system's
    mu is of the order of the input weights: measured 1.1e-2, not the 1e-6 a barrier-free system would give); rows of stage-0 inputs on
    a bound (within 1e-6) are below 5e-2 of the scale (the barrier's weight mostly holds them: measured 1.3e-2 at worst, where the free
    rows are O(1)).  Deviation from the fixed-set derivative measured on 128 instances: 1.1e-2 (inputs > 0.1 from their bounds), 5e-3
    (> 0.3), 8e-4 (> 1)."""
    b = synth.make_batch(512, seed=synth.SEED0 + 44, **MIXED)
    out = _step(ndp, b, 1, qp_mode=1)
    u0, X, U, st, it, act, (du0, _, _), Xp, Up, _ = out
    assert not st.any() and not act.any()
    cfg = oracle.default_cfg()
    lb, ub = np.array(cfg.lbu[:4]), np.array(cfg.ubu[:4])
    dist = np.minimum(np.abs(U - lb), np.abs(U - ub)).min(axis=(1, 2))
    empty = np.zeros((512, 20, 4), dtype=np.int8)
    free = np.flatnonzero(dist > 1e-2)
    assert free.size >= 50
    err = {}
    for i in free[:128]:
        r0 = _ref(oracle, b, i, Xp, Up, empty)[0]
        err[i] = np.max(np.abs(du0[i] - r0)) / scale(r0)
    for d in (1e-2, 1e-1, 3e-1, 1.0):
        e = [v for i, v in err.items() if dist[i] > d]
        print(f"interior point: {len(e)} instances with every input > {d} from its bounds: worst rel. deviation {max(e, default=0.0):.2e}")
    assert max(err.values()) <= 5e-2
    onb = np.argwhere(np.minimum(np.abs(U[:, 0] - lb), np.abs(U[:, 0] - ub)) < 1e-6)
    assert onb.shape[0] >= 1
    worst_on = 0.0
    for i, r in onb:
        worst_on = max(worst_on, np.max(np.abs(du0[i, r])) / scale(du0[i]))
    print(f"interior point: {onb.shape[0]} stage-0 inputs on a bound: worst row {worst_on:.2e} of the scale")
    assert worst_on <= 5e-2


@pytest.mark.parametrize("N", [13, 27])
def test_run_time_horizons_level_two(ndp, oracle, N):
    b = synth.make_batch(128, N=N, seed=synth.SEED0 + 45, **MIXED)
    out = _step(ndp, b, 2)
    st, it = out[3], out[4]
    idx = np.flatnonzero((st == 0) & (it == 0))
    assert idx.size >= 120
    assert _check_against_ref(oracle, b, out, idx, set(idx.tolist())) <= BAR


def test_nan_state_gives_nan_sensitivities_only_for_its_instance(ndp):
    b = synth.make_batch(256, seed=synth.SEED0 + 46, **MIXED)
    clean = _step(ndp, b, 2)
    b["x0"][5, 3] = np.nan
    bad = _step(ndp, b, 2)
    assert bad[3][5] != 0
    keep = np.arange(256) != 5
    for a, c in zip(bad[6], clean[6]):
        assert np.isnan(a[5]).all() and np.array_equal(a[keep], c[keep])


def test_refusals_name_their_reason_and_launch_nothing(ndp):
    B = 64
    for kw, why in ((dict(N=40), "N <= 27"), (dict(qp_precision=3), "qp_precision 0"), (dict(n_rti=2), "n_rti = 1")):
        eng = ndp.BatchedNMPC(B, **kw)
        with pytest.raises(ndp.NdpError, match=r"\(-2\).*" + why.replace("=", r"\=")):
            eng.enable_sensitivity(1)
        assert eng.sensitivity_level == 0
        eng.close()
    b = synth.make_batch(B, seed=synth.SEED0 + 47, **MIXED)
    eng = ndp.BatchedNMPC(B)
    eng.reset(b["xr"], b["ur"])
    eng.enable_sensitivity(1)
    eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)
    X, U = eng.get_iterate()
    K = eng.sensitivity()[0]
    with pytest.raises(ndp.NdpError, match=r"ndp_tick_config.*\(-2\).*sensitivities are enabled"):
        eng.tick_config(None)
    with pytest.raises(ndp.NdpError, match=r"\(-2\).*ndp_tick_reset"):
        eng.tick_reset()
    with pytest.raises(ndp.NdpError, match="level 2"):
        eng._check(eng._lib.ndp_get_sens(eng._h, None, None, K.ctypes.data), "ndp_get_sens")
    X2, U2 = eng.get_iterate()
    assert np.array_equal(X, X2) and np.array_equal(U, U2) and np.array_equal(eng.sensitivity()[0], K)
    eng.enable_sensitivity(0)
    assert eng.sensitivity_level == 0
    eng.tick_config(None)                                       # off again: the tick is served
    eng.close()
