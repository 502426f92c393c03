"""The adjoint of the control step on the device (run with -m gpu): rti_vjp_kernel for an upstream on u0 alone against today's Jacobians,
for full-trajectory upstreams against the dense fixed-set reference (tests/fixed_set_ref.py), against device finite differences, the recompute
against the recorded step, isolation (engine state and tape untouched, repeatable), tapes kept over later steps, refusals, and the torch
layer.  CPU side: tests/test_step_vjp.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.deriv_gpu import MIXED, _dev, _recorded_step, _t, _vjp, ndp  # noqa: F401
from tests.fixed_set_ref import scale, vjp_ref

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("form", [dict(fused=True), dict(), dict(work_queue=1), dict(work_queue=2), dict(qp_mode=1, fused=True)])
def test_gu0_only_matches_the_jacobians_and_the_recompute_is_the_step(ndp, form):
    """B = 1024, N = 20 mixed (free, pinned and interior-point instances): the VJP of a random gu0 against gu0 contracted with
    ndp_get_sens / ndp_get_sens_params, within 1e-10 of max(1, |g|max) for set finishes (interior point: 1e-6, the barrier-weighted
    system -- tests/test_step_vjp.py); the recompute's status and u0 equal the step's (u0 within 1e-12; bit-unequal instances reported)."""
    form = dict(form)
    fused = form.pop("fused", False)
    b = synth.make_batch(1024, seed=synth.SEED0 + 80, downwash=fused, **MIXED)
    r = _recorded_step(ndp, b, fused=fused, params=True, **form)
    g = np.random.default_rng(1).normal(size=(1024, 4))
    gx0, gxr, gur, gf, u0c, stc = _vjp(r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], f=r["force"], gu0=_t(g))
    r["eng"].close()
    st, it = r["st"], r["it"]
    assert np.array_equal(stc, st)
    ok = st == 0
    ipm = (it & 0xffff) > 0
    assert ok.sum() >= 900 and (r["act"][ok].any(axis=(1, 2)) | ipm[ok]).any()
    rel = np.abs(u0c - r["u0"]).max(axis=1) / np.maximum(1.0, np.abs(r["u0"]).max(axis=1))
    assert rel[ok].max() <= 1e-12
    print(f"{dict(form, fused=fused)}: {int((u0c != r['u0']).any(axis=1).sum())} of 1024 recomputed u0 bit-unequal, "
          f"{int(ipm.sum())} interior point")
    dxr, dur, df = r["J"]
    ref = (np.einsum("bij,bi->bj", r["K0"], g), np.einsum("bi,bikj->bkj", g, dxr), np.einsum("bi,bikj->bkj", g, dur),
           np.einsum("bi,bikj->bkj", g, df))
    s = np.maximum(1.0, np.max([np.abs(x).reshape(1024, -1).max(axis=1) for x in ref], axis=0))
    err = np.max([np.abs(x - y).reshape(1024, -1).max(axis=1) for x, y in zip((gx0, gxr, gur, gf), ref)], axis=0) / s
    if (ok & ~ipm).any():
        assert err[ok & ~ipm].max() <= 1e-10, err[ok & ~ipm].max()
    if (ok & ipm).any():
        assert err[ok & ipm].max() <= 1e-6, err[ok & ipm].max()
    for x in (gx0, gxr, gur, gf):
        assert np.isnan(x[~ok]).all()


@pytest.mark.parametrize("N", [2, 13, 20, 27])
def test_full_trajectory_upstream_matches_the_dense_reference(ndp, oracle, N):
    """B = 64 mixed with a supplied force, random (gu0, gX, gU): 12 seeded status-0 set finishes within 1e-9 of max(1, |g|max) of vjp_ref
    at the pre-step iterate and the step's final set; stage 0's xr row and f_N exactly 0."""
    B = 64
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 81, **MIXED)
    f = np.random.default_rng(2).normal(0.0, 0.3, (B, N + 1, 3)).astype(np.float32)
    r = _recorded_step(ndp, b, f=f, params=False)
    rng = np.random.default_rng(3)
    gu0, gX, gU = rng.normal(size=(B, 4)), rng.normal(size=(B, N + 1, 10)), rng.normal(size=(B, N, 4))
    out = _vjp(r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], f=r["force"], gu0=_t(gu0), gX=_t(gX), gU=_t(gU))
    Xl, Ul, _ = (v.cpu().numpy() for v in r["tape"])
    r["eng"].close()
    idx = np.flatnonzero((r["st"] == 0) & ((r["it"] & 0xffff) == 0))
    assert idx.size >= 40
    cfg = oracle.default_cfg(N=N, use_fd=True)
    for i in np.random.default_rng(4).choice(idx, 12, replace=False):
        ref = vjp_ref(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), Xl[i], Ul[i], r["act"][i], gu0[i], gX[i], gU[i])
        s = max(scale(x) for x in ref)
        for got, x in zip(out[:4], ref):
            assert np.max(np.abs(got[i] - x)) <= 1e-9 * s, (i, np.max(np.abs(got[i] - x)) / s)
    ok = r["st"] == 0
    assert not out[1][ok][:, 0].any() and not out[3][ok][:, N].any()


def test_device_finite_differences_of_a_trajectory_loss(ndp):
    """L = gu0.u0 + gX.X + gU.U of the step: central differences in a few entries of x0, xr, ur and f (each run from the same iterate and
    kept set) against the VJP, on the instances whose set and iteration word do not change, within 1e-6."""
    B, N = 256, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 82, **MIXED)
    f = np.random.default_rng(5).normal(0.0, 0.4, (B, N + 1, 3)).astype(np.float32)
    r = _recorded_step(ndp, b, f=f, params=False)
    eng = r["eng"]
    rng = np.random.default_rng(6)
    gu0, gX, gU = rng.normal(size=(B, 4)), rng.normal(size=(B, N + 1, 10)), rng.normal(size=(B, N, 4))
    g = _vjp(eng, r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], f=r["force"], gu0=_t(gu0), gX=_t(gX), gU=_t(gU))
    X0, U0, A0 = (v.cpu().numpy() for v in r["tape"])
    stable = (r["st"] == 0) & ((r["it"] & 0xffff) == 0)
    cases = [("x0", (3,), 1e-6), ("x0", (7,), 1e-6), ("xr", (6, 4), 1e-6), ("xr", (10, 7), 1e-6), ("ur", (0, 3), 1e-6), ("ur", (8, 1), 1e-6),
             ("f", (0, 2), 2.0 ** -14), ("f", (12, 0), 2.0 ** -14)]
    which_out = dict(x0=0, xr=1, ur=2, f=3)
    fds = []
    for which, at, h in cases:
        L = []
        for sgn in (1.0, -1.0):
            eng.set_iterate(X0, U0)
            eng.set_active_set(A0)
            a = dict(x0=b["x0"].copy(), xr=b["xr"].copy(), ur=b["ur"].copy(), f=f.copy())
            a[which][(slice(None),) + at] += sgn * h
            u, X, U, st, it = eng.update(a["x0"], a["xr"], a["ur"], f=a["f"], raise_on_status=False, full=True)
            _, A = eng.active_set()
            stable &= (st == 0) & ((it & 0xffff) == 0) & (A == r["act"]).all(axis=(1, 2))
            L.append((u * gu0).sum(axis=1) + (X * gX).sum(axis=(1, 2)) + (U * gU).sum(axis=(1, 2)))
        fds.append((which, at, (L[0] - L[1]) / (2 * h)))
    eng.close()
    assert stable.sum() >= 150
    for which, at, fd in fds:
        got = g[which_out[which]][(slice(None),) + at]
        err = np.abs(fd - got)[stable] / np.maximum(1.0, np.abs(got[stable]))
        assert err.max() <= 1e-6, (which, at, err.max())


def test_state_and_tape_untouched_and_repeatable(ndp):
    """A VJP call leaves the engine's iterate, kept sets and sensitivity buffers bit-unchanged, and the tape too; two calls on one tape
    give bit-identical gradients; a NaN state gives NaN only for its own instance."""
    B = 256
    b = synth.make_batch(B, seed=synth.SEED0 + 83, downwash=True, **MIXED)
    b["x0"][5, 3] = np.nan
    r = _recorded_step(ndp, b, fused=True, params=True)
    eng = r["eng"]
    before = [v.cpu().numpy().copy() for v in eng.device_iterate()] + [eng.active_set()[1], *eng.sensitivity()[:1], *eng.param_sensitivity()]
    tape0 = [v.cpu().numpy().copy() for v in r["tape"]]
    gu0 = _t(np.random.default_rng(7).normal(size=(B, 4)))
    gX = _t(np.random.default_rng(8).normal(size=(B, 21, 10)))
    a = _vjp(eng, r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], f=r["force"], gu0=gu0, gX=gX)
    c = _vjp(eng, r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], f=r["force"], gu0=gu0, gX=gX)
    after = [v.cpu().numpy() for v in eng.device_iterate()] + [eng.active_set()[1], *eng.sensitivity()[:1], *eng.param_sensitivity()]
    eng.close()
    for x, y in zip(before, after):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(tape0, r["tape"]):
        assert np.array_equal(x, y.cpu().numpy())
    for x, y in zip(a, c):
        assert np.array_equal(x, y, equal_nan=True)
    assert r["st"][5] != 0 and a[5][5] != 0
    keep = np.arange(B) != 5
    for x in a[:4]:
        assert np.isnan(x[5]).all() and np.isfinite(x[keep][r["st"][keep] == 0]).all()


def test_a_tape_kept_over_later_steps_still_gives_its_step(ndp):
    """The gradient of a step recorded ten steps ago (the engine has moved on) equals the one taken right after that step, bit for bit."""
    import torch
    B = 256
    b = synth.make_batch(B, seed=synth.SEED0 + 84, **MIXED)
    r = _recorded_step(ndp, b, params=False)
    eng = r["eng"]
    gu0, gU = _t(np.random.default_rng(9).normal(size=(B, 4))), _t(np.random.default_rng(10).normal(size=(B, 20, 4)))
    now = _vjp(eng, r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], gu0=gu0, gU=gU)
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    x0 = _t(b["x0"] + 0.05)
    for _ in range(10):
        eng.update_device(x0, r["t"]["xr"], r["t"]["ur"], u0)
    later = _vjp(eng, r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], gu0=gu0, gU=gU)
    eng.close()
    for x, y in zip(now, later):
        assert np.array_equal(x, y, equal_nan=True)


def test_refusals_name_their_reason_and_launch_nothing(ndp):
    import torch
    for kw, N, what in ((dict(n_rti=2), 20, "n_rti = 1"), (dict(qp_precision=1), 20, "qp_precision 0"), ({}, 40, "N <= 27")):
        B = 64
        b = synth.make_batch(B, N=N, seed=synth.SEED0 + 85, **MIXED)
        eng = ndp.BatchedNMPC(B, N=N, **kw)
        eng.reset(b["xr"], b["ur"])
        tape = eng.record_tape()
        t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
        gx0 = torch.full((B, 10), -7.0, dtype=torch.float64, device=_dev())
        with pytest.raises(ndp.NdpError, match=r"\(-2\).*" + what):
            eng.step_vjp_device(t["x0"], t["xr"], t["ur"], tape, gu0=torch.ones(B, 4, dtype=torch.float64, device=_dev()), gx0=gx0)
        torch.cuda.synchronize()
        assert (gx0 == -7.0).all()
        eng.close()
    b = synth.make_batch(64, seed=synth.SEED0 + 85, **MIXED)
    eng = ndp.BatchedNMPC(64)
    eng.reset(b["xr"], b["ur"])
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
    with pytest.raises(ndp.NdpError, match=r"\(-2\).*no upstream gradient"):
        eng.step_vjp_device(t["x0"], t["xr"], t["ur"], eng.record_tape())
    eng.close()


def test_torch_trajectory_layer_matches_control_step_on_u0(ndp):
    """A loss on u0 alone: control_step_trajectory's x0 / xr / ur / f gradients equal control_step's with parameter sensitivities (two engines
    on the same inputs), within 1e-10 of max(1, |g|max) on the set finishes."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import ControlStep, control_step_trajectory
    B, N = 256, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 86, **MIXED)
    f = np.random.default_rng(11).normal(0.0, 0.4, (B, N + 1, 3)).astype(np.float32)
    g = _t(np.random.default_rng(12).normal(size=(B, 4)))
    grads, its = [], []
    side = torch.cuda.Stream(device=_dev())      # (a stream the C-ABI can name: both layers order their copies on it)
    side.wait_stream(torch.cuda.current_stream(_dev()))
    for adjoint in (False, True):
        eng = ndp.BatchedNMPC(B, disturbance=True)
        eng.reset(b["xr"], b["ur"])
        x0, xr, ur = (_t(b[k]).requires_grad_(True) for k in ("x0", "xr", "ur"))
        ft = _t(f, torch.float32).requires_grad_(True)
        layer = (lambda *a, **k: control_step_trajectory(eng, *a, **k)[0]) if adjoint else ControlStep(eng, params=True)
        with torch.cuda.stream(side):
            u0 = layer(x0, xr, ur, f=ft)
            gr = torch.autograd.grad(u0, (x0, xr, ur, ft), g)
        side.synchronize()
        assert eng.sensitivity_level == (0 if adjoint else 1)
        grads.append([v.detach().cpu().numpy() for v in gr])
        its.append(eng.status())
        eng.close()
    st, it = its[0]
    ok = (st == 0) & ((it & 0xffff) == 0)
    assert ok.sum() >= 200 and np.array_equal(st, its[1][0])
    for a, c in zip(*grads):
        assert a.dtype == c.dtype
        s = np.maximum(1.0, np.abs(a[ok]).reshape(ok.sum(), -1).max(axis=1))
        err = np.abs(a[ok] - c[ok]).reshape(ok.sum(), -1).max(axis=1) / s
        assert err.max() <= (1e-6 if a.dtype == np.float32 else 1e-10), err.max()


def test_training_a_reference_offset_against_a_trajectory_loss(ndp):
    """Twenty Adam steps on a per-instance constant offset of the reference positions, through control_step_trajectory, against a loss on
    the predicted positions X[:, :, 0:3] (imitation of the plan the offset 0.3 gives): the loss falls below a tenth.  The iterate is restored
    before every step."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_trajectory
    B, N = 64, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 87)
    eng = ndp.BatchedNMPC(B)
    eng.reset(b["xr"], b["ur"])
    X0, U0 = eng.get_iterate()
    x0, xr, ur = (_t(b[k]) for k in ("x0", "xr", "ur"))
    mask = torch.zeros(1, 1, 10, dtype=torch.float64, device=_dev())
    mask[..., 0:3] = 1.0
    with torch.no_grad():
        eng.set_iterate(X0, U0)
        X_target = control_step_trajectory(eng, x0, (xr + 0.3 * mask).contiguous(), ur)[1][:, :, 0:3].clone()
    off = torch.zeros(B, 1, 1, dtype=torch.float64, device=_dev(), requires_grad=True)
    opt = torch.optim.Adam([off], lr=0.05)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.85)
    losses = []
    for _ in range(20):
        eng.set_iterate(X0, U0)
        X = control_step_trajectory(eng, x0, (xr + off * mask).contiguous(), ur)[1]
        loss = ((X[:, :, 0:3] - X_target) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(loss.item())
    eng.close()
    print("reference-offset training losses:", ["%.3e" % v for v in losses])
    assert losses[-1] < 0.1 * losses[0] and np.isfinite(losses).all()
