"""The forward-mode derivative of the control step on the device (run with -m gpu): rti_jvp_kernel against the dense fixed-set reference
(tests/fixed_set_ref.py), ragged workgroups, duality against ndp_step_vjp_device, consistency with the level-2 and parameter sensitivities,
isolation (engine state and tape untouched, repeatable), refusals, and the torch layer.  CPU side: tests/test_step_jvp.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests.deriv_gpu import MIXED, _dev, _jvp, _recorded_step, _t, _tangents, _tt, _vjp, ndp  # noqa: F401
from tests.fixed_set_ref import jvp_apply, jvp_system, scale

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dense(ndp):
    """B = 64 mixed with a supplied force at N = 20 and N = 13 (both kernels), T = 3: the recorded step and its tangents, shared by the dense
    and the ragged test."""
    runs = {}
    for N in (20, 13):
        B = 64
        b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
        f = np.random.default_rng(2).normal(0.0, 0.3, (B, N + 1, 3)).astype(np.float32)
        r = _recorded_step(ndp, b, f=f, params=False)
        tan = _tangents(3, B, N, 3)
        out = _jvp(r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], 3, f=r["force"], **_tt(tan))
        tape = [v.cpu().numpy() for v in r["tape"]]
        r["eng"].close()
        runs[N] = dict(b=b, f=f, r=r, tan=tan, out=out, tape=tape)
    return runs


@pytest.mark.parametrize("N", [20, 13])
def test_three_directions_match_the_dense_reference(dense, oracle, N):
    """12 seeded status-0 set finishes, at least 3 of them pinned, all three directions each: within 1e-9 of max(1, |z'|max) of jvp_ref at
    the pre-step iterate and the step's final set; dX_0 = tx0 and du0 = dU_0 exactly; pinned rows of dU exactly 0."""
    d = dense[N]
    b, f, r, tan, out = d["b"], d["f"], d["r"], d["tan"], d["out"]
    Xl, Ul, _ = d["tape"]
    assert np.array_equal(out[4], r["st"])
    ok = (r["st"] == 0) & ((r["it"] & 0xffff) == 0)
    pin = ok & r["act"].any(axis=(1, 2))
    assert ok.sum() >= 40 and pin.sum() >= 3
    rng = np.random.default_rng(4)
    idx = np.concatenate([rng.choice(np.flatnonzero(pin), 3, replace=False), rng.choice(np.flatnonzero(ok & ~pin), 9, replace=False)])
    cfg = oracle.default_cfg(N=N, use_fd=True)
    worst = 0.0
    for i in idx:
        c = jvp_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), Xl[i], Ul[i], r["act"][i])
        for k in range(3):
            ref = jvp_apply(c, *(t[i, k] for t in tan))[:3]
            s = max(scale(x) for x in ref)
            for got, x in zip(out[:3], ref):
                worst = max(worst, np.max(np.abs(got[i, k] - x)) / s)
                assert np.max(np.abs(got[i, k] - x)) <= 1e-9 * s, (i, k, np.max(np.abs(got[i, k] - x)) / s)
    print(f"N={N}: worst distance from the dense reference {worst:.3e}")
    assert np.array_equal(out[1][ok][:, :, 0], tan[0][ok]) and np.array_equal(out[0][ok], out[2][ok][:, :, 0])
    assert not out[2][ok][np.broadcast_to((r["act"][ok] != 0)[:, None], out[2][ok].shape)].any()


@pytest.mark.parametrize("N,B", [(20, 5), (20, 7), (13, 5), (13, 7)])
def test_ragged_workgroups_give_the_full_batch_results(ndp, dense, N, B):
    """A batch that fills no whole number of workgroups: every instance of B = 5 and B = 7 equals the matching instance of the B = 64 run on
    the same inputs, bit for bit (an instance is one wave and sees nothing of the others), and nothing is written behind the last one: the
    outputs are the first B rows of buffers with two guard rows, which keep their -7.0."""
    import torch
    d = dense[N]
    b = {k: v[:B] for k, v in d["b"].items() if isinstance(v, np.ndarray) and v.shape[:1] == (64,)}
    r = _recorded_step(ndp, b, f=d["f"][:B], params=False)
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    big = (z(B + 2, 3, 4), z(B + 2, 3, N + 1, 10), z(B + 2, 3, N, 4), z(B + 2, 4))
    st = torch.full((B + 2,), -1, dtype=torch.int32, device=_dev())
    r["eng"].step_jvp_device(r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], **_tt(tuple(t[:B] for t in d["tan"])), f=r["force"],
                             du0=big[0][:B], dX=big[1][:B], dU=big[2][:B], u0_check=big[3][:B], status_check=st[:B])
    torch.cuda.synchronize()
    r["eng"].close()
    out = [v.cpu().numpy() for v in big] + [st.cpu().numpy()]
    for x, y in zip(out, d["out"]):
        assert np.array_equal(x[:B], y[:B], equal_nan=True)
    assert all((x[B:] == -7.0).all() for x in out[:4]) and (out[4][B:] == -1).all()


def test_duality_with_the_adjoint_on_the_device(ndp):
    """B = 256 mixed, N = 20, one random direction and one random upstream on the same tape: <gz, JVP(t)> = <VJP(gz), t> against
    ndp_step_vjp_device, within 1e-10 of the larger side's magnitude (the largest |term|, at least 1) on set finishes -- free and pinned --
    and 1e-6 on interior-point finishes (the barrier-weighted system: the split test_gu0_only_matches_the_jacobians... uses)."""
    B, N = 256, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 40, **MIXED)
    f = np.random.default_rng(5).normal(0.0, 0.3, (B, N + 1, 3)).astype(np.float32)
    r = _recorded_step(ndp, b, f=f, params=False)
    tan = _tangents(6, B, N, 1)
    rng = np.random.default_rng(7)
    gu0, gX, gU = rng.normal(size=(B, 4)), rng.normal(size=(B, N + 1, 10)), rng.normal(size=(B, N, 4))
    j = _jvp(r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], 1, f=r["force"], **_tt(tan))
    a = _vjp(r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], f=r["force"], gu0=_t(gu0), gX=_t(gX), gU=_t(gU))
    r["eng"].close()
    assert np.array_equal(j[4], r["st"]) and np.array_equal(j[3], a[4], equal_nan=True)
    ok = r["st"] == 0
    ipm = (r["it"] & 0xffff) > 0
    pinned = r["act"].any(axis=(1, 2))
    assert (ok & ~ipm & ~pinned).sum() >= 100 and (ok & ~ipm & pinned).sum() >= 10
    lhs = [gu0 * j[0][:, 0], gX * j[1][:, 0], gU * j[2][:, 0]]
    rhs = [g * t[:, 0] for g, t in zip(a[:4], tan)]
    flat = lambda xs: np.concatenate([x.reshape(B, -1) for x in xs], axis=1)  # noqa: E731
    mag = np.maximum(1.0, np.abs(flat(lhs + rhs)).max(axis=1))
    err = np.abs(flat(lhs).sum(axis=1) - flat(rhs).sum(axis=1)) / mag
    print(f"duality gap: set finishes {err[ok & ~ipm].max():.3e} ({int((ok & ~ipm).sum())}, {int((ok & ~ipm & pinned).sum())} pinned), "
          f"interior point {err[ok & ipm].max() if (ok & ipm).any() else 0.0:.3e} ({int((ok & ipm).sum())})")
    assert err[ok & ~ipm].max() <= 1e-10
    if (ok & ipm).any():
        assert err[ok & ipm].max() <= 1e-6
    for x in j[:3]:
        assert np.isnan(x[~ok]).all()


def test_unit_directions_reproduce_the_sensitivities_that_exist(ndp):
    """tx0 = e_j for j = 0..7 in one call (T = 8) and j = 8, 9 in a second (T = 2) reproduce the columns of the level-2 dX/dx0 and dU/dx0 of
    the recorded step; a random (txr, tur, tf) direction reproduces du0/dxr . txr + du0/dur . tur + du0/df . tf from ndp_get_sens_params.
    Both within 1e-10 of max(1, |value|max) on set finishes."""
    import torch
    B, N = 256, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 40, **MIXED)
    f = np.random.default_rng(8).normal(0.0, 0.3, (B, N + 1, 3)).astype(np.float32)
    eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
    eng.reset(b["xr"], b["ur"])
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
    ft = _t(f, torch.float32)
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    eng.update_device(t["x0"], t["xr"], t["ur"], u0, f=ft)
    eng.enable_sensitivity(2)
    eng.enable_param_sensitivity()
    tape = eng.record_tape()
    eng.update_device(t["x0"], t["xr"], t["ur"], u0, f=ft)
    eng.synchronize()
    st, it = eng.status()
    _, dU, dX = eng.sensitivity()
    dxr, dur, df = eng.param_sensitivity()
    eye = np.broadcast_to(np.eye(10)[None], (B, 10, 10))
    cols = [_jvp(eng, t["x0"], t["xr"], t["ur"], tape, T, f=ft, tx0=_t(eye[:, lo:lo + T])) for lo, T in ((0, 8), (8, 2))]
    tan = _tangents(9, B, N, 1)
    p = _jvp(eng, t["x0"], t["xr"], t["ur"], tape, 1, f=ft, **_tt((None,) + tan[1:]))
    eng.close()
    ok = (st == 0) & ((it & 0xffff) == 0)
    assert ok.sum() >= 200
    jX = np.concatenate([c[1] for c in cols], axis=1)          # [B, 10 (j), N+1, 10]
    jU = np.concatenate([c[2] for c in cols], axis=1)
    for got, ref in ((jX, dX.transpose(0, 3, 1, 2)), (jU, dU.transpose(0, 3, 1, 2))):
        s = np.maximum(1.0, np.abs(ref[ok]).reshape(ok.sum(), -1).max(axis=1))
        err = np.abs(got[ok] - ref[ok]).reshape(ok.sum(), -1).max(axis=1) / s
        assert err.max() <= 1e-10, err.max()
    ref = (np.einsum("bikj,bkj->bi", dxr, tan[1][:, 0]) + np.einsum("bikj,bkj->bi", dur, tan[2][:, 0])
           + np.einsum("bikj,bkj->bi", df, tan[3][:, 0]))
    s = np.maximum(1.0, np.abs(ref[ok]).max(axis=1))
    err = np.abs(p[0][ok][:, 0] - ref[ok]).max(axis=1) / s
    assert err.max() <= 1e-10, err.max()


def test_state_and_tape_untouched_and_repeatable(ndp):
    """A JVP call leaves the engine's iterate, kept sets and sensitivity buffers bit-unchanged, and the tape too; two calls on one tape give
    bit-identical tangents; the recompute's u0 and status equal the recorded (fused) step's, bit for bit; a NaN state gives NaN only for its own instance."""
    B, N = 256, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 40, downwash=True, **MIXED)
    b["x0"][5, 3] = np.nan
    r = _recorded_step(ndp, b, fused=True, params=True)
    eng = r["eng"]
    before = [v.cpu().numpy().copy() for v in eng.device_iterate()] + [eng.active_set()[1], *eng.sensitivity()[:1], *eng.param_sensitivity()]
    tape0 = [v.cpu().numpy().copy() for v in r["tape"]]
    tan = _tt(_tangents(10, B, N, 2))
    a = _jvp(eng, r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], 2, f=r["force"], **tan)
    c = _jvp(eng, r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], 2, f=r["force"], **tan)
    after = [v.cpu().numpy() for v in eng.device_iterate()] + [eng.active_set()[1], *eng.sensitivity()[:1], *eng.param_sensitivity()]
    eng.close()
    for x, y in zip(before, after):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(tape0, r["tape"]):
        assert np.array_equal(x, y.cpu().numpy())
    for x, y in zip(a, c):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(a[4], r["st"]) and r["st"][5] != 0
    keep = (np.arange(B) != 5) & (r["st"] == 0)
    assert np.array_equal(a[3][keep], r["u0"][keep])     # (the fused step: the recompute's arithmetic is the step's, bit for bit)
    for x in a[:3]:
        assert np.isnan(x[5]).all() and np.isfinite(x[keep]).all()


def test_refusals_name_their_reason_and_launch_nothing(ndp):
    import torch
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731

    def refused(eng, b, what, T=1, tape=None, **kw):
        B, N = eng.B, eng.N
        t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
        out = dict(du0=z(B, T, 4), dX=z(B, T, N + 1, 10), dU=z(B, T, N, 4))
        args = dict(tx0=z(B, T, 10), **out)
        args.update(kw)
        with pytest.raises(ndp.NdpError, match=r"\(-2\).*" + what):
            eng.step_jvp_device(t["x0"], t["xr"], t["ur"], tape or eng.record_tape(), **args)
        torch.cuda.synchronize()
        assert all((v == -7.0).all() for v in out.values())

    for kw, N, what in ((dict(n_rti=2), 20, "n_rti = 1"), (dict(qp_precision=1), 20, "qp_precision 0"), ({}, 40, "N <= 27")):
        b = synth.make_batch(64, N=N, seed=synth.SEED0 + 85, **MIXED)
        eng = ndp.BatchedNMPC(64, N=N, **kw)
        eng.reset(b["xr"], b["ur"])
        refused(eng, b, what)
        eng.close()
    B, N = 64, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 85, **MIXED)
    eng = ndp.BatchedNMPC(B)                            # (no disturbance model: use_fd = 0)
    eng.reset(b["xr"], b["ur"])
    refused(eng, b, "n_tan must be 1..8", T=9)
    refused(eng, b, "n_tan must be 1..8", T=0)
    refused(eng, b, "no tangent", tx0=None)
    refused(eng, b, "no output", du0=None, dX=None, dU=None)
    refused(eng, b, "force tangent needs use_fd", tf=z(B, 1, N + 1, 3))
    refused(eng, b, "disturbance force needs use_fd", f=torch.zeros(B, N + 1, 3, dtype=torch.float32, device=_dev()))
    X, U, A = eng.record_tape()
    refused(eng, b, "are required", tape=(None, U, A))
    eng.close()


def test_torch_layer_returns_the_step_and_the_direct_tangents(ndp):
    """control_step_jvp's u0, X, U equal control_step_trajectory's on a second engine with the same inputs, bit for bit, and its tangents
    equal step_jvp_device's on its own tape; a direction without the T axis gives outputs without it."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_jvp, control_step_trajectory
    B, N = 64, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 40, **MIXED)
    f = _t(np.random.default_rng(11).normal(0.0, 0.4, (B, N + 1, 3)).astype(np.float32), torch.float32)
    tan = [None if v is None else _t(v) for v in _tangents(12, B, N, 2)]
    side = torch.cuda.Stream(device=_dev())      # (a stream the C-ABI can name)
    side.wait_stream(torch.cuda.current_stream(_dev()))
    x0, xr, ur = (_t(b[k]) for k in ("x0", "xr", "ur"))
    engs = [ndp.BatchedNMPC(B, disturbance=True) for _ in range(2)]
    for e in engs:
        e.reset(b["xr"], b["ur"])
    with torch.cuda.stream(side):
        tape = engs[0].record_tape(side)
        got = control_step_jvp(engs[0], x0, xr, ur, tan, f=f)
        with torch.no_grad():
            want = control_step_trajectory(engs[1], x0, xr, ur, f=f)
        direct = [torch.full_like(v, -7.0) for v in got[3:]]
        engs[0].step_jvp_device(x0, xr, ur, tape, *tan, f=f, du0=direct[0], dX=direct[1], dU=direct[2], stream=side)
        engs[0].set_iterate(*(v.cpu().numpy() for v in tape[:2]))
        engs[0].set_active_set(tape[2].cpu().numpy())
        one = control_step_jvp(engs[0], x0, xr, ur, [None if v is None else v[:, 0].contiguous() for v in tan], f=f)
    side.synchronize()
    for e in engs:
        e.close()
    assert not any(v.requires_grad for v in got)
    for x, y in zip(got, tuple(want) + tuple(direct)):
        assert torch.allclose(x, y, rtol=0, atol=0, equal_nan=True)
    assert one[3].shape == (B, 4) and one[4].shape == (B, N + 1, 10) and one[5].shape == (B, N, 4)
    for x, y in zip(one[3:], got[3:]):
        assert torch.allclose(x, y[:, 0], rtol=0, atol=0, equal_nan=True)
