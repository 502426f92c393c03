"""Forward mode of the control step along directions of the cost weights and the mass on the device (run with -m gpu):
ndp_step_jvp_model_device (rti_mjvp_kernel) against the dense reference of tests/model_jvp_ref.py, in duality with
ndp_step_vjp_model_device on the same tape, against ndp_step_jvp_device for a zero model direction, T directions against T calls,
isolation (engine state and tape untouched, repeatable), refusals and the torch layer.  CPU side: tests/test_step_model_jvp.py.

B = deriv_edges.DEVICE_B = 37 (ragged at four and at two instances per workgroup), the mixed workload with a supplied force
(deriv_edges.device_case, seed SEED: on the CPU oracle's twin all 37 are set finishes at N = 2, 13, 20 and 27, 3 / 8 / 8 / 8 of them
pinned), T = 3; N = 20 and 13 are the <20> and <0> kernels, N = 2 and 27 the ends of what they serve.

Bars: the dense reference 1e-9 of max(1, |z'|max) (tests/test_step_jvp_gpu.py's); duality 1e-10 of the largest term on set finishes and
1e-6 on interior-point finishes (its bars too)."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import model_jvp_ref as MR
from tests.deriv_edges import DEVICE_B, device_case
from tests.deriv_gpu import MIXED, _dev, _jvp, _mjvp, _recorded_step, _t, _tangents, _tt, _vjp, ndp  # noqa: F401
from tests.fixed_set_ref import scale

pytestmark = pytest.mark.gpu

SEED = synth.SEED0 + 300
HORIZONS = (20, 13, 2, 27)
T = 3
WHO = "ndp_step_jvp_model_device"


def _state(eng):
    return [v.cpu().numpy().copy() for v in eng.device_iterate()] + [eng.active_set()[1]]


@pytest.fixture(scope="module")
def runs(ndp):
    """Per horizon, once: the recorded step, the model direction alone and beside the data's (with two guard rows), the model gradient
    for a seeded upstream, and the engine's state and tape before and after.  Left unchanged."""
    out = {}
    for N in HORIZONS:
        B = DEVICE_B
        b, f = device_case(N, SEED)
        r = _recorded_step(ndp, b, f=f)
        eng = r["eng"]
        rng = np.random.default_rng(900 + N)
        tm = rng.normal(size=(B, T, 16))
        tan = _tangents(901 + N, B, N, T)
        ups = rng.normal(size=(B, 4)), rng.normal(size=(B, N + 1, 10)), rng.normal(size=(B, N, 4))
        before, tape0 = _state(eng), [v.cpu().numpy().copy() for v in r["tape"]]
        a = (r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"])
        model = _mjvp(eng, *a, tm, f=r["force"], guard=2)
        mixed = _mjvp(eng, *a, tm, f=r["force"], **_tt(tan))
        again = _mjvp(eng, *a, tm, f=r["force"], **_tt(tan))
        grad = _vjp(eng, *a, f=r["force"], gu0=_t(ups[0]), gX=_t(ups[1]), gU=_t(ups[2]), model=True)
        zero = _mjvp(eng, *a, np.zeros((B, T, 16)), f=r["force"], **_tt(tan))
        plain = _jvp(eng, *a, T, f=r["force"], **_tt(tan))
        ones = [_mjvp(eng, *a, np.ascontiguousarray(tm[:, d:d + 1]), f=r["force"], **_tt(tuple(np.ascontiguousarray(t[:, d:d + 1]) for t in tan)))
                for d in range(T)]
        after, tape1 = _state(eng), [v.cpu().numpy() for v in r["tape"]]
        eng.close()
        out[N] = dict(b=b, f=f, r=r, tm=tm, tan=tan, ups=ups, model=model, mixed=mixed, again=again, grad=grad, zero=zero, plain=plain,
                      ones=ones, before=before, after=after, tape0=tape0, tape1=tape1)
    return out


@pytest.mark.parametrize("N", HORIZONS)
def test_three_directions_match_the_dense_reference(runs, oracle, N):
    """12 seeded status-0 set finishes, 3 of them pinned, all three directions each, the model direction alone and beside the data's:
    within 1e-9 of max(1, |z'|max) of model_jvp_ref at the pre-step iterate and the step's final set; model alone: dX_0 exactly 0; mixed:
    dX_0 = tx0; du0 = dU_0 exactly; pinned rows of dU exactly 0; nothing written behind the last instance."""
    d = runs[N]
    b, f, r, tm, tan = d["b"], d["f"], d["r"], d["tm"], d["tan"]
    B = DEVICE_B
    Xl, Ul, _ = d["tape0"]
    assert np.array_equal(d["model"][4][:B], r["st"]) and np.array_equal(d["mixed"][4], r["st"])
    assert all((x[B:] == -7.0).all() for x in d["model"][:4]) and (d["model"][4][B:] == -1).all()
    ok = (r["st"] == 0) & ((r["it"] & 0xffff) == 0)
    pin = ok & r["act"].any(axis=(1, 2))
    assert ok.sum() >= 12 and pin.sum() >= 3, (int(ok.sum()), int(pin.sum()))
    rng = np.random.default_rng(4)
    idx = np.concatenate([rng.choice(np.flatnonzero(pin), 3, replace=False), rng.choice(np.flatnonzero(ok & ~pin), 9, replace=False)])
    cfg = oracle.default_cfg(N=N, use_fd=True)
    worst = worst_mixed = 0.0
    for i in idx:
        c = MR.model_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), Xl[i], Ul[i], r["act"][i])
        for k in range(T):
            for got, data, tag in ((d["model"], (), 0), (d["mixed"], tuple(t[i, k] for t in tan), 1)):
                ref = MR.model_jvp_apply(c, tm[i, k], *data)
                s = max(scale(x) for x in ref)
                e = max(np.max(np.abs(g[i, k] - x)) for g, x in zip(got[:3], ref)) / s
                if tag:
                    worst_mixed = max(worst_mixed, e)
                else:
                    worst = max(worst, e)
                assert e <= 1e-9, (i, k, tag, e)
    print(f"N={N}: worst distance from the dense reference: model direction {worst:.3e}, with the data's {worst_mixed:.3e} (bar 1e-9)")
    m, x = d["model"], d["mixed"]
    assert not m[1][:B][ok][:, :, 0].any() and np.array_equal(x[1][ok][:, :, 0], tan[0][ok])
    for o in (tuple(v[:B] for v in m), x):
        assert np.array_equal(o[0][ok], o[2][ok][:, :, 0])
        assert not o[2][ok][np.broadcast_to((r["act"][ok] != 0)[:, None], o[2][ok].shape)].any()
    assert np.abs(m[1][:B][ok]).max() > 1e-6


@pytest.mark.parametrize("N", HORIZONS)
def test_duality_with_the_model_gradient_on_the_device(runs, N):
    """<gz, JVP(theta', t)> = <VJP(gz), t> + sum_{j<15} gmodel[j] theta'_j against ndp_step_vjp_model_device on the same tape, per instance
    and direction: 1e-10 of the largest term on set finishes, 1e-6 on interior-point finishes; a failed step gives NaN everywhere."""
    d = runs[N]
    r, tm, tan, (gu0, gX, gU), j, a = d["r"], d["tm"], d["tan"], d["ups"], d["mixed"], d["grad"]
    B = DEVICE_B
    assert np.array_equal(j[4], r["st"]) and np.array_equal(j[3], a[4], equal_nan=True)
    ok = r["st"] == 0
    ipm = (r["it"] & 0xffff) > 0
    flat = lambda xs: np.concatenate([x.reshape(B, -1) for x in xs], axis=1)  # noqa: E731
    worst = {False: 0.0, True: 0.0}
    for k in range(T):
        lhs = [gu0 * j[0][:, k], gX * j[1][:, k], gU * j[2][:, k]]
        rhs = [g * t[:, k] for g, t in zip(a[:4], tan)] + [a[6][:, :15] * tm[:, k, :15]]
        mag = np.maximum(1.0, np.abs(flat(lhs + rhs)).max(axis=1))
        err = np.abs(flat(lhs).sum(axis=1) - flat(rhs).sum(axis=1)) / mag
        assert err[ok & ~ipm].max() <= 1e-10, (k, err[ok & ~ipm].max())
        worst[False] = max(worst[False], err[ok & ~ipm].max())
        if (ok & ipm).any():
            assert err[ok & ipm].max() <= 1e-6, (k, err[ok & ipm].max())
            worst[True] = max(worst[True], err[ok & ipm].max())
    print(f"N={N}: duality gap, set finishes {worst[False]:.3e} ({int((ok & ~ipm).sum())}), interior point {worst[True]:.3e} "
          f"({int((ok & ipm).sum())})")
    assert (ok & ~ipm).sum() >= 12
    for x in j[:3]:
        assert np.isnan(x[~ok]).all() and np.isfinite(x[ok]).all()


def test_duality_on_the_workload_of_the_plain_forward_modes_duality_test(ndp):
    """B = 256 mixed, N = 20 (test_duality_with_the_adjoint_on_the_device's batch and force: free, pinned and -- where the device has them
    -- interior-point finishes), one model and data direction and one upstream: 1e-10 on set finishes, 1e-6 on interior-point finishes."""
    B, N = 256, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 40, **MIXED)
    f = np.random.default_rng(5).normal(0.0, 0.3, (B, N + 1, 3)).astype(np.float32)
    r = _recorded_step(ndp, b, f=f)
    tan = _tangents(6, B, N, 1)
    rng = np.random.default_rng(7)
    gu0, gX, gU = rng.normal(size=(B, 4)), rng.normal(size=(B, N + 1, 10)), rng.normal(size=(B, N, 4))
    tm = rng.normal(size=(B, 1, 16))
    a4 = (r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"])
    j = _mjvp(r["eng"], *a4, tm, f=r["force"], **_tt(tan))
    a = _vjp(r["eng"], *a4, f=r["force"], gu0=_t(gu0), gX=_t(gX), gU=_t(gU), model=True)
    r["eng"].close()
    ok = r["st"] == 0
    ipm = (r["it"] & 0xffff) > 0
    pinned = r["act"].any(axis=(1, 2))
    assert (ok & ~ipm & ~pinned).sum() >= 100 and (ok & ~ipm & pinned).sum() >= 10
    lhs = [gu0 * j[0][:, 0], gX * j[1][:, 0], gU * j[2][:, 0]]
    rhs = [g * t[:, 0] for g, t in zip(a[:4], tan)] + [a[6][:, :15] * tm[:, 0, :15]]
    flat = lambda xs: np.concatenate([x.reshape(B, -1) for x in xs], axis=1)  # noqa: E731
    err = np.abs(flat(lhs).sum(axis=1) - flat(rhs).sum(axis=1)) / np.maximum(1.0, np.abs(flat(lhs + rhs)).max(axis=1))
    print(f"duality gap: set finishes {err[ok & ~ipm].max():.3e} ({int((ok & ~ipm).sum())}, {int((ok & ~ipm & pinned).sum())} pinned), "
          f"interior point {err[ok & ipm].max() if (ok & ipm).any() else 0.0:.3e} ({int((ok & ipm).sum())})")
    assert err[ok & ~ipm].max() <= 1e-10
    if (ok & ipm).any():
        assert err[ok & ipm].max() <= 1e-6
    for x in j[:3]:
        assert np.isnan(x[~ok]).all()


@pytest.mark.parametrize("N", HORIZONS)
def test_repeatable_t_against_one_zero_direction_and_state_untouched(runs, N):
    """Two calls give the same bits; T = 3 in one call equals three calls of one, bit for bit; with tmodel all zeros the outputs equal
    ndp_step_jvp_device's on the same data tangents as numbers (what include/ndp_nmpc.h states: the sign of a zero may differ); the
    engine's iterate and kept sets and the tape keep their bits over all of the fixture's calls."""
    d = runs[N]
    for x, y in zip(d["mixed"], d["again"]):
        assert np.array_equal(x, y, equal_nan=True)
    for k, one in enumerate(d["ones"]):
        for x, y in zip(d["mixed"][:3], one[:3]):
            assert np.array_equal(x[:, k], y[:, 0], equal_nan=True), k
    for x, y in zip(d["zero"], d["plain"]):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(d["before"], d["after"]):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(d["tape0"], d["tape1"]):
        assert np.array_equal(x, y)


def test_column_6_and_a_mass_direction_without_a_force_are_exact_zeros(ndp):
    """N = 13, B = 37: unit directions in column 6 and column 15 with a force, and in columns 6, 14, 15 on a step that read none, give
    exact zeros on every status-0 instance; the mass with a force does move the step."""
    N, B = 13, DEVICE_B
    b, f = device_case(N, SEED)
    e = np.eye(16)
    for force, cols, moves in ((f, (6, 15), False), (None, (6, 14, 15), False), (f, (14,), True)):
        r = _recorded_step(ndp, b, f=force)              # (no force: a use_fd = 0 engine)
        tm = np.ascontiguousarray(np.broadcast_to(e[list(cols)][None], (B, len(cols), 16)))
        out = _mjvp(r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], tm, f=r["force"])
        r["eng"].close()
        ok = r["st"] == 0
        assert ok.sum() >= 30
        if moves:
            assert np.abs(out[1][ok]).max() > 1e-9
        else:
            assert all(not x[ok].any() for x in out[:3])


def test_refusals_name_their_reason_and_launch_nothing(ndp):
    """-2 with the entry's name and a reason, the -7.0-filled outputs untouched: ndp_step_jvp_device's refusals, and a missing tmodel (the
    binding routes on tmodel, so that one goes through the C entry itself)."""
    import ctypes as C
    import torch
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731

    def refused(eng, b, what, nt=1, tape=None, **kw):
        B, N = eng.B, eng.N
        t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
        out = dict(du0=z(B, nt, 4), dX=z(B, nt, N + 1, 10), dU=z(B, nt, N, 4))
        args = dict(tmodel=z(B, nt, 16), **out)
        args.update(kw)
        with pytest.raises(ndp.NdpError, match=WHO + r".*\(-2\).*" + what):
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
    refused(eng, b, "n_tan must be 1..8", nt=9)
    refused(eng, b, "no output", du0=None, dX=None, dU=None)
    refused(eng, b, "force tangent needs use_fd", tf=z(B, 1, N + 1, 3))
    refused(eng, b, "disturbance force needs use_fd", f=torch.zeros(B, N + 1, 3, dtype=torch.float32, device=_dev()))
    X, U, A = eng.record_tape()
    refused(eng, b, "are required", tape=(None, U, A))
    # tmodel NULL at the C entry
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
    du0 = z(B, 1, 4)
    p = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    rc = eng._lib.ndp_step_jvp_model_device(eng._h, p(t["x0"]), p(t["xr"]), p(t["ur"]), None, p(X), p(U), p(A), 1, None, None, None, None, None,
                                            p(du0), None, None, None, None, None)
    assert rc == -2 and b"ndp_step_jvp_model_device" in eng._lib.ndp_last_error(eng._h)
    assert b"without it: ndp_step_jvp_device" in eng._lib.ndp_last_error(eng._h)
    torch.cuda.synchronize()
    assert (du0 == -7.0).all()
    eng.close()


def test_torch_layer_returns_the_direct_calls_bits(ndp):
    """control_step_jvp with tmodel: its tangents equal step_jvp_device's on its own tape, bit for bit, for [B,T,16], and [T,16] / [16]
    are that direction given to every instance; a direction without the T axis gives outputs without it; model_tangent puts the mass into
    both columns."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_jvp, model_tangent
    B, N = DEVICE_B, 20
    b, f = device_case(N, SEED)
    ft = _t(f, torch.float32)
    tan = [_t(v) for v in _tangents(12, B, N, 2)]
    tm = _t(np.random.default_rng(13).normal(size=(B, 2, 16)))
    side = torch.cuda.Stream(device=_dev())      # (a stream the C-ABI can name)
    side.wait_stream(torch.cuda.current_stream(_dev()))
    x0, xr, ur = (_t(b[k]) for k in ("x0", "xr", "ur"))
    eng = ndp.BatchedNMPC(B, disturbance=True)
    eng.reset(b["xr"], b["ur"])

    def rewind(tape):
        eng.set_iterate(*(v.cpu().numpy() for v in tape[:2]))
        eng.set_active_set(tape[2].cpu().numpy())

    with torch.cuda.stream(side):
        tape = eng.record_tape(side)
        got = control_step_jvp(eng, x0, xr, ur, tan, f=ft, tmodel=tm)
        direct = [torch.full_like(v, -7.0) for v in got[3:]]
        eng.step_jvp_device(x0, xr, ur, tape, *tan, f=ft, du0=direct[0], dX=direct[1], dU=direct[2], stream=side, tmodel=tm)
        rewind(tape)
        shared_dir = control_step_jvp(eng, x0, xr, ur, (None,) * 4, f=ft, tmodel=tm[0])
        want_shared = [torch.full_like(v, -7.0) for v in shared_dir[3:]]
        eng.step_jvp_device(x0, xr, ur, tape, f=ft, du0=want_shared[0], dX=want_shared[1], dU=want_shared[2], stream=side,
                            tmodel=tm[0].expand(B, 2, 16).contiguous())
        rewind(tape)
        mt = model_tangent(tQd=tm[0, 0, :10], tRd=tm[0, 0, 10:14], tmass=tm[0, 0, 14])
        one = control_step_jvp(eng, x0, xr, ur, (None,) * 4, f=ft, tmodel=mt)
    side.synchronize()
    eng.close()
    assert mt.shape == (16,) and mt[15] == mt[14]
    for x, y in zip(got[3:], direct):
        assert torch.allclose(x, y, rtol=0, atol=0, equal_nan=True)
    for x, y in zip(shared_dir[3:], want_shared):
        assert torch.allclose(x, y, rtol=0, atol=0, equal_nan=True)
    assert one[3].shape == (B, 4) and one[4].shape == (B, N + 1, 10) and one[5].shape == (B, N, 4)
    for x, y in zip(one[3:], shared_dir[3:]):                      # (column 15 is not read by the step)
        assert torch.allclose(x, y[:, 0], rtol=0, atol=0, equal_nan=True)
