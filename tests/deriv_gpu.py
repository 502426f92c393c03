"""What the device tests of the control step's derivatives share (tests/test_*_gpu.py): the package fixture, tensors on cuda:0, a recorded
step with its tape, step_vjp_device and step_jvp_device (with and without a model direction) with -7.0-filled outputs, and random tangents."""
import numpy as np
import pytest

from tests.step_deriv_emu import MIXED  # noqa: F401    (bench.py's `mixed` workload)


@pytest.fixture(scope="module")
def ndp():
    import ndp_nmpc_qd_amd
    return ndp_nmpc_qd_amd


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=_dev(), dtype=dtype)


def _vjp(eng, x0, xr, ur, tape, f=None, gu0=None, gX=None, gU=None, model=False, guard=0):
    """step_vjp_device on torch tensors; returns numpy (gx0, gxr, gur, gf, u0_check, status_check[, gmodel]).  guard: the outputs are the
    first B rows of buffers with that many rows more, returned whole (the rows behind B keep their -7.0 / -1)."""
    import torch
    B, N = eng.B, eng.N
    R = B + guard
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    out = (z(R, 10), z(R, N + 1, 10), z(R, N, 4), z(R, N + 1, 3), z(R, 4))
    st = torch.full((R,), -1, dtype=torch.int32, device=_dev())
    gm = z(R, 16) if model else None
    eng.step_vjp_device(x0, xr, ur, tape, gu0=gu0, gX=gX, gU=gU, f=f, gx0=out[0][:B], gxr=out[1][:B], gur=out[2][:B], gf=out[3][:B],
                        u0_check=out[4][:B], status_check=st[:B], gmodel=gm[:B] if model else None)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) + (st.cpu().numpy(),) + ((gm.cpu().numpy(),) if model else ())


def _jvp(eng, x0, xr, ur, tape, T, f=None, tx0=None, txr=None, tur=None, tf=None, guard=0):
    """step_jvp_device on torch tensors with -7.0-filled outputs; returns numpy (du0 [B,T,4], dX, dU, u0_check, status_check).  guard: as
    _vjp's."""
    import torch
    B, N = eng.B, eng.N
    R = B + guard
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    out = (z(R, T, 4), z(R, T, N + 1, 10), z(R, T, N, 4), z(R, 4))
    st = torch.full((R,), -1, dtype=torch.int32, device=_dev())
    eng.step_jvp_device(x0, xr, ur, tape, tx0=tx0, txr=txr, tur=tur, tf=tf, f=f, du0=out[0][:B], dX=out[1][:B], dU=out[2][:B],
                        u0_check=out[3][:B], status_check=st[:B])
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) + (st.cpu().numpy(),)


def _mjvp(eng, x0, xr, ur, tape, tm, f=None, tx0=None, txr=None, tur=None, tf=None, guard=0):
    """step_jvp_device with tmodel ([B,T,16] numpy) on torch tensors with -7.0-filled outputs; returns numpy (du0 [B,T,4], dX, dU,
    u0_check, status_check).  guard: the outputs are the first B rows of buffers with that many rows more, returned whole."""
    import torch
    B, N, nt = eng.B, eng.N, tm.shape[1]
    R = B + guard
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    out = (z(R, nt, 4), z(R, nt, N + 1, 10), z(R, nt, N, 4), z(R, 4))
    st = torch.full((R,), -1, dtype=torch.int32, device=_dev())
    eng.step_jvp_device(x0, xr, ur, tape, tx0=tx0, txr=txr, tur=tur, tf=tf, f=f, du0=out[0][:B], dX=out[1][:B], dU=out[2][:B],
                        u0_check=out[3][:B], status_check=st[:B], tmodel=_t(tm))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) + (st.cpu().numpy(),)


def _tangents(seed, B, N, T, force=True):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(B, T, 10)), rng.normal(size=(B, T, N + 1, 10)), rng.normal(size=(B, T, N, 4)),
            rng.normal(size=(B, T, N + 1, 3)) if force else None)


def _tt(tan):
    return dict(zip(("tx0", "txr", "tur", "tf"), (None if t is None else _t(t) for t in tan)))


def _recorded_step(ndp, b, fused=False, f=None, params=False, prepare=None, **kw):
    """A fresh engine (prepare: called with it before its first step), one warm-up step (a kept set to start from), then the recorded step:
    tape, the step through update_device, and (params) today's Jacobians.  Returns a dict of everything the tests compare."""
    import torch
    B, N = b["x0"].shape[0], b["xr"].shape[1] - 1
    eng = ndp.BatchedNMPC(B, N=N, disturbance=fused or f is not None, **kw)
    eng.reset(b["xr"], b["ur"])
    if prepare is not None:
        prepare(eng)
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur")}
    ft = _t(f, torch.float32) if f is not None else None
    nb = dict(other=_t(b["other"]), ego_xy=_t(b["ego_xy"])) if fused else {}
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    eng.update_device(t["x0"], t["xr"], t["ur"], u0, f=ft, **nb)
    if params:
        eng.enable_sensitivity(1)
        eng.enable_param_sensitivity()
    tape = eng.record_tape()
    eng.update_device(t["x0"], t["xr"], t["ur"], u0, f=ft, **nb)
    eng.synchronize()                      # (the step went on the engine's own stream: torch's default one cannot be named)
    force = eng.device_force().clone() if fused else ft
    X, U = (v.clone() for v in eng.device_iterate())
    torch.cuda.synchronize()
    st, it = eng.status()
    _, act = eng.active_set()
    r = dict(eng=eng, t=t, tape=tape, force=force, u0=u0.cpu().numpy(), X=X.cpu().numpy(), U=U.cpu().numpy(), st=st, it=it, act=act)
    if params:
        r["K0"] = eng.sensitivity()[0]
        r["J"] = eng.param_sensitivity()
    return r
