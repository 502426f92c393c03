"""The derivatives of the K-neighbour downwash on the device (run with -m gpu): ndp_downwash_multi_vjp_device and
ndp_downwash_multi_jvp_device against their single-neighbour siblings bit for bit (per slot, at K = 1, two calls, T directions against T
calls, shared rows and the same row twice), against the float64 reference (tests/mlp_multi_deriv_ref.py) on own-row inputs with redrawn
rows, closed and empty slots, a non-finite upstream row, isolation, refusals, control_step_ndp_multi end to end and a training-shaped loop.
CPU side: tests/test_downwash_multi_deriv.py.

Bars (the project's 1e-5 for this network): every parameter group max|err| <= 1e-5 max|reference group|; |df - ref| <= 1e-5 max(1,
max|ref| of the row).  No row is dropped from a reference comparison: rows below the margin are redrawn (mlp_multi_deriv_ref)."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag, synth
from tests import mlp_multi_deriv_ref as M
from tests import mlp_vjp_ref as R
from tests.deriv_gpu import MIXED, _dev, _t, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

N = 20
BAR = 1e-5
# 105 rows: a last tile of 9 rows, one workgroup for 1 (K = 1) or 7 (K = 8) workgroups of work; 147 rows: a second workgroup with one
# wave, 4 workgroups of work on 2; 64 instances: 11 workgroups for 21 / 32 of work -- the accumulators, the LDS image and the flags go
# through a second grid-stride round everywhere but at K = 1
SHAPES = [(5, 1), (5, 8), (7, 3), (64, 2), (64, 3)]
REF_SHAPES = [(64, 3), (7, 3), (2048, 2)]


@pytest.fixture(scope="module")
def engines(ndp):
    made = {}

    def get(B):
        if B not in made:
            made[B] = ndp.BatchedNMPC(B, N=N, disturbance=True)
        return made[B]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def blob():
    return _lib.load_weights()


_own = {}


def _own_case(blob, B, K, gates):
    """tests/mlp_multi_deriv_ref.own_row_case, made once per (B, K, gates) and shared (nothing changes it)."""
    if (B, K, gates) not in _own:
        _own[B, K, gates] = M.own_row_case(1000 + 10 * B + K + (500 if gates == "mixed" else 0), blob, B, K, N, gates)
    return _own[B, K, gates]


def _shared_case(seed, B, K):
    """Several instances and slots on one row of `other`, the same row twice in instance 0, empty slots, about 40 % of the gates open.
    Device against device only: nothing here is drawn for a reference."""
    rng = np.random.default_rng(seed)
    rows = max(3, (B * K) // 3)
    xr = rng.normal(0.0, 0.7, (B, N + 1, 10))
    other = rng.normal(0.0, 0.7, (rows, N + 1, 10))
    idx = rng.integers(0, rows, (B, K)).astype(np.int32)
    idx[rng.random((B, K)) < 0.2] = -1
    idx[0, :] = 1                                              # the same row in every slot of instance 0 ...
    ego_xy = rng.normal(0.0, 0.7, (B, 2))
    ego_xy[0] = other[1, 0, :2] + 0.1                          # ... and its gate open
    d = other[np.clip(idx, 0, None)][:, :, 0, :2] - ego_xy[:, None]
    open_ = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] < 1.0) & (idx >= 0)
    return dict(other=other, index=idx, xr=xr, ego_xy=ego_xy, open=open_)


def _args(c):
    return _t(c["other"]), _t(c["index"]), _t(c["xr"]), None if c["ego_xy"] is None else _t(c["ego_xy"])


def _multi_vjp(eng, c, gf, want_gz=True, want_gw=True):
    import torch
    B, K = c["index"].shape
    other, idx, xr, exy = _args(c)
    gz = torch.full((B, K, N + 1, 6), -7.0, dtype=torch.float64, device=_dev()) if want_gz else None
    gw = torch.full((mlp_frag.NPARAM,), -7.0, dtype=torch.float32, device=_dev()) if want_gw else None
    eng.downwash_multi_vjp_device(other, idx, xr, _t(gf), ego_xy=exy, gz=gz, gw=gw)
    eng.synchronize()
    torch.cuda.synchronize()
    return None if gz is None else gz.cpu().numpy(), None if gw is None else gw.cpu().numpy()


def _single_vjp(eng, c, k, gf):
    import torch
    B = c["index"].shape[0]
    other, _, xr, exy = _args(c)
    gz = torch.full((B, N + 1, 6), -7.0, dtype=torch.float64, device=_dev())
    gw = torch.full((mlp_frag.NPARAM,), -7.0, dtype=torch.float32, device=_dev())
    eng.downwash_vjp_device(other, xr, _t(gf), ego_xy=exy, other_index=_t(c["index"][:, k]), gz=gz, gw=gw)
    eng.synchronize()
    torch.cuda.synchronize()
    return gz.cpu().numpy(), gw.cpu().numpy()


def _multi_jvp(eng, c, tz, tw, T):
    """downwash_multi_jvp_device into buffers filled with -7.0 (stale memory a sum must not start from); numpy (df, f_check)."""
    import torch
    B = c["index"].shape[0]
    other, idx, xr, exy = _args(c)
    df = torch.full((B, T, N + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    fc = torch.full((B, N + 1, 3), -7.0, dtype=torch.float32, device=_dev())
    eng.downwash_multi_jvp_device(other, idx, xr, tz=None if tz is None else _t(tz), tw=None if tw is None else _t(tw), ego_xy=exy, n_tan=T,
                                  df=df, f_check=fc)
    eng.synchronize()
    torch.cuda.synchronize()
    return df.cpu().numpy(), fc.cpu().numpy()


def _single_jvp(eng, c, k, tz, tw, T):
    import torch
    B = c["index"].shape[0]
    other, _, xr, exy = _args(c)
    df = torch.full((B, T, N + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    eng.downwash_jvp_device(other, xr, tz=None if tz is None else _t(tz[:, :, k]), tw=None if tw is None else _t(tw), ego_xy=exy,
                            other_index=_t(c["index"][:, k]), n_tan=T, df=df)
    eng.synchronize()
    torch.cuda.synchronize()
    return df.cpu().numpy()


def _multi_forward(eng, c):
    import torch
    B = c["index"].shape[0]
    other, idx, xr, exy = _args(c)
    f = torch.full((B, N + 1, 3), -7.0, dtype=torch.float32, device=_dev())
    eng.downwash_multi_device(other, idx, xr, f, ego_xy=exy)
    eng.synchronize()
    torch.cuda.synchronize()
    return f.cpu().numpy()


def _directions(seed, blob, B, K, T):
    rng = np.random.default_rng(seed)
    tz = rng.normal(size=(B, T, K, N + 1, 6))
    tw = (np.asarray(blob, dtype=np.float64)[None] * 0.1 * rng.normal(size=(T, mlp_frag.NPARAM))).astype(np.float32)
    return tz, tw


# ---------------------------------------------------------------- bit-equality with the single-neighbour calls
@pytest.mark.parametrize("rows", ["own", "shared"])
@pytest.mark.parametrize("B,K", SHAPES)
def test_bit_equal_to_the_single_neighbour_calls_per_slot(engines, blob, B, K, rows):
    """g_z[:, k] is what ndp_downwash_vjp_device writes for other_index[:, k]; df is the float64 sum in slot order of what
    ndp_downwash_jvp_device gives per slot (T = 4 in one call = four calls); f_check is ndp_downwash_multi_device's force; two calls give
    the same bits; at K = 1 g_w and df are the single-neighbour call's."""
    c = _own_case(blob, B, K, "mixed") if rows == "own" else _shared_case(40 + B + K, B, K)
    eng = engines(B)
    op = c["open"]
    if K > 1:
        assert op.any() and not op.all() and (~op[:, 0] & op[:, 1:].any(axis=1)).any()
    rng = np.random.default_rng(B * K)
    gf = rng.normal(size=(B, N + 1, 3))
    gz, gw = _multi_vjp(eng, c, gf)
    gz2, gw2 = _multi_vjp(eng, c, gf)
    assert np.array_equal(gz, gz2) and np.array_equal(gw, gw2)
    assert not gz[~op].any() and np.abs(gz[op]).max(axis=(1, 2)).min() > 0
    singles = [_single_vjp(eng, c, k, gf) for k in range(K)]
    for k in range(K):
        assert np.array_equal(gz[:, k], singles[k][0]), k
    gz_only, _ = _multi_vjp(eng, c, gf, want_gw=False)
    _, gw_only = _multi_vjp(eng, c, gf, want_gz=False)
    assert np.array_equal(gz_only, gz) and np.array_equal(gw_only, gw)
    if K == 1:
        assert np.array_equal(gw, singles[0][1])
    else:                                                      # not promised bit-equal (the order differs), but the same sum
        tot = np.sum([s[1].astype(np.float64) for s in singles], axis=0)
        assert np.abs(gw - tot).max() <= 1e-4 * max(1.0, np.abs(tot).max())
    T = 4
    tz, tw = _directions(7 + B + K, blob, B, K, T)
    df, fc = _multi_jvp(eng, c, tz, tw, T)
    assert np.array_equal(fc, _multi_forward(eng, c))
    acc = None
    for k in range(K):
        d = _single_jvp(eng, c, k, tz, tw, T)
        assert not d[~op[:, k]].any()
        acc = d if acc is None else acc + d
    assert np.array_equal(df, acc)
    assert not df[~op.any(axis=1)].any() and np.abs(df[op.any(axis=1)]).max(axis=(1, 2, 3)).min() > 0
    for t in range(T):
        one, _ = _multi_jvp(eng, c, tz[:, t:t + 1], tw[t:t + 1], 1)
        assert np.array_equal(one[:, 0], df[:, t]), t
    dz, _ = _multi_jvp(eng, c, tz, None, T)                   # one kind of direction alone
    dw, _ = _multi_jvp(eng, c, None, tw, T)
    assert np.abs(dz + dw - df).max() <= 1e-3 * max(1.0, np.abs(df).max())      # (linear in the direction, up to fp32 rounding)


# ---------------------------------------------------------------- against the float64 reference
@pytest.mark.parametrize("gates", ["open", "mixed"])
@pytest.mark.parametrize("B,K", REF_SHAPES)
def test_against_the_float64_reference(ndp, engines, blob, B, K, gates):
    """g_w (every parameter group) and df (T = 2: the rows' direction alone, then rows and weights) on the own-row inputs; (2048, 2) is 672
    workgroups of work on the 256 the workspace has rows for.  g_z per slot is held to the single-neighbour bar as well."""
    c = _own_case(blob, B, K, gates)
    eng = engines(B) if B <= 64 else ndp.BatchedNMPC(B, N=N, disturbance=True)
    rng = np.random.default_rng(3 * B + K)
    gf = rng.normal(size=(B, N + 1, 3))
    gz, gw = _multi_vjp(eng, c, gf)
    T = 2
    tz, tw = _directions(11 + B + K, blob, B, K, T)
    tw[0] = 0.0
    df, _ = _multi_jvp(eng, c, tz, tw, T)
    if B > 64:
        eng.close()
    rz, rw, margin = M.vjp64(blob, c["z"], c["open"], gf)
    assert margin.min() >= R.MARGIN                            # nothing to drop: the rows below the margin were redrawn
    ge = R.group_errors(gw, rw)
    err_z = (np.abs(gz - rz).max(axis=3) / np.maximum(1.0, np.abs(rz).max(axis=3))).max()
    err_d = 0.0
    for t in range(T):
        rd = M.jvp64(blob, c["z"], c["open"], tz[:, t], tw[t])
        err_d = max(err_d, float((np.abs(df[:, t] - rd).max(axis=2) / np.maximum(1.0, np.abs(rd).max(axis=2))).max()))
    print(f"B = {B} K = {K} {gates}: {int(c['open'].sum())} of {B * K} slots open, {c['redrawn']} rows redrawn in {c['rounds']} rounds; "
          f"g_z {err_z:.3e}, df {err_d:.3e}; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert max(ge.values()) <= BAR, ge
    assert err_d <= BAR and err_z <= BAR


# ---------------------------------------------------------------- closed and empty slots, a non-finite upstream row
@pytest.mark.parametrize("how", ["empty", "closed"])
def test_every_slot_closed_or_empty_gives_exact_zeros(engines, blob, how):
    B, K = 7, 3
    c = dict(_own_case(blob, B, K, "mixed"))
    if how == "empty":
        c["index"] = np.full((B, K), -1, dtype=np.int32)
    else:
        c["ego_xy"] = c["ego_xy"] + 50.0
    gf = np.random.default_rng(1).normal(size=(B, N + 1, 3))
    gz, gw = _multi_vjp(engines(B), c, gf)
    tz, tw = _directions(2, blob, B, K, 2)
    df, fc = _multi_jvp(engines(B), c, tz, tw, 2)
    assert not gz.any() and not gw.any() and not df.any() and not fc.any()


def test_a_non_finite_upstream_row_stays_out_of_the_weights(engines, blob):
    B, K = 64, 3
    c = _own_case(blob, B, K, "mixed")
    op = c["open"]
    i = int(np.flatnonzero(op.any(axis=1) & ~op.all(axis=1))[0])          # an instance with an open and a closed slot
    gf = np.random.default_rng(4).normal(size=(B, N + 1, 3))
    bad, zeroed = gf.copy(), gf.copy()
    bad[i, 4, 1], bad[i, 9, 0] = np.nan, np.inf
    zeroed[i, 4], zeroed[i, 9] = 0.0, 0.0
    gz, gw = _multi_vjp(engines(B), c, bad)
    gz0, gw0 = _multi_vjp(engines(B), c, zeroed)
    assert np.isfinite(gw).all() and np.array_equal(gw, gw0)
    for n in (4, 9):
        assert np.isnan(gz[i, op[i], n]).all() and not gz[i, ~op[i], n].any()
    gz[i, :, (4, 9)] = 0.0
    gz0[i, :, (4, 9)] = 0.0
    assert np.isfinite(gz).all() and np.array_equal(gz, gz0)


# ---------------------------------------------------------------- isolation
def test_the_engine_is_untouched(ndp, blob):
    import torch
    B, K = 64, 2
    b = synth.make_batch(B, seed=synth.SEED0 + 90, downwash=True, **MIXED)
    c = _shared_case(5, B, K)
    c["xr"] = b["xr"]
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())

    def engine():
        e = ndp.BatchedNMPC(B, N=N, disturbance=True)
        e.reset(b["xr"], b["ur"])
        return e
    e = engine()
    step = lambda e: (e.update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"]), e.synchronize())  # noqa: E731
    step(e)
    state = lambda: [v.clone() for v in e.device_iterate()] + [e.device_force().clone(), torch.as_tensor(e.active_set()[1]),  # noqa: E731
                                                                 *(torch.as_tensor(a) for a in e.debug_mlp_fragments())]
    before = state()
    gf = np.random.default_rng(5).normal(size=(B, N + 1, 3))
    tz, tw = _directions(6, blob, B, K, 2)
    gz, gw = _multi_vjp(e, c, gf)
    df, _ = _multi_jvp(e, c, tz, tw, 2)
    assert np.abs(gw).max() > 0 and np.abs(df).max() > 0
    for x, y in zip(before, state()):
        assert torch.equal(x.cpu(), y.cpu())
    step(e)
    with_calls = u0.cpu().numpy().copy()
    e.close()
    e = engine()                                               # the same two steps without the calls in between
    step(e)
    step(e)
    assert np.array_equal(with_calls, u0.cpu().numpy())
    e.close()


# ---------------------------------------------------------------- refusals
def test_refusals_name_their_reason_and_leave_the_outputs_untouched(ndp, blob):
    import torch
    B, K = 5, 2
    c = _own_case(blob, B, 1, "mixed")
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    other, xr = _t(c["other"]), _t(c["xr"])
    idx = torch.zeros(B, 9, dtype=torch.int32, device=_dev())
    gf = torch.zeros(B, N + 1, 3, dtype=torch.float64, device=_dev())
    gz = torch.full((B, 9, N + 1, 6), -7.0, dtype=torch.float64, device=_dev())
    tw = torch.zeros(9, mlp_frag.NPARAM, dtype=torch.float32, device=_dev())
    df = torch.full((B, 9, N + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    vjp = lambda stride, i, k, g, z: e._lib.ndp_downwash_multi_vjp_device(  # noqa: E731
        e._h, p(other), stride, p(i), k, p(xr), None, p(g), p(z), None, None)
    jvp = lambda stride, i, k, T, w, d: e._lib.ndp_downwash_multi_jvp_device(  # noqa: E731
        e._h, p(other), stride, p(i), k, p(xr), None, T, None, p(w), p(d), None, None)
    for args, why in (((10, idx, 0, gf, gz), b"K must be"), ((10, idx, 9, gf, gz), b"K must be"), ((10, None, K, gf, gz), b"d_other_index"),
                      ((7, idx, K, gf, gz), b"other_stride"), ((10, idx, K, None, gz), b"d_gf"), ((10, idx, K, gf, None), b"no output")):
        assert vjp(*args) == -2 and why in e._lib.ndp_last_error(e._h), why
    for args, why in (((10, idx, 0, 1, tw, df), b"K must be"), ((10, idx, 9, 1, tw, df), b"K must be"), ((10, None, K, 1, tw, df), b"d_other_index"),
                      ((7, idx, K, 1, tw, df), b"other_stride"), ((10, idx, K, 9, tw, df), b"n_tan"), ((10, idx, K, 0, tw, df), b"n_tan"),
                      ((10, idx, K, 1, None, df), b"no tangent"), ((10, idx, K, 1, tw, None), b"d_df")):
        assert jvp(*args) == -2 and why in e._lib.ndp_last_error(e._h), why
    e.synchronize()
    torch.cuda.synchronize()
    assert (gz == -7.0).all() and (df == -7.0).all()
    e.close()
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    assert vjp(10, idx, K, gf, gz) == -6 and b"never called" in e._lib.ndp_last_error(e._h)
    assert jvp(10, idx, K, 1, tw, df) == -6 and b"never called" in e._lib.ndp_last_error(e._h)
    with pytest.raises(ValueError, match="other_index"):
        e.downwash_multi_vjp_device(other, None, xr, gf, gz=gz)
    e.close()


# ---------------------------------------------------------------- the step
def test_control_step_ndp_multi_end_to_end(ndp, blob):
    """B = 64, K = 2 on the mixed workload's x0 / xr / ur with own-row neighbours (redrawn rows, mixed gates) and one instance whose state
    is NaN.  (i) (u0, X, U) bit-equal to the engine's external-force step fed downwash_multi_device's force; (ii) the gradients of
    weights, other and xr bit-equal to the composition by hand: step VJP, the new call, scatter; (iii) the same gradients within the 1e-5
    bars of the float64 reference chained behind the device's own gf; (iv) the failed instance has NaN in its own gradients and adds
    nothing to g_w; (v) control_step_ndp_multi_jvp agrees with the backward by duality (tests/test_downwash_jvp_gpu.py's bar: the gap
    against max(1e-5, 2.5 x the gap of a float32 restatement of the network part))."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_ndp_multi, control_step_ndp_multi_jvp
    from tests.test_downwash_jvp_gpu import gap32
    B, K, T = 64, 2, 2
    b = synth.make_batch(B, seed=synth.SEED0 + 80, downwash=True, **MIXED)
    c = M.own_row_case(77, blob, B, K, N, "mixed", xr=b["xr"])
    op = c["open"]
    bad_i = int(np.flatnonzero(op.all(axis=1))[0]) if op.all(axis=1).any() else int(np.flatnonzero(op.any(axis=1))[1])
    x0 = np.array(b["x0"])
    x0[bad_i, 3] = np.nan
    rng = np.random.default_rng(9)
    up = [rng.normal(size=(B,) + s) for s in ((4,), (N + 1, 10), (N, 4))]
    up_t = [_t(g) for g in up]
    other, idx, xr, exy = _args(c)
    ur = _t(b["ur"])

    def engine():
        e = ndp.BatchedNMPC(B, N=N, disturbance=True)
        e.reset(b["xr"], b["ur"])
        f = torch.empty(B, N + 1, 3, dtype=torch.float32, device=_dev())
        warm = torch.empty(B, 4, dtype=torch.float64, device=_dev())
        e.downwash_multi_device(other, idx, xr, f, ego_xy=exy)
        e.update_device(_t(x0), xr, ur, warm, f=f)
        e.synchronize()
        return e

    # the layer
    e = engine()
    leaf = [_t(x0).requires_grad_(True), xr.clone().requires_grad_(True), ur.clone().requires_grad_(True), other.clone().requires_grad_(True)]
    w = _t(blob).requires_grad_(True)
    out = control_step_ndp_multi(e, leaf[0], leaf[1], leaf[2], leaf[3], idx, ego_xy=exy, weights=w)
    gx0, gxr, gur, go, gw = (g.cpu().numpy() for g in torch.autograd.grad(out, leaf + [w], up_t))
    torch.cuda.synchronize()
    st = e.status()[0]
    e.close()
    # (i), (ii) by hand on a twin engine
    e2 = engine()
    f2 = torch.empty(B, N + 1, 3, dtype=torch.float32, device=_dev())
    u2 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    tape = e2.record_tape()
    e2.downwash_multi_device(other, idx, xr, f2, ego_xy=exy)
    e2.update_device(_t(x0), xr, ur, u2, f=f2)
    e2.synchronize()
    X2, U2 = (v.clone() for v in e2.device_iterate())
    hx0, hxr, hur, hgf = (torch.empty(*s, dtype=torch.float64, device=_dev()) for s in ((B, 10), (B, N + 1, 10), (B, N, 4), (B, N + 1, 3)))
    e2.step_vjp_device(_t(x0), xr, ur, tape, gu0=up_t[0], gX=up_t[1], gU=up_t[2], f=f2, gx0=hx0, gxr=hxr, gur=hur, gf=hgf)
    hgz = torch.empty(B, K, N + 1, 6, dtype=torch.float64, device=_dev())
    hgw = torch.empty(mlp_frag.NPARAM, dtype=torch.float32, device=_dev())
    e2.downwash_multi_vjp_device(other, idx, xr, hgf, ego_xy=exy, gz=hgz, gw=hgw)
    e2.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(e2.status()[0], st)
    e2.close()
    for x, y in zip(out, (u2, X2, U2)):
        assert torch.equal(x.detach(), y) or np.array_equal(x.detach().cpu().numpy(), y.cpu().numpy(), equal_nan=True)
    g, hz = hgf.cpu().numpy(), hgz.cpu().numpy()
    want_xr = hxr.cpu().numpy()
    want_xr[:, :, :6] -= hz.sum(axis=1)
    want_o = np.zeros((B * K, N + 1, 10))
    want_o[:, :, :6] = hz.reshape(B * K, N + 1, 6)            # own rows: row i K + k is read by slot (i, k) alone
    assert np.array_equal(gw, hgw.cpu().numpy())
    assert np.array_equal(gxr, want_xr, equal_nan=True) and np.array_equal(go, want_o, equal_nan=True)
    assert np.array_equal(gx0, hx0.cpu().numpy(), equal_nan=True) and np.array_equal(gur, hur.cpu().numpy(), equal_nan=True)
    # (iv)
    ok = st == 0
    print(f"{int(ok.sum())} of {B} instances with status 0, {int(op.sum())} of {B * K} slots open")
    assert not ok[bad_i] and ok.sum() >= 40
    nanrow = ~np.isfinite(g).all(axis=2)
    assert nanrow[bad_i].all() and np.isnan(gx0[bad_i]).all() and np.isnan(gxr[bad_i]).all()
    assert np.isnan(go.reshape(B, K, N + 1, 10)[bad_i][op[bad_i]][:, :, :6]).all() and np.isfinite(gw).all()
    fin = ~nanrow.any(axis=1)
    assert np.isfinite(go.reshape(B, K, N + 1, 10)[fin]).all() and np.isfinite(gxr[fin]).all()
    # (iii) the float64 reference behind the device's own gf (non-finite rows: zero upstream, as the device treats them)
    rz, rw, margin = M.vjp64(blob, c["z"], op, np.where(nanrow[:, :, None], 0.0, g))
    assert margin.min() >= R.MARGIN
    ge = R.group_errors(gw, rw)
    rel = lambda x, y: float((np.abs(x - y).max(axis=-1) / np.maximum(1.0, np.abs(y).max(axis=-1))).max())  # noqa: E731
    err_o = rel(go.reshape(B, K, N + 1, 10)[fin][..., :6], rz[fin])
    err_xr = rel((hxr.cpu().numpy()[fin][:, :, :6] - gxr[fin][:, :, :6]), rz[fin].sum(axis=1))
    print(f"weights " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()) + f"; other {err_o:.3e}, xr share {err_xr:.3e}")
    assert max(ge.values()) <= BAR and err_o <= BAR and err_xr <= BAR
    # (v) forward mode on a third engine, duality on the status-0 instances
    e3 = engine()
    tan = [rng.normal(size=(B, T) + s) for s in ((10,), (N + 1, 10), (N, 4))] + [rng.normal(size=(B * K, T, N + 1, 10))]
    tw = (blob.astype(np.float64)[None] * 0.1 * rng.normal(size=(T, mlp_frag.NPARAM))).astype(np.float32)
    res = control_step_ndp_multi_jvp(e3, _t(x0), xr, ur, other, idx, [_t(v) for v in tan] + [_t(tw)], ego_xy=exy)
    torch.cuda.synchronize()
    assert np.array_equal(e3.status()[0], st)
    e3.close()
    for x, y in zip(res[:3], out):
        assert np.array_equal(x.cpu().numpy(), y.detach().cpu().numpy(), equal_nan=True)
    d_out = [v.cpu().numpy() for v in res[3:]]
    for x in d_out:
        assert np.isnan(x[~ok]).all() and np.isfinite(x[ok]).all()
    okr = np.repeat(ok, K)                                     # rows of `other` read by status-0 instances
    live = op & ok[:, None]
    assert live.sum() >= 5
    for t in range(T):
        lhs = sum(float((gq[ok] * x[ok][:, t]).sum()) for gq, x in zip(up, d_out))
        rhs = [float((gq[ok] * v[ok][:, t]).sum()) for gq, v in zip((gx0, gxr, gur), tan[:3])]
        rhs += [float((go[okr] * tan[3][okr][:, t]).sum()), float((gw.astype(np.float64) * tw[t]).sum())]
        gap = abs(lhs - sum(rhs)) / (abs(lhs) + sum(abs(r) for r in rhs))
        tzs = (tan[3].reshape(B, K, T, N + 1, 10)[:, :, t, :, :6] - tan[1][:, None, t, :, :6])[live].reshape(-1, 6)
        floor = gap32(blob, c["z"][live].reshape(-1, 6), rng.normal(size=(tzs.shape[0], 3)), tzs, tw[t])
        print(f"direction {t}: duality gap {gap:.3e} (float32 floor of the network part {floor:.3e}); <g, J t> = {lhs:.6e}, terms "
              + " ".join(f"{r:.4e}" for r in rhs))
        assert gap <= max(BAR, 2.5 * floor)


def test_three_sgd_steps_of_the_multi_module_on_one_stream(ndp, blob):
    """NDPControlStepMulti, 3 SGD steps on `weights` against a fixed quadratic loss on X, on one non-default stream, K = 2.  The weights'
    storage is installed again exactly when its version changed (once per forward after an optimiser step, never for a repeated forward),
    every loss is finite, and the force differs from step to step."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import NDPControlStepMulti
    B, K = 64, 2
    b = synth.make_batch(B, seed=synth.SEED0 + 91, downwash=True)
    c = M.own_row_case(78, blob, B, K, N, "mixed", xr=b["xr"])
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    e.reset(b["xr"], b["ur"])
    installs, real = [], e.set_mlp_weights_device

    def counted(w_, stream=None):
        installs.append(1)
        return real(w_, stream=stream)
    e.set_mlp_weights_device = counted
    other, idx, xr, exy = _args(c)
    x0, ur = _t(b["x0"]), _t(b["ur"])
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())
    losses, forces, counts = [], [], []
    with torch.cuda.stream(s):
        mod = NDPControlStepMulti(e)
        opt = torch.optim.SGD(mod.parameters(), lr=1e-3)
        for k in range(4):
            opt.zero_grad()
            u0, X, U = mod(x0, xr, ur, other, idx, ego_xy=exy)
            if k == 0:
                mod(x0, xr, ur, other, idx, ego_xy=exy)       # the same version again: nothing is installed
            counts.append(len(installs))
            f = torch.empty(B, N + 1, 3, dtype=torch.float32, device=_dev())
            e.downwash_multi_device(other, idx, xr, f, ego_xy=exy, stream=s)
            forces.append(f)
            if k == 3:
                break
            mask = torch.isfinite(X).all(dim=2).all(dim=1)
            loss = ((X[mask] - xr[mask]) ** 2).sum() / B
            loss.backward()
            assert torch.isfinite(mod.weights.grad).all() and mod.weights.grad.abs().max() > 0
            opt.step()
            losses.append(float(loss.detach()))
        s.synchronize()
    assert np.isfinite(losses).all() and len(losses) == 3
    assert counts == [1, 2, 3, 4]
    for a, d in zip(forces[:-1], forces[1:]):
        assert not torch.equal(a, d)
    e.close()
