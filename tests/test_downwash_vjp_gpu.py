"""The backward pass of the downwash network on the device (run with -m gpu): ndp_downwash_vjp_device against the float64 reference
(tests/mlp_vjp_ref.py) under four gate / addressing forms, with and without the margin rule, determinism and isolation, the weights set
from device memory, the composition with the step's adjoint (control_step_ndp) and a training-shaped loop.  CPU side:
tests/test_downwash_vjp.py.

Bars (the project's 1e-5 for this network, relative): g_z |err| <= 1e-5 max(1, max|g_z| of the row); every parameter group
max|err| <= 1e-5 max|reference group|.  Margin rule: rows whose smallest float64 |pre-activation| is below 1e-4 get gf = 0 in the
input; at most 8 % of the rows may be dropped."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag, synth
from tests import mlp_vjp_ref as R
from tests.deriv_gpu import MIXED, _dev, _t, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

B, N = 1024, 20
BAR = 1e-5


def _case(form, seed, B=B):
    """Inputs of one form (B instances): other - xr drawn as the network's golden rows, gf ~ N(0, 1).  Returns a dict with numpy arrays: other (as
    handed to the device), xr, ego_xy or None, index or None, z [B,N+1,6] (the rows the network sees), live [B] (gate open and a
    neighbour present), gf.  Nothing here depends on the weights: tests/test_downwash_weights_gpu.py runs the same cases under other blobs."""
    rng = np.random.default_rng(seed)
    xr = rng.normal(0.0, 1.0, (B, N + 1, 10))
    gf = rng.normal(size=(B, N + 1, 3))
    stride = 6 if form == "stride6" else 10
    if form == "index":
        rows = 300
        idx = rng.integers(0, rows, B).astype(np.int32)
        idx[rng.random(B) < 0.2] = -1
        idx[:8] = 5                                           # shared rows for certain
        src = np.clip(idx, 0, None)
        other = rng.normal(0.0, 1.0, (rows, N + 1, stride))
        # rows of `other` are shared: draw z for the first user of each row, the others see whatever difference results -- so give all
        # users of a row the same xr[..., :6]
        first = {}
        for i in range(B):
            first.setdefault(int(src[i]), i)
        for i in range(B):
            xr[i, :, :6] = xr[first[int(src[i])], :, :6]
        for r, i in first.items():
            other[r, :, :6] = xr[i, :, :6] + R.draw_rows(rng, (N + 1,))
        z = other[src][:, :, :6] - xr[:, :, :6]
        live = idx >= 0
        return dict(other=other, xr=xr, ego_xy=None, index=idx, z=z, live=live, gf=gf)
    z = R.draw_rows(rng, (B, N + 1))
    other = rng.normal(0.0, 1.0, (B, N + 1, stride))
    other[:, :, :6] = xr[:, :, :6] + z
    z = other[:, :, :6] - xr[:, :, :6]
    ego_xy, live = None, np.ones(B, dtype=bool)
    if form in ("part", "closed"):
        r_h = float(_lib.default_cfg().r_horiz)
        ang = rng.uniform(0, 2 * np.pi, B)
        want = rng.random(B) < 0.36 if form == "part" else np.zeros(B, dtype=bool)
        rad = np.where(want, rng.uniform(0.0, 0.9 * r_h, B), rng.uniform(1.1 * r_h, 3.0 * r_h, B))
        ego_xy = other[:, 0, :2] + (rad * np.array([np.cos(ang), np.sin(ang)])).T
        d = other[:, 0, :2] - ego_xy
        live = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < r_h * r_h
    return dict(other=other, xr=xr, ego_xy=ego_xy, index=None, z=z, live=live, gf=gf)


def _device_vjp(eng, c, gf, want_gw=True):
    import torch
    B = c["xr"].shape[0]
    gz = torch.full((B, N + 1, 6), -7.0, dtype=torch.float64, device=_dev())
    gw = torch.full((mlp_frag.NPARAM,), -7.0, dtype=torch.float32, device=_dev()) if want_gw else None
    eng.downwash_vjp_device(_t(c["other"]), _t(c["xr"]), _t(gf), ego_xy=None if c["ego_xy"] is None else _t(c["ego_xy"]),
                            other_index=None if c["index"] is None else _t(c["index"]), gz=gz, gw=gw)
    eng.synchronize()
    torch.cuda.synchronize()
    return gz.cpu().numpy(), None if gw is None else gw.cpu().numpy()


def _reference(c, gf, blob=None):
    """float64 reference of the network with the weights `blob` (None: the shipped ones) on the live rows (dead rows: zero upstream).
    Returns (g_z, g_w, margin) with [B,N+1,...] shapes."""
    B = c["xr"].shape[0]
    g = gf * c["live"][:, None, None]
    gz, gw, margin, _ = R.vjp64(_lib.load_weights() if blob is None else blob, c["z"].reshape(-1, 6), g.reshape(-1, 3))
    return gz.reshape(B, N + 1, 6), gw, margin.reshape(B, N + 1)


@pytest.fixture(scope="module")
def eng(ndp):
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    yield e
    e.close()


@pytest.mark.parametrize("form", ["open", "part", "index", "stride6"])
def test_against_the_float64_reference_with_the_margin_rule(eng, form):
    c = _case(form, 100 + len(form))
    _, _, margin = _reference(c, c["gf"])
    drop = margin < R.MARGIN
    share = float(drop.mean())
    print(f"{form}: {share:.4f} of the rows below the margin, {int(c['live'].sum())} of {B} instances live")
    assert share <= R.MAX_DROPPED
    if form == "part":
        assert 0.25 < c["live"].mean() < 0.47
    gf = c["gf"] * ~drop[:, :, None]
    gz, gw = _device_vjp(eng, c, gf)
    rz, rw, _ = _reference(c, gf)
    err = np.abs(gz - rz).max(axis=2) / np.maximum(1.0, np.abs(rz).max(axis=2))
    ge = R.group_errors(gw, rw)
    print(f"{form}: g_z error {err.max():.3e}; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert err.max() <= BAR
    assert max(ge.values()) <= BAR, ge
    assert not gz[~c["live"]].any()                           # closed and neighbour-less instances: exactly 0


def test_every_gate_closed_gives_exact_zeros(eng):
    c = _case("closed", 77)
    assert not c["live"].any()
    gz, gw = _device_vjp(eng, c, c["gf"])
    assert not gz.any() and not gw.any()


@pytest.mark.parametrize("form", ["part", "index"])
@pytest.mark.parametrize("nb", [5, 7, 2048])
def test_partial_tiles_missing_waves_and_several_rounds(ndp, nb, form):
    """Shapes the headline batch never reaches: 5 instances = 105 rows (a last tile of 9 rows, padding rows), 7 = 147 rows (a second
    workgroup with one wave), 2048 = 336 workgroups of work on 256 (the grid-stride loop's second round: accumulators, LDS image and
    flags reused).  Same bars; the share of rows under the margin is a statistic, asserted only where there are enough rows for one."""
    c = _case(form, 300 + nb, B=nb)
    e = ndp.BatchedNMPC(nb, N=N, disturbance=True)
    _, _, margin = _reference(c, c["gf"])
    drop = margin < R.MARGIN
    if nb >= 1024:
        assert float(drop.mean()) <= R.MAX_DROPPED
    gf = c["gf"] * ~drop[:, :, None]
    gz, gw = _device_vjp(e, c, gf)
    gz2, gw2 = _device_vjp(e, c, gf)
    e.close()
    rz, rw, _ = _reference(c, gf)
    assert np.array_equal(gz, gz2) and np.array_equal(gw, gw2)
    assert not gz[~c["live"]].any()
    if not c["live"].any():
        assert not gw.any()
        return
    err = np.abs(gz - rz).max(axis=2) / np.maximum(1.0, np.abs(rz).max(axis=2))
    ge = R.group_errors(gw, rw)
    print(f"B = {nb} {form}: {int(c['live'].sum())} live, g_z error {err.max():.3e}; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert err.max() <= BAR and max(ge.values()) <= BAR, ge


@pytest.mark.parametrize("form", ["open", "part"])
def test_masks_are_the_forwards_own_without_the_margin_rule(eng, form):
    """gf nonzero on every row: rows whose g_z misses the bar must be rows the margin rule would have dropped."""
    c = _case(form, 200 + len(form))
    gz, _ = _device_vjp(eng, c, c["gf"], want_gw=False)
    rz, _, margin = _reference(c, c["gf"])
    err = np.abs(gz - rz).max(axis=2) / np.maximum(1.0, np.abs(rz).max(axis=2))
    miss = err > BAR
    print(f"{form}: {int(miss.sum())} of {miss.size} rows miss the bar without the margin rule, all of them below the margin: "
          f"{bool((margin[miss] < R.MARGIN).all())}; worst error on rows above the margin {err[margin >= R.MARGIN].max():.3e}")
    assert (margin[miss] < R.MARGIN).all()


def test_two_calls_are_bit_identical_and_the_engine_is_untouched(ndp):
    import torch
    b = synth.make_batch(B, seed=synth.SEED0 + 90, downwash=True, **MIXED)
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    e.reset(b["xr"], b["ur"])
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    step = lambda: (e.update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"]), e.synchronize())  # noqa: E731
    step()
    state = lambda: [v.clone() for v in e.device_iterate()] + [e.device_force().clone(), torch.as_tensor(e.active_set()[1]),  # noqa: E731
                                                                 *(torch.as_tensor(a) for a in e.debug_mlp_fragments())]
    before = state()
    c = dict(other=b["other"], xr=b["xr"], ego_xy=b["ego_xy"], index=None)
    gf = np.random.default_rng(5).normal(size=(B, N + 1, 3))
    a1, a2 = _device_vjp(e, c, gf), _device_vjp(e, c, gf)
    assert np.array_equal(a1[0], a2[0]) and np.array_equal(a1[1], a2[1])
    assert np.abs(a1[1]).max() > 0
    after = state()
    for x, y in zip(before, after):
        assert torch.equal(x.cpu(), y.cpu())
    step()
    with_call = u0.cpu().numpy().copy()
    e.close()
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)             # the same two steps without the call in between
    e.reset(b["xr"], b["ur"])
    step()
    step()
    assert np.array_equal(with_call, u0.cpu().numpy())
    e.close()


def test_weights_set_from_device_memory_are_the_host_paths_bytes(ndp):
    import torch
    blob = _lib.load_weights()
    c = _case("open", 31)
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    f = torch.empty(B, N + 1, 3, dtype=torch.float32, device=_dev())
    run = lambda: (e.downwash_device(_t(c["other"]), _t(c["xr"]), f), e.synchronize(), f.cpu().numpy().copy())[2]  # noqa: E731
    with pytest.raises(ndp.batched.NdpError, match="never called"):
        _device_vjp(e, c, c["gf"])
    e.set_mlp_weights(blob)
    host = e.debug_mlp_fragments()
    f_host = run()
    assert np.array_equal(host[1], blob[mlp_frag.fragt_source()])
    e.set_mlp_weights(np.zeros_like(blob))
    e.set_mlp_weights_device(_t(blob))
    e.synchronize()
    dev = e.debug_mlp_fragments()
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1].view(np.uint32), dev[1].view(np.uint32))
    assert np.array_equal(f_host, run())
    pert = blob.copy()
    pert[mlp_frag.offsets()["W4"][0]:] *= 1.5
    e.set_mlp_weights_device(_t(pert))
    e.synchronize()
    assert np.abs(run() - f_host).max() > 1e-3
    # refusals
    g = torch.zeros(B, N + 1, 3, dtype=torch.float64, device=_dev())
    with pytest.raises(ndp.batched.NdpError, match="no output"):
        e.downwash_vjp_device(_t(c["other"]), _t(c["xr"]), g)
    with pytest.raises(ndp.batched.NdpError, match="d_gf is required"):
        e.downwash_vjp_device(_t(c["other"]), _t(c["xr"]), None, gz=torch.zeros(B, N + 1, 6, dtype=torch.float64, device=_dev()))
    rc = e._lib.ndp_downwash_vjp_device(e._h, f.data_ptr(), 7, None, f.data_ptr(), None, f.data_ptr(), f.data_ptr(), None, None)
    assert rc == -2 and b"other_stride" in e._lib.ndp_last_error(e._h)
    e.close()


@pytest.mark.parametrize("form", ["dense", "index"])
def test_control_step_ndp_end_to_end(ndp, form):
    """control_step_ndp on the device, the fused step on the mixed workload, random upstream on u0, X and U.  The gf that the layer hands
    to the network's backward is caught on the way (and is bit-equal to what step_vjp_device returns for the same tape and upstream); the
    margin rule is applied to it there, before the network's backward.  Then the layer's gradients of `other` and `weights` must equal the
    float64 reference network's VJP of that gf (bars of the module docstring), and xr's gradient the adjoint's gxr minus the reference g_z
    on columns 0..5.  dense: also outputs and x0 / ur gradients bit-equal control_step_trajectory's.  index: other_index with twin
    instances that share a neighbour row (their gradients add up) and instances without a neighbour."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_ndp, control_step_trajectory
    b = synth.make_batch(B, seed=synth.SEED0 + 80, downwash=True, **MIXED)
    b = {k: np.array(v) for k, v in b.items() if k in ("x0", "xr", "ur", "other", "ego_xy")}
    idx = None
    if form == "index":
        idx = np.arange(B, dtype=np.int32)
        twin = np.arange(B) % 8 == 1
        for k in ("x0", "xr", "ur", "ego_xy"):                # instance i is a copy of i - 1 and reads its neighbour row
            b[k][twin] = b[k][np.flatnonzero(twin) - 1]
        idx[twin] -= 1
        idx[np.arange(B) % 8 == 5] = -1
    src = b["other"] if idx is None else b["other"][np.clip(idx, 0, None)]
    d = src[:, 0, :2] - b["ego_xy"]
    live = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < float(_lib.default_cfg().r_horiz) ** 2) & (True if idx is None else idx >= 0)
    c = dict(xr=b["xr"], live=live, z=src[:, :, :6] - b["xr"][:, :, :6])
    _, _, margin = _reference(c, np.zeros((B, N + 1, 3)))
    drop = margin < R.MARGIN
    print(f"{form}: {int(live.sum())} live, {float(drop.mean()):.4f} of the rows below the margin")
    assert live.sum() > 100 and float(drop[live].mean()) <= R.MAX_DROPPED
    rng = np.random.default_rng(9)
    up = (_t(rng.normal(size=(B, 4))), _t(rng.normal(size=(B, N + 1, 10))), _t(rng.normal(size=(B, N, 4))))
    w = _t(_lib.load_weights()).requires_grad_(True)
    exy, idx_t = _t(b["ego_xy"]), None if idx is None else _t(idx)

    def engine():
        e = ndp.BatchedNMPC(B, N=N, disturbance=True)
        e.reset(b["xr"], b["ur"])
        leaf = {k: _t(b[k]).requires_grad_(True) for k in ("x0", "xr", "ur", "other")}
        warm = torch.empty(B, 4, dtype=torch.float64, device=_dev())
        e.update_device(leaf["x0"].detach(), leaf["xr"].detach(), leaf["ur"].detach(), warm, other=leaf["other"].detach(), ego_xy=exy,
                        other_index=idx_t)
        e.synchronize()
        return e, leaf

    e, l = engine()
    tape = e.record_tape()                                     # the state the layer's own tape records
    caught, real, drop_t = {}, e.downwash_vjp_device, _t(drop)

    def margin_rule(other_, ego_ref_, gf_, **kw):              # between the step's adjoint and the network's backward
        caught["gf"] = gf_.clone()
        gf_[drop_t & torch.isfinite(gf_).all(dim=2)] = 0.0
        return real(other_, ego_ref_, gf_, **kw)
    e.downwash_vjp_device = margin_rule
    out = control_step_ndp(e, l["x0"], l["xr"], l["ur"], l["other"], ego_xy=exy, weights=w, other_index=idx_t)
    force = e.device_force().clone()
    st = e.status()[0]
    gx0, gxr, gur, go, gw = (g.cpu().numpy() for g in torch.autograd.grad(out, (l["x0"], l["xr"], l["ur"], l["other"], w), up))
    # the same gf, recomputed from the same tape and upstream
    gf2 = torch.empty(B, N + 1, 3, dtype=torch.float64, device=_dev())
    gxr2 = torch.empty(B, N + 1, 10, dtype=torch.float64, device=_dev())
    e.step_vjp_device(l["x0"].detach(), l["xr"].detach(), l["ur"].detach(), tape, gu0=up[0], gX=up[1], gU=up[2], f=force, gxr=gxr2, gf=gf2)
    e.synchronize()
    e.close()
    g, gxr2 = gf2.cpu().numpy(), gxr2.cpu().numpy()
    assert np.array_equal(caught["gf"].cpu().numpy(), g, equal_nan=True)
    bad = ~np.isfinite(g).all(axis=2)
    okb = ~bad.any(axis=1)
    print(f"{form}: {int((st != 0).sum())} of {B} instances failed their step, {int((~okb).sum())} with non-finite gf rows")
    rz, rw, _ = _reference(c, np.where(bad[:, :, None] | drop[:, :, None], 0.0, g))
    # weights
    ge = R.group_errors(gw, rw)
    print(f"{form}: weights " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert np.isfinite(gw).all() and max(ge.values()) <= BAR, ge
    # xr: the adjoint's own gradient minus the reference g_z on columns 0..5
    rel = lambda x, y, sc: np.abs(x - y).max(axis=2) / np.maximum(1.0, np.abs(sc).max(axis=2))  # noqa: E731
    err_xr = rel(gxr[okb][:, :, :6], gxr2[okb][:, :, :6] - rz[okb], rz[okb])
    assert err_xr.max() <= BAR and np.array_equal(gxr[okb][:, :, 6:], gxr2[okb][:, :, 6:])
    # other: g_z, summed over the instances that read the row; NaN where a failed instance reads it
    rzn = np.where(bad[:, :, None], np.nan, rz)
    want = np.zeros((b["other"].shape[0], N + 1, 6))
    if idx is None:
        want[:] = rzn
    else:
        np.add.at(want, idx[idx >= 0], rzn[idx >= 0])
    fin = np.isfinite(want).all(axis=(1, 2))
    err_o = rel(go[fin][:, :, :6], want[fin], want[fin])
    print(f"{form}: other error {err_o.max():.3e}, xr error {err_xr.max():.3e}")
    assert err_o.max() <= BAR and not go[fin][:, :, 6:].any()
    assert np.isnan(go[~fin][:, :, :6]).any(axis=(1, 2)).all()
    if idx is not None:
        shared = np.flatnonzero(twin & okb & live) - 1
        # (the twins' upstream gradients differ, so do their contributions: `want` above holds their sum, and it is neither one alone)
        assert len(shared) > 10 and np.abs(go[shared][:, :, :6] - rz[shared]).max() > 1e-3
        assert np.abs(go[shared][:, :, :6] - rz[shared + 1]).max() > 1e-3
        unread = np.setdiff1d(np.arange(B), idx[idx >= 0])
        assert not go[unread].any()
    closed = okb & ~live
    assert not (gxr[closed][:, :, :6] - gxr2[closed][:, :, :6]).any()
    if idx is None:
        assert not go[closed].any()
        e1, l1 = engine()
        o1 = control_step_trajectory(e1, l1["x0"], l1["xr"], l1["ur"], other=l1["other"].detach(), ego_xy=exy)
        g1 = torch.autograd.grad(o1, (l1["x0"], l1["ur"]), up)
        torch.cuda.synchronize()
        e1.close()
        for x, y in zip(o1, out):
            assert torch.equal(x, y)
        assert np.array_equal(g1[0].cpu().numpy(), gx0, equal_nan=True) and np.array_equal(g1[1].cpu().numpy(), gur, equal_nan=True)


def test_step_gf_through_the_network_matches_the_reference_and_nan_rows_stay_out(ndp):
    """ndp_step_vjp_device's gf handed to ndp_downwash_vjp_device as it lies (failed instances: NaN rows, plus one planted): g_w is finite
    and equals the float64 reference's VJP of the finite rows (margin rule on that gf), g_z of the NaN rows is NaN."""
    import torch
    b = synth.make_batch(B, seed=synth.SEED0 + 80, downwash=True, **MIXED)
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    e.reset(b["xr"], b["ur"])
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    e.update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"])
    tape = e.record_tape()
    e.update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"])
    e.synchronize()
    force = e.device_force().clone()
    rng = np.random.default_rng(10)
    gf = torch.empty(B, N + 1, 3, dtype=torch.float64, device=_dev())
    e.step_vjp_device(t["x0"], t["xr"], t["ur"], tape, gu0=_t(rng.normal(size=(B, 4))), gX=_t(rng.normal(size=(B, N + 1, 10))),
                      gU=_t(rng.normal(size=(B, N, 4))), f=force, gf=gf)
    e.synchronize()
    d = b["other"][:, 0, :2] - b["ego_xy"]
    live = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < float(_lib.default_cfg().r_horiz) ** 2
    plant = int(np.flatnonzero(live)[3])
    gf[plant, 4, 1] = float("nan")
    g = gf.cpu().numpy()
    bad = ~np.isfinite(g).all(axis=2)
    print(f"{int(bad.any(axis=1).sum())} instances with non-finite gf rows (one planted), {int(live.sum())} live")
    c = dict(other=b["other"], xr=b["xr"], ego_xy=b["ego_xy"], index=None, live=live, z=b["other"][:, :, :6] - b["xr"][:, :, :6])
    g0 = np.where(bad[:, :, None], 0.0, g)
    _, _, margin = _reference(c, g0)
    drop = margin < R.MARGIN
    gin = np.where(drop[:, :, None] & ~bad[:, :, None], 0.0, g)          # margin rule on the finite rows; the NaN rows stay NaN
    gz, gw = _device_vjp(e, c, gin)
    e.close()
    rz, rw, _ = _reference(c, np.where(bad[:, :, None] | drop[:, :, None], 0.0, g))
    assert np.isfinite(gw).all()
    ge = R.group_errors(gw, rw)
    fin = ~bad
    err = np.abs(gz[fin] - rz[fin]).max(axis=1) / np.maximum(1.0, np.abs(rz[fin]).max(axis=1))
    print(f"step gf: g_z error {err.max():.3e}; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert err.max() <= BAR and max(ge.values()) <= BAR
    assert np.isnan(gz[bad & live[:, None]]).all() and np.isnan(gz[plant, 4]).all()
    assert not gz[~live].any()


def test_three_sgd_steps_on_one_stream(ndp):
    """NDPControlStep, 3 SGD steps on `weights` against a fixed quadratic loss on X, all on one non-default stream.  Nothing but the
    module's own forward installs weights: the device image read behind every forward differs from the one behind the forward before it
    (a fourth forward shows the third step's), every loss is finite, and with the same inputs in every step the force differs from step to
    step -- step 2's forward ran under step 1's weights.  No claim about convergence."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import NDPControlStep
    b = synth.make_batch(B, seed=synth.SEED0 + 91, downwash=True)
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    e.reset(b["xr"], b["ur"])
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())
    losses, frags, forces = [], [], []
    shipped = e.debug_mlp_fragments()[0].copy()
    with torch.cuda.stream(s):
        mod = NDPControlStep(e)
        opt = torch.optim.SGD(mod.parameters(), lr=1e-3)
        for k in range(4):
            opt.zero_grad()
            u0, X, U = mod(t["x0"], t["xr"], t["ur"], t["other"], ego_xy=t["ego_xy"])
            forces.append(e.device_force().clone())
            s.synchronize()
            frags.append(e.debug_mlp_fragments()[0].copy())    # what THIS forward ran under
            if k == 3:
                break
            mask = torch.isfinite(X).all(dim=2).all(dim=1)
            loss = ((X[mask] - t["xr"][mask]) ** 2).sum() / B
            loss.backward()
            assert torch.isfinite(mod.weights.grad).all() and mod.weights.grad.abs().max() > 0
            opt.step()
            losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and len(losses) == 3
    assert np.array_equal(shipped, frags[0])                   # the module starts from the shipped blob
    for a, c in zip(frags[:-1], frags[1:]):
        assert not np.array_equal(a, c)
    for a, c in zip(forces[:-1], forces[1:]):
        assert not torch.equal(a, c)
    e.close()
