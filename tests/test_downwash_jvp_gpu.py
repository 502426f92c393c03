"""Forward mode of the downwash network on the device (run with -m gpu): ndp_downwash_jvp_device against the float64 reference
(tests/mlp_jvp_ref.py) under four gate / addressing forms at small shapes, the recomputed force, T directions against T calls,
isolation, duality against ndp_downwash_vjp_device, weight families other than the shipped blob, refusals, and control_step_ndp_jvp.
CPU side: tests/test_downwash_jvp.py.

Bars: |df - ref| <= 1e-5 max(1, max|ref| of the row) (the project's bar for this network) on rows whose smallest float64
|pre-activation| is at least 1e-4 (mlp_vjp_ref.MARGIN); every row that misses the bar must lie below that margin.  Duality: the
normalised gap against max(1e-5, 2.5 x the gap of a plain numpy fp32 restatement of both modes)."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag, synth
from tests import mlp_families as F
from tests import mlp_jvp_ref as J
from tests import mlp_vjp_ref as R
from tests.deriv_gpu import MIXED, _dev, _t, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

BAR = 1e-5
GUARD = 2
# (N, B): 105 rows = a last tile of 9 rows; 147 rows = a second workgroup with one wave; 1 029 rows; N = 13: instance boundaries elsewhere
SHAPES = [(20, 5), (20, 7), (20, 49), (13, 5)]
FORMS = ["open", "part", "index", "stride6"]


def _case(form, seed, B, N):
    """tests/test_downwash_vjp_gpu._case with the horizon as a parameter (that one is written for N = 20): other - xr drawn by
    mlp_vjp_ref.draw_rows; forms open / part (gate) / index (shared rows and -1) / stride6.  Returns other, xr, ego_xy, index, z, live."""
    rng = np.random.default_rng(seed)
    xr = rng.normal(0.0, 1.0, (B, N + 1, 10))
    stride = 6 if form == "stride6" else 10
    if form == "index":
        rows = 300
        idx = rng.integers(0, rows, B).astype(np.int32)
        idx[rng.random(B) < 0.2] = -1
        idx[:2] = 5                                            # a shared row for certain
        src = np.clip(idx, 0, None)
        other = rng.normal(0.0, 1.0, (rows, N + 1, stride))
        first = {}
        for i in range(B):
            first.setdefault(int(src[i]), i)
        for i in range(B):
            xr[i, :, :6] = xr[first[int(src[i])], :, :6]
        for r, i in first.items():
            other[r, :, :6] = xr[i, :, :6] + R.draw_rows(rng, (N + 1,))
        return dict(other=other, xr=xr, ego_xy=None, index=idx, z=other[src][:, :, :6] - xr[:, :, :6], live=idx >= 0)
    z = R.draw_rows(rng, (B, N + 1))
    other = rng.normal(0.0, 1.0, (B, N + 1, stride))
    other[:, :, :6] = xr[:, :, :6] + z
    z = other[:, :, :6] - xr[:, :, :6]
    ego_xy, live = None, np.ones(B, dtype=bool)
    if form == "part":
        r_h = float(_lib.default_cfg().r_horiz)
        ang = rng.uniform(0, 2 * np.pi, B)
        want = rng.random(B) < 0.36
        rad = np.where(want, rng.uniform(0.0, 0.9 * r_h, B), rng.uniform(1.1 * r_h, 3.0 * r_h, B))
        ego_xy = other[:, 0, :2] + (rad * np.array([np.cos(ang), np.sin(ang)])).T
        d = other[:, 0, :2] - ego_xy
        live = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < r_h * r_h
    return dict(other=other, xr=xr, ego_xy=ego_xy, index=None, z=z, live=live)


def _mixed_case(form, B, N, base):
    """A case of `form` with at least one live and one dead instance where the form has dead ones (part, index): the first seed from
    `base` on that gives both."""
    for seed in range(base, base + 50):
        c = _case(form, seed, B, N)
        if form not in ("part", "index") or (c["live"].any() and not c["live"].all()):
            return c
    raise AssertionError("no seed with a live and a dead instance")


def _directions(seed, blob, B, N, T, which=None):
    """tz [B,T,N+1,6] ~ N(0, 1) and tw [T,17859] = blob x 0.1 N(0, 1); which[t] in ('z', 'w', 'zw'): the other part of direction t is 0."""
    rng = np.random.default_rng(seed)
    tz = rng.normal(size=(B, T, N + 1, 6))
    tw = (np.asarray(blob, dtype=np.float64)[None] * 0.1 * rng.normal(size=(T, mlp_frag.NPARAM))).astype(np.float32)
    for t, w in enumerate(which or ()):
        if "z" not in w:
            tz[:, t] = 0.0
        if "w" not in w:
            tw[t] = 0.0
    return tz, tw


def _device_jvp(eng, c, tz, tw, T, f_check=True):
    """downwash_jvp_device into -7.0-filled buffers with GUARD rows behind the batch; returns numpy (df [B+GUARD,T,N+1,3], f_check)."""
    import torch
    B, N = c["xr"].shape[0], eng.N
    df = torch.full((B + GUARD, T, N + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    fc = torch.full((B + GUARD, N + 1, 3), -7.0, dtype=torch.float32, device=_dev())
    eng.downwash_jvp_device(_t(c["other"]), _t(c["xr"]), tz=None if tz is None else _t(tz), tw=None if tw is None else _t(tw),
                            ego_xy=None if c["ego_xy"] is None else _t(c["ego_xy"]), other_index=None if c["index"] is None else _t(c["index"]),
                            n_tan=T, df=df[:B], f_check=fc[:B] if f_check else None)
    eng.synchronize()
    torch.cuda.synchronize()
    return df.cpu().numpy(), fc.cpu().numpy()


def _reference(blob, c, tz, tw):
    """(df [B,T,N+1,3], margin [B,N+1]) of the float64 network on every row (dead instances compare against exact zeros instead)."""
    B, T, np1 = tz.shape[0], tz.shape[1], tz.shape[2]
    out = np.empty((B, T, np1, 3))
    for t in range(T):
        d, margin, _ = J.jvp64(blob, c["z"].reshape(-1, 6), tz[:, t].reshape(-1, 6), tw[t])
        out[:, t] = d.reshape(B, np1, 3)
    return out, margin.reshape(B, np1)


def _check_against_reference(tag, df, ref, drop, live, assert_share):
    """The module's bar on the live rows at or above the margin; dead rows exactly 0; rows that miss the bar lie below the margin."""
    B = ref.shape[0]
    assert (df[B:] == -7.0).all()                              # nothing written behind row B (N+1)
    df = df[:B]
    assert not df[~live].any()
    err = np.abs(df - ref).max(axis=3) / np.maximum(1.0, np.abs(ref).max(axis=3))          # [B,T,N+1]
    err = err[live]
    keep = ~drop[live]
    share = float(drop.mean())
    worst = err.transpose(0, 2, 1)[keep].max()
    miss = (err > BAR).any(axis=1)
    print(f"{tag}: {int(live.sum())} of {B} live, {share:.4f} of the rows below the margin, worst error above it {worst:.3e} per direction "
          + " ".join(f"{v:.2e}" for v in err.transpose(0, 2, 1)[keep].max(axis=0)) + f", {int(miss.sum())} rows miss the bar")
    if assert_share:
        assert share <= R.MAX_DROPPED
    assert worst <= BAR
    assert not (miss & keep).any()                             # every row that misses the bar lies below the margin


@pytest.fixture(scope="module")
def engines(ndp):
    made = {}

    def get(N, B):
        if (N, B) not in made:
            made[N, B] = ndp.BatchedNMPC(B, N=N, disturbance=True)
        return made[N, B]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N,B", SHAPES)
def test_three_directions_against_the_float64_reference(engines, N, B, form):
    """T = 3: a direction of the rows alone, one of the weights alone, one of both."""
    blob = _lib.load_weights()
    c = _mixed_case(form, B, N, 1000 + 10 * B + N)
    if form in ("part", "index"):
        assert c["live"].any() and not c["live"].all()
    tz, tw = _directions(50 + B + N, blob, B, N, 3, ("z", "w", "zw"))
    ref, margin = _reference(blob, c, tz, tw)
    df, _ = _device_jvp(engines(N, B), c, tz, tw, 3)
    assert np.abs(ref[c["live"]]).max(axis=(0, 2, 3)).min() > 1e-2                # every direction moves the force
    _check_against_reference(f"N={N} B={B} {form}", df, ref, margin < R.MARGIN, c["live"], assert_share=B == 49)


@pytest.mark.parametrize("form", FORMS)
def test_f_check_is_the_forward_kernels_force(engines, form):
    """d_f_check is bit-equal to downwash_device on the same inputs (dense windows gathered for it), 0 on dead instances."""
    import torch
    N, B = 20, 49
    c = _mixed_case(form, B, N, 2000)
    tz, _ = _directions(3, _lib.load_weights(), B, N, 1)
    e = engines(N, B)
    _, fc = _device_jvp(e, c, tz, None, 1)
    dense = np.zeros((B, N + 1, 10))
    src = c["other"] if c["index"] is None else c["other"][np.clip(c["index"], 0, None)]
    dense[:, :, :src.shape[2]] = src
    f = torch.full((B, N + 1, 3), -7.0, dtype=torch.float32, device=_dev())
    e.downwash_device(_t(dense), _t(c["xr"]), f, ego_xy=None if c["ego_xy"] is None else _t(c["ego_xy"]))
    e.synchronize()
    f = f.cpu().numpy()
    f[~c["live"]] = 0.0                                        # (no neighbour: the stand-alone forward knows no other_index)
    assert np.abs(f[c["live"]]).max() > 1e-3
    assert np.array_equal(fc[:B].view(np.uint32), f.view(np.uint32)) and (fc[B:] == -7.0).all()


@pytest.fixture(scope="module")
def stepped(ndp):
    """B = 49, N = 20: an engine that has run one fused step on the mixed workload, and that step's inputs."""
    import torch
    B, N = 49, 20
    b = synth.make_batch(B, seed=synth.SEED0 + 90, downwash=True, **MIXED)
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    e.reset(b["xr"], b["ur"])
    t = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
    e.update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"])
    e.synchronize()
    yield e, b
    e.close()


def test_f_check_after_a_fused_step_is_the_steps_force(stepped):
    e, b = stepped
    B, N = 49, 20
    c = dict(other=b["other"], xr=b["xr"], ego_xy=b["ego_xy"], index=None)
    tz, _ = _directions(4, _lib.load_weights(), B, N, 1)
    _, fc = _device_jvp(e, c, tz, None, 1)
    force = e.device_force().cpu().numpy()
    assert np.abs(force).max() > 1e-3 and not force.all()      # open and closed instances
    assert np.array_equal(fc[:B].view(np.uint32), force.view(np.uint32))


def test_eight_directions_equal_eight_calls_and_the_engine_is_untouched(stepped):
    """T = 8 in one call against eight calls of one direction, bit for bit; two identical calls; guard rows; iterate, force buffer, kept
    sets and both weight images untouched."""
    import torch
    e, b = stepped
    B, N, T = 49, 20, 8
    blob = _lib.load_weights()
    state = lambda: [v.clone() for v in e.device_iterate()] + [e.device_force().clone(), torch.as_tensor(e.active_set()[1]),  # noqa: E731
                                                                 *(torch.as_tensor(a) for a in e.debug_mlp_fragments())]
    before = state()
    c = _mixed_case("part", B, N, 3000)
    tz, tw = _directions(5, blob, B, N, T, ("z", "w", "zw", "zw", "zw", "z", "w", "zw"))
    a1, a2 = _device_jvp(e, c, tz, tw, T), _device_jvp(e, c, tz, tw, T)
    assert np.array_equal(a1[0], a2[0]) and np.array_equal(a1[1], a2[1])
    assert (a1[0][B:] == -7.0).all() and (a1[1][B:] == -7.0).all()
    assert np.abs(a1[0][:B][c["live"]]).max(axis=(0, 2, 3)).min() > 1e-2
    for t in range(T):
        one = _device_jvp(e, c, np.ascontiguousarray(tz[:, t:t + 1]), np.ascontiguousarray(tw[t:t + 1]), 1)
        assert np.array_equal(one[0][:B, 0], a1[0][:B, t]), t
        assert np.array_equal(one[1], a1[1])
    # the rows' direction alone, with no weights' direction given at all: what the same direction gives beside zeros of the other kind
    zo = _device_jvp(e, c, np.ascontiguousarray(tz[:, 0:1]), None, 1)
    assert np.array_equal(zo[0][:B, 0], a1[0][:B, 0])
    for x, y in zip(before, state()):
        assert torch.equal(x.cpu(), y.cpu())


# ---------------------------------------------------------------- duality against the backward pass
def _net32(blob, z):
    p = {k: np.asarray(v, dtype=np.float32) for k, v in mlp_frag.split(np.asarray(blob, dtype=np.float32)).items()}
    a = [np.asarray(z, dtype=np.float32)]
    for l in (1, 2, 3):
        a.append(np.maximum(a[-1] @ p[f"W{l}"].T + p[f"b{l}"], np.float32(0.0)))
    return p, a


def gap32(blob, z, gf, tz, tw):
    """The duality gap of a plain numpy float32 restatement of both modes (every product and sum in float32, the masks of the float32
    forward): what fp32 arithmetic itself leaves of <gf, J t> - <J' gf, t>.  The floor the device's gap is held against."""
    f32 = np.float32
    p, a = _net32(blob, z)
    d = {k: np.asarray(v, dtype=f32) for k, v in mlp_frag.split(np.asarray(tw, dtype=f32)).items()}
    dh = np.asarray(tz, dtype=f32)
    for l in (1, 2, 3, 4):
        dh = dh @ p[f"W{l}"].T + a[l - 1] @ d[f"W{l}"].T + d[f"b{l}"]
        if l < 4:
            dh = dh * (a[l] > 0)
    g = np.asarray(gf, dtype=f32)
    gw = {}
    for l in (4, 3, 2, 1):
        gw[f"W{l}"], gw[f"b{l}"] = g.T @ a[l - 1], g.sum(axis=0, dtype=f32)
        g = g @ p[f"W{l}"]
        if l > 1:
            g = g * (a[l - 1] > 0)
    s = lambda x, y: float((np.asarray(x, dtype=np.float64) * np.asarray(y, dtype=np.float64)).sum())  # noqa: E731
    terms = [s(gf, dh), s(g, tz), sum(s(gw[k], d[k]) for k in d)]
    return abs(terms[0] - terms[1] - terms[2]) / sum(abs(t) for t in terms)


def _device_gap(eng, c, gf, tz, tw):
    import torch
    B, N = c["xr"].shape[0], eng.N
    df, _ = _device_jvp(eng, c, tz[:, None], tw[None], 1)
    gz = torch.full((B, N + 1, 6), -7.0, dtype=torch.float64, device=_dev())
    gw = torch.full((mlp_frag.NPARAM,), -7.0, dtype=torch.float32, device=_dev())
    eng.downwash_vjp_device(_t(c["other"]), _t(c["xr"]), _t(gf), ego_xy=None if c["ego_xy"] is None else _t(c["ego_xy"]),
                            other_index=None if c["index"] is None else _t(c["index"]), gz=gz, gw=gw)
    eng.synchronize()
    torch.cuda.synchronize()
    terms = [float((gf * df[:B, 0]).sum()), float((gz.cpu().numpy() * tz).sum()), float((gw.cpu().numpy().astype(np.float64) * tw).sum())]
    return abs(terms[0] - terms[1] - terms[2]) / sum(abs(t) for t in terms), terms


@pytest.mark.parametrize("form", ["part", "index"])
def test_duality_with_the_backward_pass_on_the_device(engines, form):
    """|<gf, df> - <g_z, tz> - <g_w, tw>| over the sum of the absolute terms against ndp_downwash_vjp_device, every row (both kernels use
    the forward's own masks: no margin rule).  gf and tz are drawn as float32 values, which both kernels read exactly."""
    N, B = 20, 49
    blob = _lib.load_weights()
    c = _mixed_case(form, B, N, 4000)
    assert c["live"].any() and not c["live"].all()
    rng = np.random.default_rng(8)
    gf = rng.normal(size=(B, N + 1, 3)).astype(np.float32).astype(np.float64)
    tz, tw = _directions(9, blob, B, N, 1)
    tz, tw = tz[:, 0].astype(np.float32).astype(np.float64), tw[0]
    live = c["live"]
    floor = gap32(blob, c["z"][live].reshape(-1, 6), gf[live].reshape(-1, 3), tz[live].reshape(-1, 6), tw)
    gap, terms = _device_gap(engines(N, B), c, gf, tz, tw)
    print(f"{form}: duality gap on the device {gap:.3e}, float32 floor {floor:.3e}, bar {max(BAR, 2.5 * floor):.3e}; terms "
          + " ".join(f"{t:.4e}" for t in terms))
    assert min(abs(t) for t in terms) > 1e-3
    assert gap <= max(BAR, 2.5 * floor)


# ---------------------------------------------------------------- other weights
@pytest.mark.parametrize("name", ["tiny2", "big2", "pert"])
def test_weight_families(ndp, name):
    """B = 49, T = 2 (the rows' direction alone, then both) under weights other than the shipped blob; the rescaled families put fp16
    subnormals into the pair image the tangent's W2 and W3 are rebuilt from.  Same bar; the margin rule as mlp_families.drop_rows states
    it for the family."""
    N, B = 20, 49
    blob = F.family(name)
    c = _mixed_case("part", B, N, 5000)
    tz, tw = _directions(60, blob, B, N, 2, ("z", "zw"))
    ref, _ = _reference(blob, c, tz, tw)
    drop = F.drop_rows(name, blob, c["z"])
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    e.set_mlp_weights(blob)
    df, _ = _device_jvp(e, c, tz, tw, 2)
    e.close()
    _check_against_reference(f"{name}", df, ref, drop, c["live"], assert_share=True)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(ndp):
    import torch
    N, B = 20, 5
    c = _case("open", 1, B, N)
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    other, xr = _t(c["other"]), _t(c["xr"])
    tz = torch.zeros(B, 9, N + 1, 6, dtype=torch.float64, device=_dev())
    tw = torch.zeros(9, mlp_frag.NPARAM, dtype=torch.float32, device=_dev())
    df = torch.full((B, 9, N + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    call = lambda stride, T, z, w, d: e._lib.ndp_downwash_jvp_device(  # noqa: E731
        e._h, other.data_ptr(), stride, None, xr.data_ptr(), None, T, *(None if x is None else x.data_ptr() for x in (z, w, d)), None, None)
    for args, why in (((10, 0, tz, tw, df), b"n_tan"), ((10, 9, tz, tw, df), b"n_tan"), ((10, 1, None, None, df), b"no tangent"),
                      ((10, 1, tz, tw, None), b"d_df"), ((7, 1, tz, tw, df), b"other_stride")):
        assert call(*args) == -2 and why in e._lib.ndp_last_error(e._h), why
    e.synchronize()
    torch.cuda.synchronize()
    assert (df == -7.0).all()
    e.close()
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    assert e._lib.ndp_downwash_jvp_device(e._h, other.data_ptr(), 10, None, xr.data_ptr(), None, 1, tz.data_ptr(), None, df.data_ptr(),
                                          None, None) == -6
    assert b"never called" in e._lib.ndp_last_error(e._h)
    with pytest.raises(ValueError, match="without the T axis"):
        e.downwash_jvp_device(other, xr, tz=tz[:, 0], n_tan=8, df=df[:, 0])
    e.close()
    torch.cuda.synchronize()
    assert (df == -7.0).all()


# ---------------------------------------------------------------- the step
@pytest.mark.parametrize("N", [20, 13])
def test_control_step_ndp_jvp(ndp, N):
    """control_step_ndp_jvp on the mixed workload, B = 64, T = 2: (i) u0, X, U bit-equal to control_step_ndp's on a twin engine; (ii) du0,
    dX, dU bit-equal to downwash_jvp_device then step_jvp_device by hand on the same tape; (iii) duality against control_step_ndp's
    backward on the status-0 instances, held to the network's duality bar (the step's own gap is about 1e-13); (iv) instances whose step
    failed have NaN tangents and stay out of (iii)."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_ndp, control_step_ndp_jvp
    B, T = 64, 2
    blob = _lib.load_weights()
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 80, downwash=True, **MIXED)
    rng = np.random.default_rng(12)
    tan = [rng.normal(size=(B, T) + s) for s in ((10,), (N + 1, 10), (N, 4), (N + 1, 10))]
    tw = (blob.astype(np.float64)[None] * 0.1 * rng.normal(size=(T, mlp_frag.NPARAM))).astype(np.float32)
    up = [rng.normal(size=(B,) + s) for s in ((4,), (N + 1, 10), (N, 4))]
    exy = _t(b["ego_xy"])

    def engine():
        e = ndp.BatchedNMPC(B, N=N, disturbance=True)
        e.reset(b["xr"], b["ur"])
        leaf = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other")}
        warm = torch.empty(B, 4, dtype=torch.float64, device=_dev())
        e.update_device(leaf["x0"], leaf["xr"], leaf["ur"], warm, other=leaf["other"], ego_xy=exy)
        e.synchronize()
        return e, leaf

    e, l = engine()
    tape = e.record_tape()                                     # the state the layer's own tape records
    tt = [_t(t) for t in tan] + [_t(tw)]
    u0, X, U, du0, dX, dU = control_step_ndp_jvp(e, l["x0"], l["xr"], l["ur"], l["other"], tt, ego_xy=exy)
    torch.cuda.synchronize()
    st = e.status()[0]
    # (ii) by hand on the same tape
    tz = (tt[3][..., :6] - tt[1][..., :6]).contiguous()
    tf = torch.full((B, T, N + 1, 3), -7.0, dtype=torch.float64, device=_dev())
    e.downwash_jvp_device(l["other"], l["xr"], tz=tz, tw=tt[4], ego_xy=exy, n_tan=T, df=tf)
    hand = [torch.full((B, T) + s, -7.0, dtype=torch.float64, device=_dev()) for s in ((4,), (N + 1, 10), (N, 4))]
    e.step_jvp_device(l["x0"], l["xr"], l["ur"], tape, tt[0], tt[1], tt[2], tf, f=e.device_force(), du0=hand[0], dX=hand[1], dU=hand[2])
    e.synchronize()
    torch.cuda.synchronize()
    e.close()
    out = [v.cpu().numpy() for v in (du0, dX, dU)]
    for x, y in zip(out, hand):
        assert np.array_equal(x, y.cpu().numpy(), equal_nan=True)
    # (i) and the backward, on a twin engine
    e2, l2 = engine()
    leaf = {k: v.requires_grad_(True) for k, v in l2.items()}
    w = _t(blob).requires_grad_(True)
    o2 = control_step_ndp(e2, leaf["x0"], leaf["xr"], leaf["ur"], leaf["other"], ego_xy=exy, weights=w)
    grads = [g.cpu().numpy() for g in torch.autograd.grad(o2, (leaf["x0"], leaf["xr"], leaf["ur"], leaf["other"], w), [_t(g) for g in up])]
    torch.cuda.synchronize()
    assert np.array_equal(e2.status()[0], st)
    e2.close()
    for x, y in zip((u0, X, U), o2):
        assert torch.equal(x, y.detach())
    # (iv)
    ok = st == 0
    print(f"N={N}: {int(ok.sum())} of {B} instances with status 0")
    assert ok.sum() >= 40
    for x in out:
        assert np.isnan(x[~ok]).all() and np.isfinite(x[ok]).all()
    # (iii)
    d = b["other"][:, 0, :2] - b["ego_xy"]
    live = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < float(_lib.default_cfg().r_horiz) ** 2) & ok
    assert live.sum() >= 5
    z = (b["other"][:, :, :6] - b["xr"][:, :, :6])[live].reshape(-1, 6)
    for t in range(T):
        lhs = sum(float((g[ok] * x[ok][:, t]).sum()) for g, x in zip(up, out))
        rhs = [float((g[ok] * v[ok][:, t]).sum()) for g, v in zip(grads[:4], tan)] + [float((grads[4].astype(np.float64) * tw[t]).sum())]
        gap = abs(lhs - sum(rhs)) / (abs(lhs) + sum(abs(r) for r in rhs))
        nz = int(live.sum()) * (N + 1)
        floor = gap32(blob, z, rng.normal(size=(nz, 3)), (tan[3][live][:, t, :, :6] - tan[1][live][:, t, :, :6]).reshape(-1, 6), tw[t])
        print(f"N={N} direction {t}: duality gap {gap:.3e} (float32 floor of the network part {floor:.3e}); <g, J t> = {lhs:.6e}, terms "
              + " ".join(f"{r:.4e}" for r in rhs))
        assert gap <= max(BAR, 2.5 * floor)
