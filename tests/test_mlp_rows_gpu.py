"""The network on sample rows and its fused fit on the device (run with -m gpu): ndp_mlp_rows_device bit for bit against
ndp_downwash_device, ndp_mlp_fit_rows_device against the float64 reference (tests/mlp_rows_ref.py), index lists against materialised
batches, empty and non-finite rows, loss only, repeatability and isolation, other weights, refusals, and the torch layer with a 40-step
mini-batch fit.  CPU side: tests/test_mlp_rows.py.

Engine B = 15, N = 20 (315 nodes: the windows of the forward comparison); its batch shape plays no part in the row calls.  Outputs are
filled with -7.0 and have guard entries behind them that must keep it.

Bars.  gw: the project's 1e-5 per parameter group, relative to the group's largest reference entry (mlp_vjp_ref.group_errors), against
fit64_at -- the float64 VJP with the upstream taken from the DEVICE's float32 predictions, so that the forward's own error (3.7e-6, held
elsewhere) is not charged twice.  loss: |loss / loss64 - 1| <= 1e-12 against the float64 sum over the device's own d_f: every term is an
exact fp64 square of an fp32 residual, what remains is summation error of about M 2^-53 with M <= 300.  Margin rule as in
tests/test_downwash_vjp_gpu.py: rows whose smallest float64 |pre-activation| is below 1e-4 get rw = 0, at most 8 % of them."""
import ctypes as C

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag, synth
from tests import mlp_families
from tests import mlp_rows_ref as F
from tests import mlp_train_ref as T
from tests import mlp_vjp_ref as R
from tests.deriv_gpu import MIXED, _dev, _t, ndp  # noqa: F401

pytestmark = pytest.mark.gpu

B, N = 15, 20
NP = mlp_frag.NPARAM
BAR, LOSS_BAR = 1e-5, 1e-12
GUARD = 5
# test_torch_layer_and_a_minibatch_fit: |ratio_device / ratio_reference - 1| of loss[-1] / loss[0].  The first run on the MI355X measured
# 3.9e-6; the bar is ten times that (generous on purpose: a ReLU that flips near its kink moves a trajectory discretely)
FIT_RATIO_BAR = 3.9e-5


@pytest.fixture(scope="module")
def eng(ndp):
    e = ndp.BatchedNMPC(B, N=N, disturbance=True)
    yield e
    e.close()


def _rows(seed, n):
    """n rows as the device holds them: draw_rows rounded to float32."""
    return R.draw_rows(np.random.default_rng(seed), (n,)).astype(np.float32)


def _labelled(seed, n, blob):
    """(z float32 [n,6], y float32 [n,3] = the float64 network + N(0, 0.3^2), rw float32 [n] = U(0.5, 2) with the margin rule's zeros)."""
    rng = np.random.default_rng(seed)
    z = R.draw_rows(rng, (n,)).astype(np.float32)
    _, _, margin, f = R.vjp64(blob, z, np.zeros((n, 3)))
    y = (f + rng.normal(0.0, 0.3, (n, 3))).astype(np.float32)
    rw, share = F.margin_weights(rng, margin)
    return z, y, rw, share


def _fit(eng, z, y, rw, index, scale, groups=0, M=None, want=("loss", "gw", "f", "info")):
    """One ndp_mlp_fit_rows_device call on -7.0-filled outputs with guards; returns dict of numpy arrays (guards checked)."""
    import torch
    R_ = z.shape[0]
    M = (R_ if index is None else len(index)) if M is None else M
    full = lambda n, dt: torch.full((n,), -7, dtype=dt, device=_dev())  # noqa: E731
    out = dict(loss=full(1 + GUARD, torch.float64), gw=full(NP + GUARD, torch.float32), info=full(2 + GUARD, torch.int32))
    fbuf = torch.full((M + GUARD, 3), -7.0, dtype=torch.float32, device=_dev())
    eng.mlp_fit_rows_device(_t(z), _t(y), scale, index=None if index is None else _t(np.asarray(index, dtype=np.int32)),
                            row_weight=None if rw is None else _t(rw), groups=groups, M=M,
                            loss=out["loss"][:1] if "loss" in want else None, gw=out["gw"][:NP] if "gw" in want else None,
                            f=fbuf[:M] if "f" in want else None, info=out["info"][:2] if "info" in want else None)
    eng.synchronize()
    torch.cuda.synchronize()
    res = {}
    for k, n in (("loss", 1), ("gw", NP), ("info", 2)):
        a = out[k].cpu().numpy()
        assert (a[n:] == -7).all(), k
        if k not in want:
            assert (a == -7).all(), k
        res[k] = a[:n]
    fa = fbuf.cpu().numpy()
    assert (fa[M:] == -7.0).all() and ("f" in want or (fa == -7.0).all())
    res["f"] = fa[:M]
    res["loss"] = float(res["loss"][0])
    return res


def _check_against_reference(blob, z, y, rw, index, scale, got, tag):
    """Bars of the module docstring; prints every figure before it asserts."""
    loss64 = F.loss64_at(got["f"], y, rw, index, scale)
    ref = F.fit64_at(blob, z, got["f"], y, rw, index, scale)
    ge = R.group_errors(got["gw"], ref)
    full = F.fit64(blob, z, y, rw, index, scale)[0]
    print(f"{tag}: loss {got['loss']:.9e}, |loss / loss64 - 1| {abs(got['loss'] / loss64 - 1.0):.2e}, |loss / fit64 - 1| "
          f"{abs(got['loss'] / full - 1.0):.2e}; groups " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert np.isfinite(got["gw"]).all() and np.isfinite(got["loss"])
    assert abs(got["loss"] / loss64 - 1.0) <= LOSS_BAR
    assert max(ge.values()) <= BAR, ge


# ------------------------------------------------------------------------------------------------------------------------- 1 forward
def test_rows_forward_is_downwash_device_bit_for_bit(eng):
    import torch
    n = 300
    z = _rows(1, n)
    other = np.zeros((B * (N + 1), 10))
    other[:n, :6] = z.astype(np.float64)
    f_win = torch.empty(B, N + 1, 3, dtype=torch.float32, device=_dev())
    eng.downwash_device(_t(other.reshape(B, N + 1, 10)), torch.zeros(B, N + 1, 10, dtype=torch.float64, device=_dev()), f_win)
    eng.synchronize()
    want = f_win.cpu().numpy().reshape(-1, 3)[:n]
    assert np.abs(want).max() > 1e-3
    f = torch.full((n + GUARD, 3), -7.0, dtype=torch.float32, device=_dev())
    eng.mlp_rows_device(_t(z), f[:n])
    eng.synchronize()
    got = f.cpu().numpy()
    assert (got[n:] == -7.0).all()
    assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32))
    # a permuted index with duplicates, -1 and one value >= R
    rng = np.random.default_rng(2)
    index = rng.permutation(n).astype(np.int32)[:257]
    index[[5, 100, 256]] = -1
    index[[6, 7]] = index[8]
    index[33] = n
    f = torch.full((len(index) + GUARD, 3), -7.0, dtype=torch.float32, device=_dev())
    eng.mlp_rows_device(_t(z), f[:len(index)], index=_t(index))
    eng.synchronize()
    got = f.cpu().numpy()
    src, live = F.gather(index, n)
    assert (got[len(index):] == -7.0).all()
    assert (got[:len(index)][~live].view(np.uint32) == 0).all() and int((~live).sum()) == 4
    assert np.array_equal(got[:len(index)][live].view(np.uint32), want[src[live]].view(np.uint32))
    # the torch layer's evaluation call: the same bytes, no graph
    from ndp_nmpc_qd_amd.torch_layer import downwash_rows
    ft = downwash_rows(eng, _t(z), index=_t(index))
    assert not ft.requires_grad and np.array_equal(ft.cpu().numpy().view(np.uint32), got[:len(index)].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- 2 the reference
def _fit_case(M, blob):
    """The rows of the M-row case.  M = 1: the first row of a draw whose margin is at least 1e-4.  M = 33: default_rng(0) (one row under
    the margin; three would break the 8 % cap)."""
    if M == 1:
        z, y, rw, _ = _labelled(0, 33, blob)
        k = int(np.flatnonzero(rw != 0)[0])
        return z[k:k + 1], y[k:k + 1], rw[k:k + 1], 0.0
    return _labelled(0 if M == 33 else 40 + M, M, blob)


@pytest.mark.parametrize("groups", [0, 1, 2])
@pytest.mark.parametrize("M", [1, 31, 33, 129, 300])
def test_fit_against_the_float64_reference(eng, M, groups):
    blob = _lib.load_weights()
    z, y, rw, share = _fit_case(M, blob)
    print(f"M = {M}, groups = {groups}: {share:.4f} of the rows below the margin")
    assert share <= F.MAX_DROPPED
    scale = 1.0 / (3 * M)
    got = _fit(eng, z, y, rw, None, scale, groups=groups)
    _check_against_reference(blob, z, y, rw, None, scale, got, f"M {M} groups {groups}")
    assert list(got["info"]) == [M, 0]            # every row is finite, none is an empty slot: all used (rows with rw = 0 too)
    f64 = F.fit64(blob, z, y, rw, None, scale)[3]
    assert np.abs(got["f"] - f64).max() <= BAR * max(1.0, np.abs(f64).max())


# ------------------------------------------------------------------------------------------------------------- 3 index = materialised
@pytest.mark.parametrize("groups", [0, 1, 3])
def test_an_index_list_equals_the_materialised_batch(eng, groups):
    blob = _lib.load_weights()
    n = 200
    z, y, rw, _ = _labelled(11, n, blob)
    rng = np.random.default_rng(12)
    index = rng.integers(0, n, 170).astype(np.int32)
    index[[0, 64, 65, 169]] = -1
    index[128:160] = -1                           # a whole tile of empty slots
    index[[20, 21]] = index[22]
    index[90] = n + 7
    src, live = F.gather(index, n)
    scale = 1.0 / (3 * int(live.sum()))
    a = _fit(eng, z, y, rw, index, scale, groups=groups)
    b = _fit(eng, z[src], y[src], (rw[src] * live).astype(np.float32), None, scale, groups=groups)
    assert a["loss"] == b["loss"] and np.array_equal(a["gw"].view(np.uint32), b["gw"].view(np.uint32))
    assert (a["f"][~live].view(np.uint32) == 0).all()
    assert np.array_equal(a["f"][live].view(np.uint32), b["f"][live].view(np.uint32))
    assert list(a["info"]) == [int(live.sum()), 0] and list(b["info"]) == [len(index), 0]
    _check_against_reference(blob, z, y, rw, index, scale, a, f"index, groups {groups}")


# ------------------------------------------------------------------------------------------------------------- 4 nothing in, nothing out
@pytest.mark.parametrize("how", ["empty", "weightless"])
def test_nothing_in_nothing_out(eng, how):
    z, y, rw, _ = _labelled(13, 70, _lib.load_weights())
    if how == "empty":
        got = _fit(eng, z, y, rw, np.r_[np.full(50, -1), np.full(20, 70)], 1.0)
        assert list(got["info"]) == [0, 0] and not got["f"].any()
    else:
        got = _fit(eng, z, y, np.zeros_like(rw), None, 1.0)
        assert list(got["info"]) == [70, 0] and got["f"].any()
    assert got["loss"] == 0.0 and not got["gw"].any() and np.isfinite(got["gw"]).all()


# ------------------------------------------------------------------------------------------------------------------- 5 non-finite rows
def test_non_finite_rows_are_skipped_and_counted(eng):
    blob = _lib.load_weights()
    n = 150
    z, y, rw, _ = _labelled(14, n, blob)
    zd, yd, rwd = z.copy(), y.copy(), rw.copy()
    zd[3, 2], zd[40, 5], zd[131, 0] = np.nan, np.inf, -np.inf
    yd[7, 1], yd[64, 0], yd[149, 2] = np.inf, np.nan, np.nan
    rwd[9], rwd[100] = np.nan, np.inf
    bad = np.zeros(n, dtype=bool)
    bad[[3, 40, 131, 7, 64, 149, 9, 100]] = True
    scale = 1.0 / (3 * n)
    got = _fit(eng, zd, yd, rwd, None, scale, groups=2)
    assert list(got["info"]) == [n - 8, 8]
    assert np.isfinite(got["f"][~bad]).all() and np.isnan(got["f"][[3, 40, 131]]).all()
    # the same fit with those rows' rw = 0 (and their entries finite)
    rwc = np.where(bad, np.float32(0.0), rw)
    fc = dict(got, f=np.where(bad[:, None], np.float32(0.0), got["f"]))
    _check_against_reference(blob, z, y, rwc, None, scale, fc, "non-finite rows")
    clean = _fit(eng, z, y, rwc, None, scale, groups=2)
    assert clean["loss"] == got["loss"] and np.array_equal(clean["gw"], got["gw"])


# ------------------------------------------------------------------------------------------------- 6 loss only, 7 repeatability, isolation
def test_loss_only_and_two_calls_are_bit_identical(eng):
    z, y, rw, _ = _labelled(40 + 300, 300, _lib.load_weights())
    scale = 1.0 / 900
    for groups in (0, 1, 2):
        a = _fit(eng, z, y, rw, None, scale, groups=groups)
        b = _fit(eng, z, y, rw, None, scale, groups=groups)
        assert a["loss"] == b["loss"] and np.array_equal(a["gw"].view(np.uint32), b["gw"].view(np.uint32)) and np.array_equal(a["f"], b["f"])
        lo = _fit(eng, z, y, rw, None, scale, groups=groups, want=("loss",))
        assert lo["loss"] == a["loss"]
        fo = _fit(eng, z, y, rw, None, scale, groups=groups, want=("f", "info"))
        assert np.array_equal(fo["f"], a["f"]) and list(fo["info"]) == [300, 0]


def test_the_engine_and_the_backward_workspace_are_untouched(ndp):
    import torch
    b = synth.make_batch(B, seed=synth.SEED0 + 90, downwash=True, **MIXED)
    z, y, rw, _ = _labelled(15, 300, _lib.load_weights())
    gf = _t(np.random.default_rng(5).normal(size=(B, N + 1, 3)))

    def run(with_call):
        e = ndp.BatchedNMPC(B, N=N, disturbance=True)
        try:
            e.reset(b["xr"], b["ur"])
            t = {k: _t(b[k]) for k in ("x0", "xr", "ur", "other", "ego_xy")}
            u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
            gw = torch.empty(NP, dtype=torch.float32, device=_dev())
            e.update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"])
            e.synchronize()
            state = lambda: [v.clone() for v in e.device_iterate()] + [e.device_force().clone(), torch.as_tensor(e.active_set()[1]),  # noqa: E731
                                                                         *(torch.as_tensor(a) for a in e.debug_mlp_fragments())]
            before = state()
            if with_call:
                assert np.abs(_fit(e, z, y, rw, None, 1.0 / 900)["gw"]).max() > 0
            for x, w in zip(before, state()):
                assert torch.equal(x.cpu(), w.cpu())
            e.downwash_vjp_device(t["other"], t["xr"], gf, ego_xy=t["ego_xy"], gw=gw)
            e.update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"])
            e.synchronize()
            torch.cuda.synchronize()
            return u0.cpu().numpy().copy(), gw.cpu().numpy().copy()
        finally:
            e.close()
    (u_a, g_a), (u_b, g_b) = run(True), run(False)
    assert np.array_equal(u_a, u_b) and np.array_equal(g_a.view(np.uint32), g_b.view(np.uint32)) and np.abs(g_a).max() > 0


# ------------------------------------------------------------------------------------------------------------------- 8 other weights
def test_fit_at_weights_other_than_the_shipped_blob(ndp):
    blob = mlp_families.family("pert")
    z, y, rw, share = _labelled(16, 300, blob)
    print(f"pert: {share:.4f} of the rows below the margin")
    assert share <= F.MAX_DROPPED
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    try:
        e.set_mlp_weights(blob)
        for groups in (0, 1):
            got = _fit(e, z, y, rw, None, 1.0 / 900, groups=groups)
            _check_against_reference(blob, z, y, rw, None, 1.0 / 900, got, f"pert, groups {groups}")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------- 9 refusals
def test_refusals(ndp):
    import torch
    e = ndp.BatchedNMPC(B, N=N, disturbance=True, load_mlp=False)
    try:
        n = 40
        z, y = _t(_rows(3, n)), torch.zeros(n, 3, dtype=torch.float32, device=_dev())
        idx = torch.zeros(n + 8, dtype=torch.int32, device=_dev())
        loss = torch.full((1,), -7.0, dtype=torch.float64, device=_dev())
        gw = torch.full((NP,), -7.0, dtype=torch.float32, device=_dev())
        f = torch.full((n + 8, 3), -7.0, dtype=torch.float32, device=_dev())
        info = torch.full((2,), -7, dtype=torch.int32, device=_dev())
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        lib, h = e._lib, e._h
        err = lambda: lib.ndp_last_error(h).decode()  # noqa: E731

        def fit(z_=z, y_=y, index=None, R_=n, M=n, groups=0, outs=(loss, gw, f, info), handle=h):
            return lib.ndp_mlp_fit_rows_device(handle, p(z_), p(y_), None, p(index), R_, M, 1.0, groups, *(p(o) for o in outs), None)

        def rows(z_=z, index=None, R_=n, M=n, f_=f, handle=h):
            return lib.ndp_mlp_rows_device(handle, p(z_), p(index), R_, M, p(f_), None)
        assert fit(handle=None) == -1 and rows(handle=None) == -1
        assert fit(z_=None) == -1 and fit(y_=None) == -1 and rows(z_=None) == -1
        assert fit() == -6 and "never called" in err()
        assert rows() == -6 and "never called" in err()
        e.set_mlp_weights(_lib.load_weights())
        for kw, why in ((dict(R_=0), "at least 1"), (dict(M=0), "at least 1"), (dict(M=n + 1), "may not exceed R"),
                        (dict(groups=-1), "groups"), (dict(groups=_lib.FIT_MAX_GROUPS + 1), "groups"),
                        (dict(outs=(None, None, None, info)), "no output")):
            assert fit(**kw) == -2 and why in err(), (kw, err())
        for kw, why in ((dict(R_=0), "at least 1"), (dict(M=-3), "at least 1"), (dict(M=n + 1), "may not exceed R"), (dict(f_=None), "d_f is required")):
            assert rows(**kw) == -2 and why in err(), (kw, err())
        e.synchronize()
        torch.cuda.synchronize()
        for t in (loss, gw, f, info):
            assert bool((t == -7).all())
        # with an index list M may exceed R; groups at its limit is served
        assert fit(index=idx, M=n + 8, groups=_lib.FIT_MAX_GROUPS) == 0 and rows(index=idx, M=n + 8) == 0
        e.synchronize()
        torch.cuda.synchronize()
        assert list(info.cpu().numpy()) == [n + 8, 0] and bool(torch.isfinite(gw).all()) and not bool((f == -7).any())
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------- 10 torch
def _minibatch_case():
    """300 rows labelled by the float64 network under the shipped blob, the start shipped (1 + 0.02 N(0, 1)), 40 seeded index lists of 64."""
    rng = np.random.default_rng(91)
    z = R.draw_rows(rng, (300,)).astype(np.float32)
    shipped = _lib.load_weights()
    y = R.vjp64(shipped, z, np.zeros((300, 3)))[3].astype(np.float32)
    start = (shipped.astype(np.float64) * (1.0 + 0.02 * rng.normal(size=shipped.size))).astype(np.float32)
    lists = [rng.choice(300, 64, replace=False).astype(np.int32) for _ in range(40)]
    return z, y, start, lists


def test_torch_layer_and_a_minibatch_fit(eng):
    """weights.grad after (3 loss).backward() is 3 gw of the raw call, bit for bit.  Then 40 mini-batch steps (64 of 300 rows per step,
    DownwashAdamSN with sn = 4) beside the same loop on the float64 reference (fit64 + mlp_train_ref.step64); the loss over all 300 rows
    before the first step, before the last and after it.  Measured on the MI355X: device 5.957604e-02 -> 5.017076e-03, reference
    5.957600e-02 -> 5.017093e-03, both ratios 0.084213, their relative deviation 3.9e-6; the bar FIT_RATIO_BAR is ten times that, 3.9e-5."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN, downwash_fit_rows
    z, y, start, lists = _minibatch_case()
    zt, yt = _t(z), _t(y)
    try:
        rng = np.random.default_rng(92)
        rw = rng.uniform(0.5, 2.0, 300).astype(np.float32)
        index = np.r_[lists[0], [-1, -1, 300]].astype(np.int32)
        w = torch.nn.Parameter(_t(start))
        info = torch.zeros(2, dtype=torch.int32, device=_dev())
        loss = downwash_fit_rows(eng, zt, yt, w, index=_t(index), row_weight=_t(rw), scale=1.0 / 192, groups=2, info=info)
        assert loss.dtype == torch.float64 and loss.dim() == 0
        (3.0 * loss).backward()
        torch.cuda.synchronize()
        raw = _fit(eng, z, y, rw, index, 1.0 / 192, groups=2)
        assert float(loss.detach()) == raw["loss"] and list(info.cpu().numpy()) == [64, 0]
        assert np.array_equal(w.grad.cpu().numpy().view(np.uint32), (np.float32(3.0) * raw["gw"]).view(np.uint32))
        with torch.no_grad():
            assert float(downwash_fit_rows(eng, zt, yt, w)) == _fit(eng, z, y, None, None, 1.0 / 900)["loss"]      # scale None: 1 / (3 M)
        # ---- the fit
        w = torch.nn.Parameter(_t(start))
        opt = DownwashAdamSN(w, eng, sn=4.0)
        full = lambda: float(downwash_fit_rows(eng, zt, yt, w.detach()))  # noqa: E731
        dev_full, dev_batch = [full()], []
        for k, idx in enumerate(lists):
            if k == len(lists) - 1:
                dev_full.append(full())
            opt.zero_grad()
            loss = downwash_fit_rows(eng, zt, yt, w, index=_t(idx))
            loss.backward()
            opt.step()
            dev_batch.append(loss.detach())
        dev_full.append(full())
        dev_batch = [float(x) for x in dev_batch]
        assert int(opt.state[w]["step"].item()) == 40 and int(opt.state[w]["info"][0]) == 0
    finally:
        eng.set_mlp_weights(_lib.load_weights())
    p, m, v = start.copy(), np.zeros_like(start), np.zeros_like(start)
    ref_full = [F.fit64(p, z, y, None, None, 1.0 / 900)[0]]
    for k, idx in enumerate(lists):
        if k == len(lists) - 1:
            ref_full.append(F.fit64(p, z, y, None, None, 1.0 / 900)[0])
        gw = F.fit64(p, z, y, None, idx, 1.0 / 192)[1].astype(np.float32)
        s = T.step64(p, gw, m, v, k, cap=4.0)
        p, m, v = s["p"], s["m"], s["v"]
    ref_full.append(F.fit64(p, z, y, None, None, 1.0 / 900)[0])
    r_dev, r_ref = dev_full[-1] / dev_full[0], ref_full[-1] / ref_full[0]
    dev = abs(r_dev / r_ref - 1.0)
    print(f"mini-batch fit: device loss {dev_full[0]:.6e} -> {dev_full[-1]:.6e} (ratio {r_dev:.6f}), reference {ref_full[0]:.6e} -> "
          f"{ref_full[-1]:.6e} (ratio {r_ref:.6f}); deviation of the ratios {dev:.3e}")
    assert np.isfinite(dev_full).all() and np.isfinite(dev_batch).all()
    assert dev_full[-1] < dev_full[0] and ref_full[-1] < ref_full[0]
    assert dev_full[-1] != dev_full[-2]                        # the loss after the last step is not the stale weights'
    assert dev <= FIT_RATIO_BAR
