"""The derivatives of the downwash force on the plant, on the CPU: the float64 reference (tests/plant_force_deriv_ref.py) against central
differences of the float64 force and against itself by duality, the redraw loop of its shared-state inputs, the new exports and their
bindings, the new kernels' ISA, and the torch layer's gather / scatter on a stub engine.  GPU side: tests/test_plant_force_deriv_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_vjp_ref as R
from tests import plant_force_deriv_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = (("ndp_plant_force_vjp_device", 9), ("ndp_plant_force_multi_vjp_device", 10), ("ndp_plant_force_jvp_device", 11),
           ("ndp_plant_force_multi_jvp_device", 12))


def test_new_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    for name, nargs in SYMBOLS:
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        at = getattr(lib, name).argtypes
        assert len(at) == nargs, name
        multi = "multi" in name
        assert at[3 + multi] is C.c_int and at[4 + multi] is C.c_double          # gate, scale
        if multi:
            assert at[3] is C.c_int                                               # K
        if "jvp" in name:
            assert at[5 + multi] is C.c_int                                       # n_tan
        assert getattr(lib, name)(*[None if t is C.c_void_p else 1 for t in at]) == -1          # a null handle is refused first
    assert lib.ndp_abi_version() == 9
    from ndp_nmpc_qd_amd import torch_layer
    from ndp_nmpc_qd_amd.batched import BatchedNMPC
    for name in ("plant_force_vjp_device", "plant_force_multi_vjp_device", "plant_force_jvp_device", "plant_force_multi_jvp_device"):
        assert callable(getattr(BatchedNMPC, name)), name
    assert callable(torch_layer.plant_force) and callable(torch_layer.plant_force_jvp)


def test_new_kernels_use_no_scratch_and_run_on_the_matrix_instructions():
    from ndp_nmpc_qd_amd import build, isa_inspect
    build.build()
    co = isa_inspect.CodeObject(_lib.LIB_PATH)
    k = co.kernels()
    for want in ("plant_force_vjp_kernel", "plant_force_jvp_kernel", "plant_force_reduce_kernel"):
        names = [n for n in k if want in n]
        assert len(names) == 1, (want, names)
        m = k[names[0]]
        print(want, m)
        assert m["scratch"] == 0 and m["spill"] == 0 and m["sgpr_spill"] == 0, (want, m)
        if want != "plant_force_reduce_kernel":
            ins = co.disassemble(names[0])
            assert sum(s.startswith("v_mfma_f32_32x32x") for s in ins) >= 100, want
            assert any(s.startswith("v_mfma_f32_32x32x2_f32") for s in ins) and any(s.startswith("v_mfma_f32_32x32x16_f16") for s in ins), want
    vjp = k[[n for n in k if "plant_force_vjp_kernel" in n][0]]
    assert vjp["lds"] == 0                                     # (its LDS is dynamic: mlp_vjp_kernel's image, asked for at the launch)


@pytest.fixture(scope="module")
def case():
    blob = _lib.load_weights()
    c = F.shared_case(7, blob, 7, 3)
    _, op, _ = F.gather(c["x"], c["index"], True)
    has = c["index"] >= 0
    assert op.any() and (has & ~op).any() and (~has).any()
    # vehicles share states: some vehicle is ego of an open slot and neighbour in another vehicle's open slot
    assert np.intersect1d(np.flatnonzero(op.any(axis=1)), c["index"][op]).size > 0
    return blob, c


@pytest.mark.parametrize("gate,scale", [(True, 1.0), (False, 0.7)])
def test_reference_matches_central_differences_of_the_float64_force(case, gate, scale):
    """<gf, f> differenced (step 1e-6) in every state entry of every vehicle and in a sample of the weights of every group."""
    blob, c = case
    x, idx = c["x"], c["index"]
    B = x.shape[0]
    rng = np.random.default_rng(5)
    gf = rng.normal(size=(B, 3))
    gz, gx, gw, margin = F.vjp64(blob, x, idx, gf, gate, scale)
    _, op, _ = F.gather(x, idx, gate)
    assert margin[idx >= 0].min() >= R.MARGIN and not gz[~op].any() and not gx[:, 6:].any()
    loss = lambda b, xx: float((F.force64(b, xx, idx, gate, scale) * gf).sum())  # noqa: E731
    h = 1e-6
    for v in range(B):
        for col in range(10):
            xp, xm = x.copy(), x.copy()
            xp[v, col] += h
            xm[v, col] -= h
            fd = (loss(blob, xp) - loss(blob, xm)) / (2 * h)
            assert abs(fd - gx[v, col]) <= 1e-6 * max(1.0, np.abs(gx[v]).max()), (v, col, fd, gx[v, col])
    b64 = np.asarray(blob, dtype=np.float64)
    for name, (o, shp) in mlp_frag.offsets().items():
        cnt = int(np.prod(shp))
        top = np.abs(gw[o:o + cnt]).max()
        for i in rng.choice(cnt, size=min(cnt, 3), replace=False):
            bp, bm = b64.copy(), b64.copy()
            bp[o + i] += h
            bm[o + i] -= h
            fd = (loss(bp, x) - loss(bm, x)) / (2 * h)
            assert abs(fd - gw[o + i]) <= 1e-6 * top, (name, i, fd, gw[o + i])


def test_reference_modes_are_dual(case):
    """<gf, df> = <g_x, tx> + <g_w, tw> inside the reference (vjp64 is autograd plus the scatter, jvp64 is written out plus the gather)."""
    blob, c = case
    x, idx = c["x"], c["index"]
    rng = np.random.default_rng(6)
    gf, tx = rng.normal(size=(x.shape[0], 3)), rng.normal(size=x.shape)
    tw = np.asarray(blob, dtype=np.float64) * 0.1 * rng.normal(size=mlp_frag.NPARAM)
    for gate, scale in ((True, 1.0), (False, 0.7)):
        _, gx, gw, _ = F.vjp64(blob, x, idx, gf, gate, scale)
        df = F.jvp64(blob, x, idx, tx, tw, gate, scale)
        lhs, rhs = float((gf * df).sum()), float((gx * tx).sum() + (gw * tw).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)
        assert np.allclose(F.jvp64(blob, x, idx, tx, None, gate, scale) + F.jvp64(blob, x, idx, None, tw, gate, scale), df, rtol=0, atol=1e-12)
    # a direction of the attitude columns alone moves nothing
    tq = np.zeros_like(x)
    tq[:, 6:] = rng.normal(size=(x.shape[0], 4))
    assert not F.jvp64(blob, x, idx, tq, None).any()


def test_the_chain_reference_is_dual_and_matches_central_differences():
    blob = _lib.load_weights()
    B, K, ticks = 3, 2, 2
    c = F.shared_case(12, blob, B, K, empty=0.0)
    x0, idx = c["x"], c["index"]
    u = F.P.inputs(B, ticks, 3)[1]
    xs, fs = F.chain_forward(blob, x0, u, idx)
    assert F.chain_ok(blob, xs, idx) and np.abs(fs).max() > 0
    rng = np.random.default_rng(2)
    g = rng.normal(size=(B, 10))
    gx0, gu, gw = F.chain_vjp(blob, x0, u, idx, g)
    tx0, tu = rng.normal(size=(B, 10)), rng.normal(size=u.shape)
    tw = np.asarray(blob, dtype=np.float64) * 0.1 * rng.normal(size=mlp_frag.NPARAM)
    d = F.chain_jvp(blob, x0, u, idx, tx0, tu, tw)
    lhs, rhs = float((g * d).sum()), float((gx0 * tx0).sum() + (gu * tu).sum() + (gw * tw).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)
    h = 1e-6
    end = lambda a, b: F.chain_forward(blob, a, b, idx)[0][-1]  # noqa: E731
    fd = (end(x0 + h * tx0, u + h * tu) - end(x0 - h * tx0, u - h * tu)) / (2 * h)
    d0 = F.chain_jvp(blob, x0, u, idx, tx0, tu, np.zeros(mlp_frag.NPARAM))
    assert np.abs(fd - d0).max() <= 1e-6 * max(1.0, np.abs(d0).max())


@pytest.mark.parametrize("B,K", [(5, 1), (32, 1), (7, 3), (33, 2), (64, 3), (257, 2), (2048, 2)])
def test_redraw_loop_terminates_and_leaves_no_failing_slot(B, K):
    blob = _lib.load_weights()
    c = F.shared_case(100 + B + K, blob, B, K)
    print(f"B = {B} K = {K}: {c['redrawn']} states redrawn, {c['rounds']} rounds")
    assert c["rounds"] <= F.MAX_ROUNDS and not F.failing(blob, c["x"], c["index"]).any()
    idx = c["index"]
    assert not (idx == np.arange(B)[:, None]).any()
    if B * K >= 64:
        assert 0.05 < (idx < 0).mean() < 0.3 and len(np.unique(idx[idx >= 0])) < (idx >= 0).sum()          # empty slots; states shared


def test_redraw_loop_asserts_its_cap_where_it_cannot_terminate():
    with pytest.raises(AssertionError, match="does not terminate"):
        F.shared_case(1, _lib.load_weights(), 64, 8)


# ---------------------------------------------------------------- the torch layer on a stub engine
class _Stub:
    """An engine whose 'network' is net(z) = M z (M [3,6]) with no gate: CPU tensors, the layer's routing without a device."""

    def __init__(self, B):
        import torch
        self.B = B
        self.M = torch.arange(18, dtype=torch.float64).reshape(3, 6) / 10 - 0.7
        self.installed, self.calls = 0, []

    def set_mlp_weights_device(self, blob, stream=None):
        self.installed += 1

    def _z(self, x, idx):
        import torch
        has = (idx >= 0) & (idx < self.B)
        o = torch.where(has, idx.long(), torch.arange(self.B)[:, None])
        return x[o][..., :6] - x[:, None, :6], has

    def plant_force_multi_device(self, x, other_index, f_out, xy_out=None, gate=True, scale=1.0, stream=None):
        z, has = self._z(x, other_index)
        f_out.copy_(scale * ((z @ self.M.T) * has[:, :, None]).sum(dim=1))

    def plant_force_multi_vjp_device(self, x, other_index, gf, gz=None, gw=None, gate=True, scale=1.0, stream=None):
        import torch
        _, has = self._z(x, other_index)
        self.calls.append(("vjp", gz is not None, gw is not None))
        if gz is not None:
            gz.copy_(scale * (gf @ self.M)[:, None] * has[:, :, None])
        if gw is not None:
            gw.copy_(torch.full((17859,), float(gf.sum())))

    def plant_force_multi_jvp_device(self, x, other_index, tx=None, tw=None, n_tan=None, df=None, f_check=None, gate=True, scale=1.0,
                                     stream=None):
        import torch
        has = (other_index >= 0) & (other_index < self.B)
        o = torch.where(has, other_index.long(), torch.arange(self.B)[:, None])
        self.calls.append(("jvp", tx, tw, n_tan))
        tz = tx[o][..., :6] - tx[:, None, :, :6]               # [B,K,T,6]
        df.copy_(scale * ((tz @ self.M.T) * has[:, :, None, None]).sum(dim=1))
        if f_check is not None:
            self.plant_force_multi_device(x, other_index, f_check, scale=scale)

    def synchronize(self):
        pass


def test_plant_force_graph_shape_on_a_stub_engine():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import plant_force, plant_force_jvp
    B = 5
    g = torch.Generator().manual_seed(3)
    eng = _Stub(B)
    # vehicle 2 in its own slot, an index past the batch, the same neighbour twice, empty slots, vehicle 4 unread
    idx = torch.tensor([[1, 1, 0], [0, -1, 3], [2, -1, -1], [3 + B, 2, -1], [-1, 0, 0]], dtype=torch.int32)
    x = torch.randn(B, 10, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.zeros(17859, dtype=torch.float32, requires_grad=True)
    f = plant_force(eng, x, idx, scale=0.7, weights=w)
    assert f.shape == (B, 3) and f.dtype == torch.float64 and eng.installed == 1 and not f[2].any()
    gf = torch.randn(B, 3, generator=g, dtype=torch.float64)
    gx, gw = torch.autograd.grad(f, (x, w), gf)
    gz = 0.7 * gf @ eng.M
    want = torch.zeros(B, 10, dtype=torch.float64)
    for v in range(B):
        for k in range(3):
            o = int(idx[v, k])
            if 0 <= o < B and o != v:
                want[o, :6] += gz[v]
                want[v, :6] -= gz[v]
    assert gx.shape == (B, 10) and torch.allclose(gx, want, rtol=0, atol=1e-13) and not gx[:, 6:].any()
    assert gw.shape == (17859,) and gw.dtype == torch.float32 and eng.calls[-1] == ("vjp", True, True)
    plant_force(eng, x, idx, weights=w)
    assert eng.installed == 1                                  # the same tensor, the same version: not installed again
    # partial requires_grad: only what is needed is asked of the engine
    torch.autograd.grad(plant_force(eng, x.detach(), idx, weights=w), (w,), gf)
    assert eng.calls[-1] == ("vjp", False, True)
    torch.autograd.grad(plant_force(eng, x, idx), (x,), gf)
    assert eng.calls[-1] == ("vjp", True, False)
    # [B] is [B,1]; None is nobody: a zero force with zero gradients
    f1 = plant_force(eng, x, idx[:, 0])
    assert torch.equal(f1, plant_force(eng, x, idx[:, :1]))
    f0 = plant_force(eng, x, None, weights=w)
    assert not f0.any() and not any(t.any() for t in torch.autograd.grad(f0, (x, w), gf))
    # a vehicle that is its own neighbour alone: an exactly zero gradient
    own = torch.full((B, 2), -1, dtype=torch.int32)
    own[2, 1] = 2
    assert not torch.autograd.grad(plant_force(eng, x, own), (x,), gf)[0].any()
    # the weights replaced between forward and backward
    f = plant_force(eng, x, idx, weights=w)
    plant_force(eng, x, idx, weights=torch.zeros(17859, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="replaced"):
        torch.autograd.grad(f, (x,), gf)
    # forward mode: the states' directions go to the engine as they are (the device gathers)
    tx = torch.randn(B, 2, 10, generator=g, dtype=torch.float64)
    ff, df = plant_force_jvp(eng, x, idx, (tx, None), scale=0.7)
    assert eng.calls[-1][1].shape == (B, 2, 10) and eng.calls[-1][3] == 2 and df.shape == (B, 2, 3)
    assert torch.equal(ff, plant_force(eng, x, idx, scale=0.7).detach())
    for t in range(2):
        assert abs(float((gf * df[:, t]).sum()) - float((gx * tx[:, t]).sum())) <= 1e-12
    _, d1 = plant_force_jvp(eng, x, idx, (tx[:, 0], None), scale=0.7)
    assert d1.shape == (B, 3) and torch.equal(d1, df[:, 0])
    with pytest.raises(ValueError, match="no tangent"):
        plant_force_jvp(eng, x, idx, (None, None))
