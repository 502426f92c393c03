"""The backward pass of the downwash network on the CPU: the exports and their bindings, properties of the kernels' ISA, the float64
reference derivative (tests/mlp_vjp_ref.py) against central finite differences, the torch layer's gradient routing on a stub engine, and
the index map of the transposed weight image.  GPU side: tests/test_downwash_vjp_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_vjp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    for name, nargs in (("ndp_downwash_vjp_device", 10), ("ndp_set_mlp_weights_device", 3)):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.ndp_downwash_vjp_device.argtypes[2] is C.c_int                    # other_stride
    # a null handle is refused before anything is touched
    assert lib.ndp_downwash_vjp_device(None, None, 10, None, None, None, None, None, None, None) == -1
    assert lib.ndp_set_mlp_weights_device(None, None, None) == -1
    from ndp_nmpc_qd_amd.batched import BatchedNMPC
    assert callable(BatchedNMPC.downwash_vjp_device) and callable(BatchedNMPC.set_mlp_weights_device)


def test_vjp_kernels_isa_properties():
    """mlp_vjp_kernel and the reduction use no scratch; the backward kernel runs on the matrix instructions, has no floating-point global
    atomic (the reduction is a fixed-order sum) and asks for at most 160 KB of LDS (its dynamic size is VJ_LDS_FLOATS in the source)."""
    from ndp_nmpc_qd_amd import build, isa_inspect
    build.build()
    co = isa_inspect.CodeObject(_lib.LIB_PATH)
    k = co.kernels()
    vjp = [n for n in k if "mlp_vjp_kernel" in n]
    red = [n for n in k if "mlp_vjp_reduce_kernel" in n]
    frag = [n for n in k if "mlp_frag_kernel" in n]
    assert len(vjp) == 1 and len(red) == 1 and len(frag) == 1
    for n in vjp + red + frag:
        assert k[n]["scratch"] == 0 and k[n]["spill"] == 0, (n, k[n])
    ins = co.disassemble(vjp[0])
    assert sum(s.startswith("v_mfma_f32_32x32x") for s in ins) >= 100
    assert any(s.startswith("v_mfma_f32_32x32x2_f32") for s in ins) and any(s.startswith("v_mfma_f32_32x32x16_f16") for s in ins)
    for n in vjp + red:
        assert not [s for s in co.disassemble(n) if re.match(r"(global|flat|buffer)_atomic", s)], n
    src = open(os.path.join(ROOT, "ndp_nmpc_qd_amd", "csrc", "mlp_vjp.hip")).read()
    m = re.search(r"VJ_PITCH = (\d+), VJ_WAVE = (\d+) \* VJ_PITCH, VJ_FLAGS = 4 \* VJ_WAVE, VJ_LDS_FLOATS = VJ_FLAGS \+ (\d+)", src)
    assert m is not None, "csrc/mlp_vjp.hip: the enum line that defines VJ_LDS_FLOATS no longer has the form this test reads"
    lds = (4 * int(m.group(2)) * int(m.group(1)) + int(m.group(3))) * 4 + k[vjp[0]]["lds"]
    assert 0 < lds <= 160 * 1024, lds


def test_reference_derivative_matches_central_differences():
    """tests/mlp_vjp_ref.py against central finite differences of the float64 network (step 1e-6, 1e-6 relative) on rows that pass the
    margin rule: the gradient of the input rows, and of a sample of weights of every group."""
    blob = _lib.load_weights()
    rng = np.random.default_rng(11)
    z = R.draw_rows(rng, (96,))
    gf = rng.normal(size=(96, 3))
    _, _, margin, _ = R.vjp64(blob, z, gf)
    keep = margin >= R.MARGIN
    assert keep.sum() >= 80
    z, gf = z[keep], gf[keep]
    gz, gw, margin, f0 = R.vjp64(blob, z, gf)
    loss = lambda b, zz: float((R.vjp64(b, zz, gf)[3] * gf).sum())  # noqa: E731
    h = 1e-6
    for r in range(0, z.shape[0], 9):
        for i in range(6):
            zp, zm = z.copy(), z.copy()
            zp[r, i] += h
            zm[r, i] -= h
            fd = (loss(blob, zp) - loss(blob, zm)) / (2 * h)
            assert abs(fd - gz[r, i]) <= 1e-6 * max(1.0, np.abs(gz[r]).max()), (r, i, fd, gz[r, i])
    b64 = np.asarray(blob, dtype=np.float64)
    for name, (o, shp) in mlp_frag.offsets().items():
        n = int(np.prod(shp))
        scale = np.abs(gw[o:o + n]).max()
        for i in rng.choice(n, size=min(n, 4), replace=False):
            bp, bm = b64.copy(), b64.copy()
            bp[o + i] += h
            bm[o + i] -= h
            fd = (loss(bp, z) - loss(bm, z)) / (2 * h)
            assert abs(fd - gw[o + i]) <= 1e-6 * scale, (name, i, fd, gw[o + i])


def test_margin_rule_drops_few_rows_of_the_test_distribution():
    """The share of rows whose ReLU pattern is decided by less than 1e-4 under the shipped weights and the tests' input distribution."""
    z = R.draw_rows(np.random.default_rng(12), (21504,))
    margin = R.vjp64(_lib.load_weights(), z, np.zeros((21504, 3)))[2]
    share = float((margin < R.MARGIN).mean())
    print(f"rows below the margin: {share:.4f}")
    assert share <= R.MAX_DROPPED


def test_transposed_fragment_index_map_reproduces_the_transposes():
    """fragt_source (the numpy restatement of csrc/mlp_vjp.hip's map): record (it, st, r), lane l holds W[st*32 + f0(r) + 4 (l>>5)][it*32 +
    (l&31)] -- un-permuted, the records of each layer are W transposed, every weight exactly once."""
    src = mlp_frag.fragt_source()
    assert src.shape == (mlp_frag.FRT_TOTAL,) and len(np.unique(src)) == mlp_frag.FRT_TOTAL
    blob = np.arange(mlp_frag.NPARAM, dtype=np.float32)
    w = mlp_frag.split(blob)
    img = blob[src]
    for name, base, nst, nit in (("W3", 0, 4, 2), ("W2", 128 * 64, 2, 4)):
        rec = img[base:base + 128 * 64].reshape(nit, nst, 16, 2, 32)      # [it][st][r][half][lane & 31]
        wt = np.empty((nit * 32, nst * 32), dtype=np.float32)             # W' [in][out]
        for r in range(16):
            for half in range(2):
                out = mlp_frag.f0(r) + 4 * half
                wt[:, out::32] = rec[:, :, r, half, :].transpose(0, 2, 1).reshape(nit * 32, nst)
        assert np.array_equal(wt, w[name].T), name


# ---------------------------------------------------------------- the torch layer's gradient routing
class _StubNet:
    """An engine whose 'network' is f = z M' (z = (other - ego_ref)[..., :6], M [3,6]) and whose step is u0 = sum of f, X = xr scaled,
    U = ur: CPU tensors, the layer's routing without a device."""

    def __init__(self, B, N):
        import torch
        self.B, self.N = B, N
        self.M = torch.arange(18, dtype=torch.float64).reshape(3, 6) / 10 - 0.7
        self.installed = 0
        self._force = None

    def _rows(self, other, other_index):
        return other if other_index is None else other[other_index.clamp(min=0).long()]

    def set_mlp_weights_device(self, blob, stream=None):
        self.installed += 1

    def downwash_device(self, other, ego_ref, f_out, ego_xy=None, stream=None):
        f_out.copy_(((other - ego_ref)[:, :, :6] @ self.M.T).float())

    def downwash_vjp_device(self, other, ego_ref, gf, ego_xy=None, other_index=None, gz=None, gw=None, stream=None):
        import torch
        g = gf @ self.M
        if other_index is not None:
            g = g * (other_index >= 0).double()[:, None, None]
        if gz is not None:
            gz.copy_(g)
        if gw is not None:
            gw.copy_(torch.full((17859,), float(gf.sum())))

    def record_tape(self, stream=None):
        import torch
        return (torch.zeros(1), torch.zeros(1), torch.zeros(1, dtype=torch.int8))

    def update_device(self, x0, xr, ur, u0, f=None, other=None, ego_xy=None, stream=None, other_index=None):
        rows = self._rows(other, other_index)
        f = ((rows[:, :, :6] - xr[:, :, :6]) @ self.M.T).float()
        if other_index is not None:
            f[other_index < 0] = 0
        self._force, self._X, self._U = f, 2.0 * xr, ur.clone()
        u0.copy_(f.double().sum(dim=(1, 2))[:, None].expand(-1, 4))

    def device_iterate(self):
        return self._X, self._U

    def device_force(self):
        return self._force

    def step_vjp_device(self, x0, xr, ur, tape, gu0=None, gX=None, gU=None, f=None, gx0=None, gxr=None, gur=None, gf=None, stream=None):
        if gx0 is not None:
            gx0.zero_()
        if gxr is not None:
            gxr.copy_(2.0 * gX)
        if gur is not None:
            gur.copy_(gU)
        if gf is not None:
            gf.copy_(gu0.sum(dim=1)[:, None, None].expand(-1, self.N + 1, 3))

    def synchronize(self):
        pass


def test_downwash_routes_gradients_with_the_right_signs_and_shapes():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import downwash
    B, N = 5, 20
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng = _StubNet(B, N)
    other, ego = r(B, N + 1, 10).requires_grad_(True), r(B, N + 1, 10).requires_grad_(True)
    w = torch.zeros(17859, dtype=torch.float32, requires_grad=True)
    f = downwash(eng, other, ego, weights=w)
    assert f.shape == (B, N + 1, 3) and f.dtype == torch.float32 and eng.installed == 1
    gf = torch.randn(B, N + 1, 3, generator=g)
    go, ge, gw = torch.autograd.grad(f, (other, ego, w), gf)
    gz = gf.double() @ eng.M
    assert go.shape == other.shape and torch.equal(go[:, :, :6], gz) and not go[:, :, 6:].any()
    assert torch.equal(ge[:, :, :6], -gz) and not ge[:, :, 6:].any()
    assert gw.shape == (17859,) and gw.dtype == torch.float32
    downwash(eng, other, ego, weights=w)
    assert eng.installed == 1                                  # the same tensor, the same version: not installed again
    with torch.no_grad():
        w += 1.0
    downwash(eng, other, ego, weights=w)
    assert eng.installed == 2
    # shared neighbour rows add up; an instance without a neighbour contributes nothing; [rows, N+1, 6] windows
    rows = r(3, N + 1, 6).requires_grad_(True)
    idx = torch.tensor([2, 0, 2, -1, 0], dtype=torch.int32)
    f = downwash(eng, rows, ego, other_index=idx)
    assert not f[3].any()
    (gr,) = torch.autograd.grad(f, rows, gf)
    assert gr.shape == rows.shape
    assert torch.allclose(gr[2], gz[0] + gz[2], rtol=0, atol=1e-14) and torch.allclose(gr[0], gz[1] + gz[4], rtol=0, atol=1e-14)
    assert not gr[1].any()
    with pytest.raises(ValueError, match="ego_xy requires grad"):
        downwash(eng, other, ego, ego_xy=torch.zeros(B, 2, dtype=torch.float64, requires_grad=True))


def test_control_step_ndp_composes_the_two_backward_passes():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_ndp
    B, N = 4, 20
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng = _StubNet(B, N)
    x0 = r(B, 10).requires_grad_(True)
    xr, ur, other = r(B, N + 1, 10).requires_grad_(True), r(B, N, 4).requires_grad_(True), r(B, N + 1, 10).requires_grad_(True)
    w = torch.zeros(17859, dtype=torch.float32, requires_grad=True)
    u0, X, U = control_step_ndp(eng, x0, xr, ur, other, weights=w)
    gu0, gX, gU = r(B, 4), r(B, N + 1, 10), r(B, N, 4)
    gx0, gxr, gur, go, gw = torch.autograd.grad((u0, X, U), (x0, xr, ur, other, w), (gu0, gX, gU))
    gf = gu0.sum(dim=1)[:, None, None].expand(-1, N + 1, 3)
    gz = gf @ eng.M
    assert torch.equal(gur, gU) and not gx0.any()
    want = 2.0 * gX
    want[:, :, :6] -= gz
    assert torch.allclose(gxr, want, rtol=0, atol=1e-14)
    assert torch.allclose(go[:, :, :6], gz, rtol=0, atol=1e-14) and not go[:, :, 6:].any()
    assert torch.allclose(gw, torch.full((17859,), float(gf.sum()), dtype=torch.float32))
    with pytest.raises(ValueError, match="ego_xy requires grad"):
        control_step_ndp(eng, x0, xr, ur, other, ego_xy=torch.zeros(B, 2, dtype=torch.float64, requires_grad=True))


def test_existing_layers_still_refuse_other():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step, control_step_trajectory
    B, N = 2, 20
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    eng = _StubNet(B, N)
    eng.sensitivity_level, eng.param_sensitivity_enabled = 1, True
    for fn in (control_step, control_step_trajectory):
        with pytest.raises(ValueError, match="other requires grad"):
            fn(eng, z(B, 10), z(B, N + 1, 10), z(B, N, 4), other=z(B, N + 1, 10).requires_grad_(True))
