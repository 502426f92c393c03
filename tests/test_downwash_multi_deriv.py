"""The derivatives of the K-neighbour downwash on the CPU: the exports and their bindings, properties of the two new kernels' ISA, the
float64 reference (tests/mlp_multi_deriv_ref.py) against central finite differences of the summed force and against itself by duality,
the redraw loop of the reference inputs, and the torch layer's slot scatter / gather routing on a stub engine.  GPU side:
tests/test_downwash_multi_deriv_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_multi_deriv_ref as M
from tests import mlp_vjp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    for name, nargs in (("ndp_downwash_multi_vjp_device", 11), ("ndp_downwash_multi_jvp_device", 13)):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
        assert getattr(lib, name).argtypes[2] is C.c_int and getattr(lib, name).argtypes[4] is C.c_int      # other_stride, K
    assert lib.ndp_downwash_multi_jvp_device.argtypes[7] is C.c_int                                           # n_tan
    # a null handle is refused before anything is touched
    assert lib.ndp_downwash_multi_vjp_device(None, None, 10, None, 2, None, None, None, None, None, None) == -1
    assert lib.ndp_downwash_multi_jvp_device(None, None, 10, None, 2, None, None, 1, None, None, None, None, None) == -1
    assert lib.ndp_abi_version() == 9
    from ndp_nmpc_qd_amd import torch_layer
    from ndp_nmpc_qd_amd.batched import BatchedNMPC
    assert callable(BatchedNMPC.downwash_multi_vjp_device) and callable(BatchedNMPC.downwash_multi_jvp_device)
    for name in ("downwash_multi", "control_step_ndp_multi", "NDPControlStepMulti", "downwash_multi_jvp", "control_step_ndp_multi_jvp"):
        assert callable(getattr(torch_layer, name)), name


def test_multi_kernels_isa_properties():
    """mlp_vjp_multi_kernel and mlp_jvp_multi_kernel use no scratch and run on the matrix instructions; the backward kernel asks for at
    most the 160 KB of LDS mlp_vjp_kernel is held to (the same dynamic size, VJ_LDS_FLOATS in the source)."""
    from ndp_nmpc_qd_amd import build, isa_inspect
    build.build()
    co = isa_inspect.CodeObject(_lib.LIB_PATH)
    k = co.kernels()
    vjp = [n for n in k if "mlp_vjp_multi_kernel" in n]
    jvp = [n for n in k if "mlp_jvp_multi_kernel" in n]
    assert len(vjp) == 1 and len(jvp) == 1
    for n in vjp + jvp:
        assert k[n]["scratch"] == 0 and k[n]["spill"] == 0, (n, k[n])
        ins = co.disassemble(n)
        assert sum(s.startswith("v_mfma_f32_32x32x") for s in ins) >= 100, n
        assert any(s.startswith("v_mfma_f32_32x32x2_f32") for s in ins) and any(s.startswith("v_mfma_f32_32x32x16_f16") for s in ins), n
    src = open(os.path.join(ROOT, "ndp_nmpc_qd_amd", "csrc", "mlp_vjp.hip")).read()
    m = re.search(r"VJ_PITCH = (\d+), VJ_WAVE = (\d+) \* VJ_PITCH, VJ_FLAGS = 4 \* VJ_WAVE, VJ_LDS_FLOATS = VJ_FLAGS \+ (\d+)", src)
    assert m is not None, "csrc/mlp_vjp.hip: the enum line that defines VJ_LDS_FLOATS no longer has the form this test reads"
    lds = (4 * int(m.group(2)) * int(m.group(1)) + int(m.group(3))) * 4 + k[vjp[0]]["lds"]
    assert 0 < lds <= 160 * 1024, lds


@pytest.fixture(scope="module")
def case():
    blob = _lib.load_weights()
    c = M.own_row_case(21, blob, 4, 3, 5, "mixed")
    assert c["open"].any() and not c["open"].all()
    return blob, c


def test_reference_matches_central_differences_of_the_summed_force(case):
    """<gf, f> of the summed float64 force, differenced (step 1e-6) in input rows of every slot and in a sample of weights of every group:
    g_z of an open slot, exactly 0 on a closed one, and g_w as the sum over the slots."""
    blob, c = case
    z, op = c["z"], c["open"]
    rng = np.random.default_rng(5)
    gf = rng.normal(size=z.shape[:1] + z.shape[2:3] + (3,))
    gz, gw, margin = M.vjp64(blob, z, op, gf)
    assert margin.min() >= R.MARGIN
    assert not gz[~op].any() and np.abs(gz[op]).min(axis=(1, 2)).max() > 0
    loss = lambda b, zz: float((M.force64(b, zz, op) * gf).sum())  # noqa: E731
    h = 1e-6
    for i in range(z.shape[0]):
        for k in range(z.shape[1]):
            for n, col in ((0, 1), (3, 4)):
                zp, zm = z.copy(), z.copy()
                zp[i, k, n, col] += h
                zm[i, k, n, col] -= h
                fd = (loss(blob, zp) - loss(blob, zm)) / (2 * h)
                assert abs(fd - gz[i, k, n, col]) <= 1e-6 * max(1.0, np.abs(gz[i, k, n]).max()), (i, k, n, fd, gz[i, k, n, col])
    b64 = np.asarray(blob, dtype=np.float64)
    for name, (o, shp) in mlp_frag.offsets().items():
        cnt = int(np.prod(shp))
        scale = np.abs(gw[o:o + cnt]).max()
        for i in rng.choice(cnt, size=min(cnt, 3), replace=False):
            bp, bm = b64.copy(), b64.copy()
            bp[o + i] += h
            bm[o + i] -= h
            fd = (loss(bp, z) - loss(bm, z)) / (2 * h)
            assert abs(fd - gw[o + i]) <= 1e-6 * scale, (name, i, fd, gw[o + i])


def test_reference_modes_are_dual(case):
    """<gf, df> = <g_z, tz> + <g_w, tw> inside the reference (vjp64 is autograd, jvp64 is written out: a check of both and of the slot sums)."""
    blob, c = case
    z, op = c["z"], c["open"]
    rng = np.random.default_rng(6)
    gf = rng.normal(size=z.shape[:1] + z.shape[2:3] + (3,))
    tz = rng.normal(size=z.shape)
    tw = np.asarray(blob, dtype=np.float64) * 0.1 * rng.normal(size=mlp_frag.NPARAM)
    gz, gw, _ = M.vjp64(blob, z, op, gf)
    df = M.jvp64(blob, z, op, tz, tw)
    lhs, rhs = float((gf * df).sum()), float((gz * tz).sum() + (gw * tw).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)
    # the parts alone, and a closed slot's direction moves nothing
    assert np.allclose(M.jvp64(blob, z, op, tz, None) + M.jvp64(blob, z, op, None, tw), df, rtol=0, atol=1e-12)
    tz_closed = tz * ~op[:, :, None, None]
    assert not M.jvp64(blob, z, op, tz_closed, None).any()


@pytest.mark.parametrize("gates", ["open", "mixed"])
def test_redraw_loop_terminates_and_leaves_no_row_below_the_margin(gates):
    blob = _lib.load_weights()
    c = M.own_row_case(31, blob, 64, 3, 20, gates)
    margin = M.vjp64(blob, c["z"], c["open"], np.zeros((64, 21, 3)))[2]
    total = margin.size
    print(f"{gates}: {c['redrawn']} of {total} rows redrawn in {c['rounds']} rounds, smallest margin {margin.min():.3e}")
    assert c["rounds"] <= M.MAX_ROUNDS and margin.min() >= R.MARGIN
    assert 0.02 * total < c["redrawn"] < 0.08 * total          # the measured share per (row, slot) is 4.2 - 4.5 %
    if gates == "mixed":
        op = c["open"]
        assert 0.25 < op.mean() < 0.47 and (~op[:, 0] & op[:, 1:].any(axis=1)).any()
        assert c["index"].shape == (64, 3) and len(np.unique(c["index"])) == 64 * 3


# ---------------------------------------------------------------- the torch layer's slot routing
class _StubMulti:
    """An engine whose 'network' is f = sum over the slots with index >= 0 of z_k M' (z_k = (other[o_k] - ego_ref)[..., :6], M [3,6]) and
    whose step is u0 = sum of f, X = 2 xr, U = ur: CPU tensors, the layer's routing without a device."""

    def __init__(self, B, N):
        import torch
        self.B, self.N = B, N
        self.M = torch.arange(18, dtype=torch.float64).reshape(3, 6) / 10 - 0.7
        self.installed = 0
        self.calls = []

    def set_mlp_weights_device(self, blob, stream=None):
        self.installed += 1

    def _z(self, other, other_index, ego_ref):
        return other[other_index.clamp(min=0).long()][..., :6] - ego_ref[:, None, :, :6]          # [B,K,N+1,6]

    def downwash_multi_device(self, other, other_index, ego_ref, f_out, ego_xy=None, stream=None):
        has = (other_index >= 0).double()[:, :, None, None]
        f_out.copy_(((self._z(other, other_index, ego_ref) @ self.M.T) * has).sum(dim=1).float())

    def downwash_multi_vjp_device(self, other, other_index, ego_ref, gf, ego_xy=None, gz=None, gw=None, stream=None):
        import torch
        has = (other_index >= 0).double()[:, :, None, None]
        if gz is not None:
            gz.copy_((gf @ self.M)[:, None] * has)
        if gw is not None:
            gw.copy_(torch.full((17859,), float(gf.sum())))

    def downwash_multi_jvp_device(self, other, other_index, ego_ref, tz=None, tw=None, ego_xy=None, n_tan=None, df=None, f_check=None,
                                  stream=None):
        has = (other_index >= 0).double()[:, None, :, None, None]
        self.calls.append(tz)
        df.copy_(((tz @ self.M.T) * has).sum(dim=2))
        if f_check is not None:
            self.downwash_multi_device(other, other_index, ego_ref, f_check)

    def record_tape(self, stream=None):
        import torch
        return (torch.zeros(1), torch.zeros(1), torch.zeros(1, dtype=torch.int8))

    def update_device(self, x0, xr, ur, u0, f=None, other=None, ego_xy=None, stream=None, other_index=None):
        assert other is None and f is not None                # the multi layer takes the external-force step
        self._X, self._U = 2.0 * xr, ur.clone()
        u0.copy_(f.double().sum(dim=(1, 2))[:, None].expand(-1, 4))

    def device_iterate(self):
        return self._X, self._U

    def step_vjp_device(self, x0, xr, ur, tape, gu0=None, gX=None, gU=None, f=None, gx0=None, gxr=None, gur=None, gf=None, stream=None):
        if gx0 is not None:
            gx0.zero_()
        if gxr is not None:
            gxr.copy_(2.0 * gX)
        if gur is not None:
            gur.copy_(gU)
        if gf is not None:
            gf.copy_(gu0.sum(dim=1)[:, None, None].expand(-1, self.N + 1, 3))

    def step_jvp_device(self, x0, xr, ur, tape, tx0=None, txr=None, tur=None, tf=None, f=None, du0=None, dX=None, dU=None, stream=None):
        du0.copy_(tf.sum(dim=(2, 3))[:, :, None].expand(-1, -1, 4))
        dX.copy_(2.0 * txr)
        dU.copy_(tur)

    def synchronize(self):
        pass


def _slots():
    import torch
    # 5 instances, 3 slots, 4 rows of `other`: row 2 twice in instance 0, rows shared across instances, empty slots, row 1 unread
    return torch.tensor([[2, 2, 0], [0, -1, 3], [-1, -1, -1], [3, 2, -1], [-1, 0, 0]], dtype=torch.int32)


def test_downwash_multi_scatters_over_slots_and_instances():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import downwash_multi
    B, N = 5, 20
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng, idx = _StubMulti(B, N), _slots()
    rows, ego = r(4, N + 1, 6).requires_grad_(True), r(B, N + 1, 10).requires_grad_(True)
    w = torch.zeros(17859, dtype=torch.float32, requires_grad=True)
    f = downwash_multi(eng, rows, idx, ego, weights=w)
    assert f.shape == (B, N + 1, 3) and f.dtype == torch.float32 and eng.installed == 1 and not f[2].any()
    gf = torch.randn(B, N + 1, 3, generator=g)
    gr, ge, gw = torch.autograd.grad(f, (rows, ego, w), gf)
    gz = gf.double() @ eng.M                                   # per instance; every slot with a neighbour gets it
    want = torch.zeros(4, N + 1, 6, dtype=torch.float64)
    for i in range(B):
        for k in range(3):
            if idx[i, k] >= 0:
                want[idx[i, k]] += gz[i]
    assert gr.shape == rows.shape and torch.allclose(gr, want, rtol=0, atol=1e-13)
    assert not gr[1].any() and torch.allclose(gr[2], 2 * gz[0] + gz[3], rtol=0, atol=1e-13)
    cnt = (idx >= 0).sum(dim=1).double()
    assert torch.allclose(ge[:, :, :6], -gz * cnt[:, None, None], rtol=0, atol=1e-13) and not ge[:, :, 6:].any()
    assert gw.shape == (17859,) and gw.dtype == torch.float32
    downwash_multi(eng, rows, idx, ego, weights=w)
    assert eng.installed == 1                                  # the same tensor, the same version: not installed again
    with pytest.raises(ValueError, match="ego_xy requires grad"):
        downwash_multi(eng, rows, idx, ego, ego_xy=torch.zeros(B, 2, dtype=torch.float64, requires_grad=True))


def test_control_step_ndp_multi_composes_the_two_backward_passes():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import NDPControlStepMulti, control_step_ndp_multi
    B, N = 5, 20
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng, idx = _StubMulti(B, N), _slots()
    x0 = r(B, 10).requires_grad_(True)
    xr, ur, other = r(B, N + 1, 10).requires_grad_(True), r(B, N, 4).requires_grad_(True), r(4, N + 1, 10).requires_grad_(True)
    w = torch.zeros(17859, dtype=torch.float32, requires_grad=True)
    u0, X, U = control_step_ndp_multi(eng, x0, xr, ur, other, idx, weights=w)
    cnt = (idx >= 0).sum(dim=1).double()
    f = (((other[idx.clamp(min=0).long()][..., :6] - xr[:, None, :, :6]) @ eng.M.T) * (idx >= 0)[:, :, None, None]).sum(dim=1).float()
    assert torch.equal(u0[:, 0], f.double().sum(dim=(1, 2))) and torch.equal(X, 2.0 * xr)
    gu0, gX, gU = r(B, 4), r(B, N + 1, 10), r(B, N, 4)
    gx0, gxr, gur, go, gw = torch.autograd.grad((u0, X, U), (x0, xr, ur, other, w), (gu0, gX, gU))
    gf = gu0.sum(dim=1)[:, None, None].expand(-1, N + 1, 3)
    gz = gf @ eng.M
    assert torch.equal(gur, gU) and not gx0.any()
    want = 2.0 * gX
    want[:, :, :6] -= gz * cnt[:, None, None]
    assert torch.allclose(gxr, want, rtol=0, atol=1e-13)
    wo = torch.zeros(4, N + 1, 6, dtype=torch.float64)
    for i in range(B):
        for k in range(3):
            if idx[i, k] >= 0:
                wo[idx[i, k]] += gz[i]
    assert torch.allclose(go[:, :, :6], wo, rtol=0, atol=1e-13) and not go[:, :, 6:].any()
    assert torch.allclose(gw, torch.full((17859,), float(gf.sum()), dtype=torch.float32))
    with pytest.raises(ValueError, match="ego_xy requires grad"):
        control_step_ndp_multi(eng, x0, xr, ur, other, idx, ego_xy=torch.zeros(B, 2, dtype=torch.float64, requires_grad=True))
    mod = NDPControlStepMulti(eng, weights=np.zeros(17859, dtype=np.float32))
    assert isinstance(mod.weights, torch.nn.Parameter) and mod.weights.shape == (17859,)
    out = mod(x0, xr, ur, other, idx)
    assert torch.equal(out[0], u0)


def test_multi_jvp_gathers_the_direction_of_every_slots_row():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_ndp_multi_jvp, downwash_multi_jvp
    B, N, T = 5, 20, 2
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng, idx = _StubMulti(B, N), _slots()
    rows, ego = r(4, N + 1, 10), r(B, N + 1, 10)
    t_rows, t_ego = r(4, T, N + 1, 10), r(B, T, N + 1, 10)
    f, df = downwash_multi_jvp(eng, rows, idx, ego, (t_rows, t_ego, None))
    tz = eng.calls[-1]
    assert tz.shape == (B, T, 3, N + 1, 6) and tz.is_contiguous()
    for i in range(B):
        for k in range(3):
            if idx[i, k] >= 0:
                assert torch.equal(tz[i, :, k], t_rows[idx[i, k], :, :, :6] - t_ego[i, :, :, :6])
    has = (idx >= 0).double()
    want = torch.einsum("btknc,k...->btnc", (tz @ eng.M.T) * has[:, None, :, None, None], torch.ones(3, dtype=torch.float64))
    assert df.shape == (B, T, N + 1, 3) and torch.allclose(df, want, rtol=0, atol=1e-13) and f.shape == (B, N + 1, 3)
    # without the T axis; only the ego window's direction: every slot sees its negative
    f1, df1 = downwash_multi_jvp(eng, rows, idx, ego, (None, t_ego[:, 0], None))
    assert df1.shape == (B, N + 1, 3) and torch.equal(eng.calls[-1][:, 0, 1], -t_ego[:, 0, :, :6])
    x0, ur = r(B, 10), r(B, N, 4)
    out = control_step_ndp_multi_jvp(eng, x0, ego, ur, rows, idx, (r(B, T, 10), t_ego, r(B, T, N, 4), t_rows, None))
    assert torch.equal(eng.calls[-1], tz)
    assert out[3].shape == (B, T, 4) and torch.allclose(out[3][:, :, 0], want.sum(dim=(2, 3)), rtol=0, atol=1e-12)
    assert torch.equal(out[4], 2.0 * t_ego)
