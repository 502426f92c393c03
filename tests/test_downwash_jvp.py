"""Forward mode of the downwash network on the CPU: the export and its bindings, properties of the kernel's ISA, the float64 reference
(tests/mlp_jvp_ref.py) against central finite differences and against the reverse-mode reference by duality, and the torch layer's tangent
routing on a stub engine.  GPU side: tests/test_downwash_jvp_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_jvp_ref as J
from tests import mlp_vjp_ref as R
from tests.test_downwash_vjp import _StubNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _directions(rng, blob, rows):
    """tz ~ N(0, 1) per row, tw = blob x 0.1 N(0, 1) per parameter (the draws of the device tests)."""
    return rng.normal(size=(rows, 6)), (np.asarray(blob, dtype=np.float64) * 0.1 * rng.normal(size=mlp_frag.NPARAM)).astype(np.float32)


def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    name = "ndp_downwash_jvp_device"
    assert re.search(r"\bint " + name + r"\s*\(", hdr)
    assert name in _lib.EXPORTS and hasattr(lib, name)
    fn = getattr(lib, name)
    assert len(fn.argtypes) == 12
    assert fn.argtypes[2] is C.c_int and fn.argtypes[6] is C.c_int             # other_stride, n_tan
    assert fn(None, None, 10, None, None, None, 1, None, None, None, None, None) == -1
    m = re.search(r"#define\s+NDP_ABI_VERSION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == lib.ndp_abi_version() == 9
    from ndp_nmpc_qd_amd.batched import BatchedNMPC
    assert callable(BatchedNMPC.downwash_jvp_device)
    from ndp_nmpc_qd_amd import build
    assert "mlp_jvp.hip" in build.UNITS


def test_jvp_kernel_isa_properties():
    """One mlp_jvp_kernel, without scratch or spills (scalar ones included), on the matrix instructions -- the forward's fp16 ones and the
    exact fp32 one of the tangent --, without a global atomic and without LDS; and still exactly one mlp_vjp_kernel."""
    from ndp_nmpc_qd_amd import build, isa_inspect
    build.build()
    co = isa_inspect.CodeObject(_lib.LIB_PATH)
    k = co.kernels()
    jvp = [n for n in k if "mlp_jvp_kernel" in n]
    assert len(jvp) == 1 and len([n for n in k if "mlp_vjp_kernel" in n]) == 1
    m = k[jvp[0]]
    assert m["scratch"] == 0 and m["spill"] == 0 and m["sgpr_spill"] == 0, m
    ins = co.disassemble(jvp[0])
    assert sum(s.startswith("v_mfma_f32_32x32x") for s in ins) >= 100
    # per direction: 12 + 12 (layer 1), 128 + 128 (layer 2), 128 + 128 (layer 3) exact fp32 instructions; the forward: 12 and 96 fp16 ones
    assert sum(s.startswith("v_mfma_f32_32x32x2_f32") for s in ins) == 12 + 2 * (12 + 128 + 128)
    assert sum(s.startswith("v_mfma_f32_32x32x16_f16") for s in ins) == 96
    assert not [s for s in ins if re.match(r"(global|flat|buffer)_atomic", s)]
    assert not [s for s in ins if re.match(r"ds_(read|write|load|store)", s)]   # (the half-wave sums are ds_bpermute: no LDS memory)
    assert m["lds"] <= 160 * 1024                                               # static; the launch asks for no dynamic LDS
    src = open(os.path.join(ROOT, "ndp_nmpc_qd_amd", "csrc", "mlp_jvp.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(mlp_jvp_kernel, dim3\(\(ntiles \+ 3\) / 4\), dim3\(256\), 0,", src)


def _kept_rows(blob, rng, n):
    z = R.draw_rows(rng, (n,))
    keep = J.jvp64(blob, z)[1] >= R.MARGIN
    assert keep.sum() >= 0.8 * n
    return z[keep]


def test_reference_jvp_matches_central_differences():
    """jvp64 against central finite differences of the float64 network (step 1e-6, 1e-6 relative) on rows that pass the margin rule: in
    z along tz, along tw, and along both."""
    blob = _lib.load_weights()
    rng = np.random.default_rng(21)
    z = _kept_rows(blob, rng, 96)
    tz, tw = _directions(rng, blob, z.shape[0])
    b64, t64 = np.asarray(blob, dtype=np.float64), tw.astype(np.float64)
    f64 = lambda b, zz: R.forward64(_params(b), _tt(zz))[0].numpy()  # noqa: E731
    h = 1e-6
    for dz, dw in ((tz, None), (None, tw), (tz, tw)):
        df = J.jvp64(blob, z, dz, dw)[0]
        zp, zm = (z + h * dz, z - h * dz) if dz is not None else (z, z)
        bp, bm = (b64 + h * t64, b64 - h * t64) if dw is not None else (b64, b64)
        fd = (f64(bp, zp) - f64(bm, zm)) / (2 * h)
        err = np.abs(fd - df).max(axis=1) / np.maximum(1.0, np.abs(df).max(axis=1))
        assert np.abs(df).max() > 1e-3
        assert err.max() <= 1e-6, err.max()


def _tt(a):
    import torch
    return torch.tensor(np.asarray(a, dtype=np.float64))


def _params(b64):
    """mlp_vjp_ref.params64 for a blob that is float64 already (a perturbed one: it must not be rounded to float32 on the way)."""
    return {k: _tt(v) for k, v in mlp_frag.split(np.asarray(b64, dtype=np.float64)).items()}


def test_references_are_dual():
    """<gf, jvp64(tz, tw)> = <g_z, tz> + <g_w, tw> against vjp64 (autograd) to 1e-12 relative: every row, no margin rule (both hold the
    same float64 masks)."""
    blob = _lib.load_weights()
    rng = np.random.default_rng(22)
    z = R.draw_rows(rng, (200,))
    gf = rng.normal(size=(200, 3))
    tz, tw = _directions(rng, blob, 200)
    df = J.jvp64(blob, z, tz, tw)[0]
    gz, gw, _, _ = R.vjp64(blob, z, gf)
    terms = [(gf * df).sum(), (gz * tz).sum(), (gw * tw.astype(np.float64)).sum()]
    gap = abs(terms[0] - terms[1] - terms[2]) / sum(abs(t) for t in terms)
    print(f"duality of the references: gap {gap:.2e}")
    assert gap <= 1e-12


# ---------------------------------------------------------------- the torch layer's tangent routing
class _StubJvp(_StubNet):
    """_StubNet (f = z M') with the two forward-mode calls: df = tz M' + sum(tw), and a step whose tangent is du0 = sum of tf, dX = 2 txr,
    dU = tur.  Every call's arguments are kept."""

    def __init__(self, B, N):
        super().__init__(B, N)
        self.net, self.step = [], []

    def downwash_jvp_device(self, other, ego_ref, tz=None, tw=None, ego_xy=None, other_index=None, n_tan=None, df=None, f_check=None,
                            stream=None):
        self.net.append(dict(tz=tz, tw=tw, n_tan=n_tan, df=df, other_index=other_index))
        out = 0.0 if tz is None else tz @ self.M.T
        if tw is not None:
            out = out + tw.double().sum(dim=1)[None, :, None, None]
        df.copy_(out.expand_as(df))
        if f_check is not None:
            rows = self._rows(other, other_index)
            f_check.copy_(((rows[:, :, :6] - ego_ref[:, :, :6]) @ self.M.T).float())

    def step_jvp_device(self, x0, xr, ur, tape, tx0=None, txr=None, tur=None, tf=None, f=None, du0=None, dX=None, dU=None, stream=None):
        import torch
        self.step.append(dict(tx0=tx0, txr=txr, tur=tur, tf=tf, f=f))
        du0.copy_(torch.zeros_like(du0) if tf is None else tf.sum(dim=(2, 3))[:, :, None].expand_as(du0))
        dX.copy_(2.0 * txr if txr is not None else torch.zeros_like(dX))
        dU.copy_(tur if tur is not None else torch.zeros_like(dU))


def test_downwash_jvp_routes_tangents_with_the_right_signs_columns_and_axes():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import downwash_jvp
    B, N, T = 5, 20, 3
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng = _StubJvp(B, N)
    other, ego = r(B, N + 1, 10), r(B, N + 1, 10)
    to, te = r(B, T, N + 1, 10), r(B, T, N + 1, 10)
    w = torch.zeros(17859, dtype=torch.float32)
    f, df = downwash_jvp(eng, other, ego, (to, te, None), weights=w)
    assert eng.installed == 1 and f.shape == (B, N + 1, 3) and f.dtype == torch.float32
    assert torch.equal(f, ((other - ego)[:, :, :6] @ eng.M.T).float())
    c = eng.net[-1]
    assert c["n_tan"] == T and c["tw"] is None and c["tz"].shape == (B, T, N + 1, 6) and c["tz"].is_contiguous()
    assert torch.equal(c["tz"], to[..., :6] - te[..., :6])                      # sign and columns
    assert df.shape == (B, T, N + 1, 3) and df.dtype == torch.float64 and torch.equal(df, c["tz"] @ eng.M.T)
    # one side only
    downwash_jvp(eng, other, ego, (None, te, None))
    assert torch.equal(eng.net[-1]["tz"], -te[..., :6])
    downwash_jvp(eng, other, ego, (to, None, None))
    assert torch.equal(eng.net[-1]["tz"], to[..., :6])
    # the weights' direction alone: no tz at all
    tw = torch.randn(T, 17859, generator=g)
    _, df = downwash_jvp(eng, other, ego, (None, None, tw))
    c = eng.net[-1]
    assert c["tz"] is None and c["tw"].shape == (T, 17859) and c["tw"].dtype == torch.float32 and df.shape == (B, T, N + 1, 3)
    # without the T axis: T = 1 inside, no axis outside
    _, df1 = downwash_jvp(eng, other, ego, (to[:, 0], te[:, 0], tw[0]))
    c = eng.net[-1]
    assert c["n_tan"] == 1 and c["tz"].shape == (B, 1, N + 1, 6) and c["tw"].shape == (1, 17859) and df1.shape == (B, N + 1, 3)
    assert torch.equal(df1, (to[:, 0, :, :6] - te[:, 0, :, :6]) @ eng.M.T + tw[0].double().sum())
    # other_index: every instance reads its neighbour row's direction; [rows, T, N+1, 6] windows
    rows, trows = r(3, N + 1, 6), r(3, T, N + 1, 6)
    idx = torch.tensor([2, 0, 2, -1, 0], dtype=torch.int32)
    downwash_jvp(eng, rows, ego, (trows, te, None), other_index=idx)
    c = eng.net[-1]
    assert c["other_index"] is idx
    assert torch.equal(c["tz"], trows[idx.clamp(min=0).long()] - te[..., :6])
    with pytest.raises(ValueError, match="no tangent"):
        downwash_jvp(eng, other, ego, (None, None, None))
    with pytest.raises(ValueError, match="disagree"):
        downwash_jvp(eng, other, ego, (to, te[:, :2], None))


def test_control_step_ndp_jvp_chains_the_network_into_the_step():
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_ndp_jvp
    B, N, T = 4, 20, 2
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng = _StubJvp(B, N)
    x0, xr, ur, other = r(B, 10), r(B, N + 1, 10), r(B, N, 4), r(B, N + 1, 10)
    tx0, txr, tur, to = r(B, T, 10), r(B, T, N + 1, 10), r(B, T, N, 4), r(B, T, N + 1, 10)
    tw = torch.randn(T, 17859, generator=g)
    u0, X, U, du0, dX, dU = control_step_ndp_jvp(eng, x0, xr, ur, other, (tx0, txr, tur, to, tw))
    n, s = eng.net[-1], eng.step[-1]
    assert torch.equal(n["tz"], to[..., :6] - txr[..., :6]) and torch.equal(n["tw"], tw) and n["n_tan"] == T
    assert s["tf"] is n["df"]                                                    # the network's output, handed over as it lies
    assert s["f"] is eng.device_force()                                          # the force the step wrote
    assert torch.equal(s["tx0"], tx0) and torch.equal(s["txr"], txr) and torch.equal(s["tur"], tur)
    tf = n["tz"] @ eng.M.T + tw.double().sum(dim=1)[None, :, None, None]
    assert du0.shape == (B, T, 4) and torch.equal(du0, tf.sum(dim=(2, 3))[:, :, None].expand(-1, -1, 4))
    assert torch.equal(dX, 2.0 * txr) and torch.equal(dU, tur) and torch.equal(X, 2.0 * xr) and torch.equal(U, ur)
    assert u0.shape == (B, 4)
    # nothing behind the force: the network is not called, tf = None
    calls = len(eng.net)
    control_step_ndp_jvp(eng, x0, xr, ur, other, (tx0, None, tur, None, None))
    assert len(eng.net) == calls and eng.step[-1]["tf"] is None
    # without the T axis
    out = control_step_ndp_jvp(eng, x0, xr, ur, other, (None, txr[:, 0], None, to[:, 0], None))
    assert out[3].shape == (B, 4) and out[4].shape == (B, N + 1, 10) and out[5].shape == (B, N, 4)
    assert eng.net[-1]["tz"].shape == (B, 1, N + 1, 6) and eng.step[-1]["tf"].shape == (B, 1, N + 1, 3)
    # other_index gathers the neighbour rows' directions
    idx = torch.tensor([1, 1, -1, 0], dtype=torch.int32)
    control_step_ndp_jvp(eng, x0, xr, ur, other, (None, txr, None, to, None), other_index=idx)
    assert torch.equal(eng.net[-1]["tz"], to[idx.clamp(min=0).long()][..., :6] - txr[..., :6])
