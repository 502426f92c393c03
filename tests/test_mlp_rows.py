"""The network on sample rows and its fused fit, CPU side: the float64 reference (tests/mlp_rows_ref.py) held to torch autograd of
nn.MSELoss and to central differences, the two entry points' declarations and bindings, and properties of the two kernels' code
objects.  GPU side: tests/test_mlp_rows_gpu.py."""
import ctypes as C
import os
import re

import numpy as np

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_rows_ref as F
from tests import mlp_vjp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=5, n=40):
    rng = np.random.default_rng(seed)
    blob = _lib.load_weights()
    z = R.draw_rows(rng, (n,))
    y = rng.normal(0.0, 0.5, (n, 3))
    rw = rng.uniform(0.5, 2.0, n)
    index = rng.integers(0, n, 57)
    index[[3, 20, 41]] = -1                     # empty slots
    index[7] = n + 2                            # past the data: empty as well
    index[[10, 11, 12]] = index[9]              # one row four times
    return blob, z, y, rw, index


def test_fit64_is_torch_mse_weighted_indexed():
    """fit64 against autograd of nn.MSELoss(reduction='none') on a float64 nn.Sequential of the same shape, weighted per row and summed
    over an index list with duplicates, -1 and >= R slots: loss and every gradient entry to 1e-12 relative."""
    import torch
    blob, z, y, rw, index = _case()
    p = mlp_frag.split(blob)
    net = torch.nn.Sequential(torch.nn.Linear(6, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3)).double()
    with torch.no_grad():
        for l, lin in enumerate(net[::2], start=1):
            lin.weight.copy_(torch.tensor(p[f"W{l}"].astype(np.float64)))
            lin.bias.copy_(torch.tensor(p[f"b{l}"].astype(np.float64)))
    live = (index >= 0) & (index < z.shape[0])
    src = torch.tensor(index[live])
    n_real = int(live.sum())
    per = torch.nn.MSELoss(reduction="none")(net(torch.tensor(z)[src]), torch.tensor(y)[src])          # [m, 3]
    loss_t = (torch.tensor(rw)[src][:, None] * per).sum() / (3 * n_real)
    loss_t.backward()
    gw_t = torch.cat([t.grad.reshape(-1) for lin in net[::2] for t in (lin.weight, lin.bias)]).numpy()
    loss, gw, margin, f = F.fit64(blob, z, y, rw, index, 1.0 / (3 * n_real))
    assert abs(loss / float(loss_t.detach()) - 1.0) <= 1e-12
    assert np.abs(gw - gw_t).max() <= 1e-12 * np.abs(gw_t).max()
    assert np.isinf(margin[~live]).all() and np.isfinite(margin[live]).all()
    assert (f[~live] == 0.0).all() and f[live].any()
    # plain nn.MSELoss over all rows: no index, no weights, scale 1 / (3 n)
    net.zero_grad()
    plain = torch.nn.MSELoss()(net(torch.tensor(z)), torch.tensor(y))
    loss_p = F.fit64(blob, z, y, None, None, 1.0 / (3 * z.shape[0]))[0]
    assert abs(loss_p / float(plain.detach()) - 1.0) <= 1e-12


def test_fit64_against_central_differences():
    blob, z, y, rw, index = _case(seed=6)
    scale = 1.0 / (3 * 53)
    loss, gw, margin, _ = F.fit64(blob, z, y, rw, index, scale)
    assert margin.min() > 1e-6                  # (no row sits on a kink within the step below)
    off = mlp_frag.offsets()
    picks = [off["W1"][0] + 5, off["b1"][0] + 17, off["W2"][0] + 4321, off["b2"][0] + 3, off["W3"][0] + 777, off["b3"][0] + 100,
             off["W4"][0] + 200, off["b4"][0] + 2]
    h = 1e-6
    for i in picks:
        up, dn = blob.astype(np.float64), blob.astype(np.float64)
        up[i] += h
        dn[i] -= h
        fd = (F.fit64(up, z, y, rw, index, scale)[0] - F.fit64(dn, z, y, rw, index, scale)[0]) / (2 * h)
        assert abs(fd - gw[i]) <= 1e-6 * max(np.abs(gw).max(), abs(gw[i])), (i, fd, gw[i])


def test_fit64_at_uses_the_given_predictions():
    """With the float64 forces handed in, fit64_at is fit64's gradient; the loss over given predictions forms its residuals in float32."""
    blob, z, y, rw, index = _case(seed=7)
    scale = 0.01
    loss, gw, _, f = F.fit64(blob, z, y, rw, index, scale)
    assert np.abs(F.fit64_at(blob, z, f, y, rw, index, scale) - gw).max() <= 1e-13 * np.abs(gw).max()
    z32, y32 = z.astype(np.float32), y.astype(np.float32)
    f32 = F.fit64(blob, z32, y32, rw, index, scale)[3].astype(np.float32)
    assert abs(F.loss64_at(f32, y32, rw, index, scale) / F.fit64(blob, z32, y32, rw, index, scale)[0] - 1.0) < 1e-5


def test_the_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in ("ndp_mlp_rows_device", "ndp_mlp_fit_rows_device"):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        want = [C.c_void_p if "*" in p else scalars[p.split()[0]] for p in params]
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == want, (name, params)
    declared = set(re.findall(r"\b(ndp_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS)
    assert lib.ndp_mlp_rows_device(None, None, None, 1, 1, None, None) == -1
    assert lib.ndp_mlp_fit_rows_device(None, None, None, None, None, 1, 1, 1.0, 0, None, None, None, None, None) == -1
    m = re.search(r"#define\s+NDP_ABI_VERSION\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == lib.ndp_abi_version() == 9
    m = re.search(r"#define\s+NDP_FIT_MAX_GROUPS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.FIT_MAX_GROUPS and 1 <= _lib.FIT_MAX_GROUPS <= 256
    from ndp_nmpc_qd_amd.batched import BatchedNMPC
    assert callable(BatchedNMPC.mlp_rows_device) and callable(BatchedNMPC.mlp_fit_rows_device)
    from ndp_nmpc_qd_amd import torch_layer
    assert callable(torch_layer.downwash_rows) and callable(torch_layer.downwash_fit_rows)
    assert "no autograd" in torch_layer.downwash_rows.__doc__.lower()


def test_row_kernels_isa_properties():
    """Both kernels are in the built library and use no scratch (what the fit's allocator moves aside it keeps in accumulation registers);
    no fixed LDS (the fit's image is dynamic, sized at launch like mlp_vjp_kernel's); the forward alone spills nothing.  They are a unit of
    their own: the backward kernels' code object holds nothing new."""
    from ndp_nmpc_qd_amd import build, isa_inspect
    assert "mlp_fit.hip" in build.UNITS and "mlp_fit.hip" not in build.HOST_ONLY
    build.build()
    co = isa_inspect.CodeObject(_lib.LIB_PATH)
    k = co.kernels()
    found = {}
    for stem in ("mlp_fit_rows_kernel", "mlp_rows_kernel"):
        names = [n for n in k if stem in n]
        assert len(names) == 1, (stem, names)
        m = found[stem] = k[names[0]]
        assert m["scratch"] == 0 and m["sgpr_spill"] == 0, (stem, m)
        assert m["vgpr"] <= 512 and m["lds"] == 0, (stem, m)
    assert found["mlp_rows_kernel"]["spill"] == 0
    home = {co.code_object_of(n) for n in k if "mlp_fit_rows_kernel" in n or "mlp_rows_kernel" in n}
    assert len(home) == 1
    assert sorted(n for n in k if co.code_object_of(n) in home) == sorted(n for n in k if "mlp_fit_" in n or "mlp_rows_kernel" in n)
