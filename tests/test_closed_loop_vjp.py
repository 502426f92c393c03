"""The one-call closed loop and its reverse mode (ndp_closed_loop_device, ndp_closed_loop_vjp_device), CPU side: the interface (header,
binding, interface version), the two link kernels' code-object properties, the torch layer's `closed_loop` on a stub engine, and the
MODEL-gradient composition of the reference (tests/closed_loop_vjp_ref.py) held to central differences of the oracle's closed loop.
Device side: tests/test_closed_loop_vjp_gpu.py."""
import os
import re
import types

import numpy as np
import pytest

from ndp_nmpc_qd_amd import build, isa_inspect as I
from tests import closed_loop_chain_ref as R
from tests import closed_loop_vjp_ref as M
from tests.test_closed_loop_chain_gpu import _pick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ndp_closed_loop_tape_bytes", "ndp_closed_loop_device", "ndp_closed_loop_vjp_device")
KERNELS = ("closed_loop_fwd_link_kernel", "closed_loop_rev_link_kernel")
FD_BAR = 1e-6                                        # tests/test_closed_loop_chain.py's and test_model_grad_gpu.py's finite-difference bar


def test_every_export_is_declared_and_bound():
    from ndp_nmpc_qd_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "ndp_nmpc.h")) as fh:
        hdr = fh.read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
        assert re.search(r"\bint %s\(ndp_handle \*h, int ticks," % name, hdr), name
    assert len(lib.ndp_closed_loop_device.argtypes) == 15 and len(lib.ndp_closed_loop_vjp_device.argtypes) == 23
    with open(os.path.join(ROOT, "ndp_nmpc_qd_amd", "build.py")) as fh:
        assert '"closed_loop.hip"' in fh.read()


def test_the_interface_version_stays_9():
    from ndp_nmpc_qd_amd import _lib
    with open(os.path.join(ROOT, "include", "ndp_nmpc.h")) as fh:
        m = re.search(r"#define NDP_ABI_VERSION (\d+)", fh.read())
    assert m and int(m.group(1)) == 9 and _lib.ABI_VERSION == 9
    assert _lib.load().ndp_abi_version() == 9


def test_the_link_kernels_keep_their_state_in_registers():
    """No scratch, no spill, no LDS, at most 256 VGPRs; both in one code object (csrc/closed_loop.hip's), which is not the one the plant's
    rollout kernels live in."""
    co = I.CodeObject(build.build())
    k = co.kernels()
    home = set()
    for part in KERNELS:
        found = [n for n in k if part in n]
        assert len(found) == 1, (part, found)
        v = k[found[0]]
        assert v["scratch"] == 0 and v["spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (part, v)
        assert v["vgpr"] + v["agpr"] <= 256, (part, v)
        home.add(co.code_object_of(found[0]))
    assert len(home) == 1
    plant = [n for n in k if "plant_rollout_vjp_kernel" in n]
    assert len(plant) == 1 and co.code_object_of(plant[0]) not in home


# ---- the torch layer on a stub engine
class _Stub:
    """closed_loop_device / closed_loop_vjp_device on CPU tensors: records what it was handed; the outputs are simple functions of the
    inputs, the gradients constants per output."""

    def __init__(self, B, N):
        self.B, self.N = B, N
        self.cfg = types.SimpleNamespace(Qd=[1.0] * 10, Rd=[2.0] * 4, mass=1.5)
        self.calls = []

    def set_model(self, Qd=None, Rd=None, mass=None):
        self.calls.append(("set_model", Qd, Rd, mass))
        if Qd is not None:
            self.cfg.Qd = list(Qd)
        if Rd is not None:
            self.cfg.Rd = list(Rd)
        if mass is not None:
            self.cfg.mass = mass

    def closed_loop_tape(self, ticks):
        import torch
        return torch.zeros((ticks, 256), dtype=torch.uint8)

    def closed_loop_device(self, x0, xr, ur, xs, us, f=None, fp=None, Xs=None, status=None, tape=None, dt=None, substeps=None, stream=None):
        self.calls.append(("fwd", dict(x0=x0, xr=xr, ur=ur, f=f, fp=fp, dt=dt, substeps=substeps, stream=stream, tape=tape)))
        xs[:] = x0[None] + 1.0
        us[:] = ur[:, :, 0, :]
        Xs[:] = xr
        tape[:] = 7

    def closed_loop_vjp_device(self, x0, xr, ur, xs, us, tape, f=None, fp=None, gxs=None, gus=None, gXs=None, gx0=None, gxr=None, gur=None,
                               gf=None, gfp=None, gmodel=None, status_check=None, dt=None, substeps=None, stream=None):
        outs = dict(gx0=gx0, gxr=gxr, gur=gur, gf=gf, gfp=gfp, gmodel=gmodel)
        self.calls.append(("bwd", dict(f=f, fp=fp, tape=tape, ups=(gxs, gus, gXs), dt=dt, substeps=substeps,
                                       asked={n for n, t in outs.items() if t is not None})))
        for i, t in enumerate(outs.values()):
            if t is not None:
                t[:] = float(i + 1)
        if gmodel is not None:
            gmodel[:] = 1.0
            gmodel[:, 14], gmodel[:, 15] = 3.0, 0.5
            gmodel[1] = float("nan")                 # a failed vehicle contributes nothing


def test_torch_closed_loop_on_a_stub_engine():
    """Argument marshalling (detached contiguous tensors, f float32 as given, dt and substeps passed on, the model installed by value), the
    three outputs, ONE backward call, only the leaves that require a gradient asked for, f's gradient in f's dtype, the mass' gradient the
    sum of columns 14 and 15 over the finite rows."""
    torch = pytest.importorskip("torch")
    from ndp_nmpc_qd_amd import torch_layer as TL
    K, B, N = 3, 4, 5
    g = torch.Generator().manual_seed(3)
    mk = lambda *s, dt=torch.float64: torch.randn(*s, generator=g, dtype=dt)  # noqa: E731
    eng = _Stub(B, N)
    x0, xr, ur = mk(B, 10).requires_grad_(), mk(K, B, N + 1, 10), mk(K, B, N, 4).requires_grad_()
    f, fp = mk(K, B, N + 1, 3, dt=torch.float32).requires_grad_(), mk(K, B, 3)
    Qd = torch.full((10,), 1.0, dtype=torch.float64, requires_grad=True)
    Rd = torch.full((4,), 2.5, dtype=torch.float64)
    mass = torch.tensor(1.5, dtype=torch.float64, requires_grad=True)
    xs, us, Xs = TL.closed_loop(eng, x0, xr, ur, f=f, fp=fp, Qd=Qd, Rd=Rd, mass=mass, dt=0.02, substeps=2)
    assert eng.calls[0] == ("set_model", None, (2.5,) * 4, None)          # only what differs from the engine's values
    kind, fw = eng.calls[1]
    assert kind == "fwd" and fw["dt"] == 0.02 and fw["substeps"] == 2 and fw["stream"] is None
    assert fw["f"].dtype == torch.float32 and not fw["f"].requires_grad and not fw["x0"].requires_grad
    assert tuple(xs.shape) == (K, B, 10) and tuple(us.shape) == (K, B, 4) and tuple(Xs.shape) == (K, B, N + 1, 10)
    assert torch.equal(xs, (x0.detach()[None] + 1.0).expand(K, B, 10)) and torch.equal(Xs, xr)
    (xs.sum() + 2.0 * us.sum()).backward()
    assert [c[0] for c in eng.calls] == ["set_model", "fwd", "bwd"]
    bw = eng.calls[2][1]
    assert bw["asked"] == {"gx0", "gur", "gf", "gmodel"} and bw["ups"][2] is None and bw["dt"] == 0.02 and bw["substeps"] == 2
    assert torch.equal(bw["ups"][0], torch.ones(K, B, 10, dtype=torch.float64)) and torch.equal(bw["ups"][1], torch.full((K, B, 4), 2.0, dtype=torch.float64))
    assert (bw["tape"] == 7).all() and bw["f"].dtype == torch.float32
    assert torch.equal(x0.grad, torch.full((B, 10), 1.0, dtype=torch.float64)) and torch.equal(ur.grad, torch.full((K, B, N, 4), 3.0, dtype=torch.float64))
    assert f.grad.dtype == torch.float32 and torch.equal(f.grad, torch.full((K, B, N + 1, 3), 4.0))
    assert xr.grad is None and fp.grad is None and Rd.grad is None
    assert torch.equal(Qd.grad, torch.full((10,), float(B - 1), dtype=torch.float64))
    assert mass.grad.shape == mass.shape and float(mass.grad) == (B - 1) * 3.5
    # nothing requires a gradient: no backward call; the model changed behind the layer's back: the backward raises
    xs2, _, _ = TL.closed_loop(eng, x0.detach(), xr, ur.detach(), fp=fp)
    assert not xs2.requires_grad
    xs3, _, _ = TL.closed_loop(eng, x0, xr, ur)
    eng.cfg.mass = 2.0
    with pytest.raises(RuntimeError, match="model .* was changed"):
        xs3.sum().backward()


# ---- the model gradient's composition
def test_model_gradient_composition_against_the_oracles_closed_loop(oracle):
    """ext form, B = 65, K = 3, N = 7 on the oracle's own record: sum_k model_grad_ref with the reverse sweep's upstreams plus the plant's
    mass share, against central differences of the oracle's closed loop (every tick restarted from the recorded iterate and kept set) in
    Qd[0], Rd[3] and the mass -- within 1e-6 of max(1, |g|) on the referenced vehicles, all of which keep their sets in every run.  The
    mass moves controller and plant together: its derivative is column 14 + column 15, and the plant's share is not small."""
    K, N, B = 3, 7, 65
    a = R.ext_inputs(B, K, N, 20231516)
    rec = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], f=a["f"])
    ok = R.set_finish(rec)
    which = _pick(rec, ok)
    assert len(which) == 6
    G, H, A = R.upstreams(K, B, N, seed=31)
    sys_ = R.systems(oracle, rec, which)
    tot, per = M.model_reverse(oracle, sys_, rec, G, H, A)
    assert not tot[:, 6].any() and np.abs(tot[:, 15]).max() > 1e-3
    for col, got in ((0, tot[:, 0]), (13, tot[:, 13]), (14, tot[:, 14] + tot[:, 15])):
        fd, stable = M.model_fd(oracle, rec, G, H, A, col)
        assert stable[which].all(), (col, stable[which])
        err = np.abs(fd[which] - got) / np.maximum(1.0, np.abs(got))
        print(f"column {col}: worst |fd - g| / max(1, |g|) = {err.max():.2e}, |g|max {np.abs(got).max():.2e}")
        assert err.max() <= FD_BAR, (col, err)
        assert np.abs(got).max() > 1e-6
