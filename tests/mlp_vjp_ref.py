"""The reference derivative of the downwash network: the 6-128-64-128-3 ReLU network (Linear ReLU Linear ReLU Linear ReLU Linear) written
in torch float64 from the weight blob, autograd for the gradient of its input rows and of its weights, and every row's smallest |hidden
pre-activation| -- the margin by which its ReLU pattern is decided.  Used by tests/test_downwash_vjp.py (checked there against central
finite differences) and tests/test_downwash_vjp_gpu.py."""
import numpy as np
import torch

from ndp_nmpc_qd_amd import mlp_frag

MARGIN = 1e-4      # rows whose smallest |pre-activation| is below this may have a ReLU decided by rounding (fp32 against fp64)
MAX_DROPPED = 0.08


def params64(blob):
    """{name: float64 tensor} of the eight parameter groups of a blob (numpy float32 [17859])."""
    return {k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in mlp_frag.split(np.asarray(blob)).items()}


def forward64(p, z):
    """(force [R,3], margin [R]) for input rows z [R,6] float64: margin = min over the three hidden layers of |pre-activation|."""
    h, margin = z, None
    for l in (1, 2, 3):
        pre = h @ p[f"W{l}"].T + p[f"b{l}"]
        m = pre.detach().abs().min(dim=1).values
        margin = m if margin is None else torch.minimum(margin, m)
        h = torch.relu(pre)
    return h @ p["W4"].T + p["b4"], margin


def vjp64(blob, z, gf):
    """The network's vector-Jacobian product in float64: z [R,6] input rows, gf [R,3] upstream (a row of zeros drops out of everything).
    Returns numpy (g_z [R,6], g_w [17859] in blob order, margin [R], force [R,3])."""
    p = {k: v.clone().requires_grad_(True) for k, v in params64(blob).items()}
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    f, margin = forward64(p, zt)
    names = [n for n, _ in mlp_frag.SHAPES]
    grads = torch.autograd.grad(f, [zt] + [p[n] for n in names], grad_outputs=torch.tensor(np.asarray(gf, dtype=np.float64)))
    gw = torch.cat([g.reshape(-1) for g in grads[1:]])
    return grads[0].numpy(), gw.numpy(), margin.numpy(), f.detach().numpy()


def draw_rows(rng, shape):
    """other - ego rows as the network's golden inputs are drawn: positions U(-1.5, 1.5), velocities U(-3, 3); shape (..., 6)."""
    z = np.empty(tuple(shape) + (6,))
    z[..., :3] = rng.uniform(-1.5, 1.5, tuple(shape) + (3,))
    z[..., 3:] = rng.uniform(-3.0, 3.0, tuple(shape) + (3,))
    return z


def group_errors(gw, ref):
    """{group: max|gw - ref| / max|ref|} over the eight parameter groups."""
    out = {}
    for name, (o, shp) in mlp_frag.offsets().items():
        n = int(np.prod(shp))
        out[name] = float(np.abs(gw[o:o + n] - ref[o:o + n]).max() / np.abs(ref[o:o + n]).max())
    return out
