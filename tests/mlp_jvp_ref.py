"""The reference forward-mode derivative of the downwash network in float64, written out layer by layer (no autograd: tests/mlp_vjp_ref.py's
vjp64 is autograd, so the duality of the two is a check of both).  Built on mlp_vjp_ref.params64 / forward64.  Used by
tests/test_downwash_jvp.py (checked there against central finite differences and against vjp64) and tests/test_downwash_jvp_gpu.py."""
import numpy as np
import torch

from ndp_nmpc_qd_amd import mlp_frag
from tests import mlp_vjp_ref as R


def jvp64(blob, z, tz=None, tw=None):
    """The network's Jacobian-vector product in float64: z [R,6] input rows, tz [R,6] their direction (None = 0), tw [17859] the
    direction of the weights in blob order (None = 0).  Returns numpy (df [R,3], margin [R], force [R,3]); margin as forward64's."""
    p = R.params64(blob)
    zt = torch.tensor(np.asarray(z, dtype=np.float64))
    f, margin = R.forward64(p, zt)
    d = None if tw is None else {k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in mlp_frag.split(np.asarray(tw)).items()}
    h, dh = zt, torch.zeros_like(zt) if tz is None else torch.tensor(np.asarray(tz, dtype=np.float64))
    for l in (1, 2, 3, 4):
        pre = h @ p[f"W{l}"].T + p[f"b{l}"]
        dpre = dh @ p[f"W{l}"].T
        if d is not None:
            dpre = dpre + h @ d[f"W{l}"].T + d[f"b{l}"]
        if l == 4:
            assert torch.equal(pre, f)
            return dpre.numpy(), margin.numpy(), f.numpy()
        h, dh = torch.relu(pre), dpre * (pre > 0)
