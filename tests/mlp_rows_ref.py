"""The float64 reference of the fit on sample rows (ndp_mlp_fit_rows_device), built on tests/mlp_vjp_ref.py: the weighted, indexed squared
error of the 6-128-64-128-3 network and its weight gradient.  Used by tests/test_mlp_rows.py (held there to torch autograd of nn.MSELoss
and to central differences) and tests/test_mlp_rows_gpu.py.

Index rules, as the C interface states them: batch row m uses data row index[m] (None: row m); an index < 0 or >= R is an empty slot that
contributes nothing and whose force is exactly 0; an index listed twice counts twice."""
import numpy as np

from tests import mlp_vjp_ref as R

MARGIN, MAX_DROPPED = R.MARGIN, R.MAX_DROPPED


def gather(index, n_rows, M=None):
    """(src [M] int64 with empty slots clamped to 0, live [M] bool) of an index list over n_rows data rows (None: the first M rows)."""
    if index is None:
        idx = np.arange(n_rows if M is None else M, dtype=np.int64)
    else:
        idx = np.asarray(index, dtype=np.int64)
    live = (idx >= 0) & (idx < n_rows)
    return np.where(live, idx, 0), live


def fit64(blob, z, y, rw, index, scale):
    """(loss, gw [17859], margin [M], f [M,3]): loss = scale * sum_m rw |net(z) - y|^2 over the batch rows, its gradient in the blob's
    order, every batch row's smallest |pre-activation| (inf on empty slots) and the float64 force (0 on empty slots)."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    src, live = gather(index, z.shape[0])
    w = (np.ones(z.shape[0]) if rw is None else np.asarray(rw, dtype=np.float64))[src] * live
    zb, yb = z[src], y[src]
    f = R.vjp64(blob, zb, np.zeros_like(yb))[3]
    e = f - yb
    loss = float(scale * (w * (e * e).sum(axis=1)).sum())
    _, gw, margin, _ = R.vjp64(blob, zb, 2.0 * scale * w[:, None] * e)
    return loss, gw, np.where(live, margin, np.inf), f * live[:, None]


def fit64_at(blob, z, f_dev, y, rw, index, scale):
    """gw [17859]: the float64 VJP with the upstream 2 scale rw (f_dev - y) taken from the DEVICE's float32 predictions f_dev [M,3] -- the
    yardstick of the device's gradient: the forward's own error, held elsewhere, is not charged to the gradient a second time."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    src, live = gather(index, z.shape[0])
    w = (np.ones(z.shape[0]) if rw is None else np.asarray(rw, dtype=np.float64))[src] * live
    e = np.where(live[:, None], np.asarray(f_dev, dtype=np.float64) - y[src], 0.0)
    return R.vjp64(blob, z[src], 2.0 * scale * w[:, None] * e)[1]


def loss64_at(f_dev, y, rw, index, scale):
    """The float64 loss over the device's own float32 predictions, residuals formed in float32 as the kernel forms them."""
    y32 = np.asarray(y, dtype=np.float32)
    src, live = gather(index, y32.shape[0])
    w = (np.ones(y32.shape[0]) if rw is None else np.asarray(rw, dtype=np.float64))[src] * live
    e = (np.asarray(f_dev, dtype=np.float32) - y32[src]).astype(np.float64)
    e[~live] = 0.0
    return float(scale * (w * (e * e).sum(axis=1)).sum())


def margin_weights(rng, margin, lo=0.5, hi=2.0):
    """rw ~ U(lo, hi) as float32 with the margin rule's zeros: rows whose ReLU pattern rounding may decide get weight 0.  Returns (rw,
    share of rows dropped)."""
    rw = rng.uniform(lo, hi, margin.shape[0]).astype(np.float32)
    drop = margin < MARGIN
    rw[drop] = 0.0
    return rw, float(drop.mean())
