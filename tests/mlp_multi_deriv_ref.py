"""The reference derivatives of the downwash force summed over K neighbour slots, in float64 torch on tests/mlp_vjp_ref.py and
tests/mlp_jvp_ref.py: the force is the sum over the OPEN slots of the float64 network, g_z is per slot, g_w and df are sums over the
slots.  And the inputs of the reference comparisons: every (instance, slot) has a row of `other` of its own, every input row whose
smallest float64 |pre-activation| is below mlp_vjp_ref.MARGIN is REDRAWN until it is not (nothing is dropped: with K slots sharing one
upstream the single-neighbour rule -- zero the upstream of such rows -- would drop 8.5 % of the rows at K = 2 and 30 % at K = 8), and no
gate distance lies within 10 % of r_horiz^2.  Used by tests/test_downwash_multi_deriv.py and tests/test_downwash_multi_deriv_gpu.py."""
import numpy as np

from tests import mlp_jvp_ref as J
from tests import mlp_vjp_ref as R

MAX_ROUNDS = 40      # of the redraw loop: a round redraws ~4.4 % of what the round before it redrew


def force64(blob, z, open_):
    """f [B,np1,3]: the sum over the open slots of the float64 network on z [B,K,np1,6]; open_ [B,K] bool."""
    B, K, np1 = z.shape[:3]
    f = R.vjp64(blob, z.reshape(-1, 6), np.zeros((B * K * np1, 3)))[3].reshape(B, K, np1, 3)
    return (f * open_[:, :, None, None]).sum(axis=1)


def vjp64(blob, z, open_, gf):
    """The adjoint of force64: gf [B,np1,3] is the upstream of the SUM, so every open slot sees it.  Returns (g_z [B,K,np1,6] per slot, 0 on
    closed slots; g_w [17859], the sum over rows and slots; margin [B,K,np1])."""
    B, K, np1 = z.shape[:3]
    up = np.broadcast_to(gf[:, None], (B, K, np1, 3)) * open_[:, :, None, None]
    gz, gw, margin, _ = R.vjp64(blob, z.reshape(-1, 6), up.reshape(-1, 3))
    return gz.reshape(B, K, np1, 6), gw, margin.reshape(B, K, np1)


def jvp64(blob, z, open_, tz=None, tw=None):
    """The tangent of force64 along tz [B,K,np1,6] (per slot, None = 0) and tw [17859] (None = 0): df [B,np1,3], the sum over the open
    slots."""
    B, K, np1 = z.shape[:3]
    d = J.jvp64(blob, z.reshape(-1, 6), None if tz is None else tz.reshape(-1, 6), tw)[0].reshape(B, K, np1, 3)
    return (d * open_[:, :, None, None]).sum(axis=1)


def draw_own_rows(rng, blob, B, K, np1, want_open=None, r_h=1.0):
    """Inputs in which every slot has a row of its own: z [B,K,np1,6] as mlp_vjp_ref.draw_rows draws them, except that node 0's xy of slot
    (i, k) is off[i] + rad (cos, sin) with rad U(0, 0.9 r_h) where want_open[i, k] and U(1.1 r_h, 3 r_h) where not (want_open None: no
    gate, plain rows) -- off [B,2] is ego_xy minus the ego window's xy at node 0, so |other xy - ego_xy| = rad.  Rows below the margin are
    redrawn by the same rule until none is.  Returns (z, off, redrawn rows in total, rounds)."""
    z = np.empty((B, K, np1, 6))
    off = rng.uniform(-0.5, 0.5, (B, 2))
    todo = np.ones((B, K, np1), dtype=bool)
    redrawn, rounds = -todo.sum(), 0
    while todo.any():
        rounds += 1
        assert rounds <= MAX_ROUNDS, "the redraw loop does not terminate"
        ii, kk, nn = np.nonzero(todo)
        new = R.draw_rows(rng, (len(ii),))
        if want_open is not None:
            at0 = nn == 0
            w = want_open[ii[at0], kk[at0]]
            rad = np.where(w, rng.uniform(0.0, 0.9 * r_h, w.size), rng.uniform(1.1 * r_h, 3.0 * r_h, w.size))
            ang = rng.uniform(0.0, 2.0 * np.pi, w.size)
            new[at0, 0:2] = off[ii[at0]] + (rad * np.array([np.cos(ang), np.sin(ang)])).T
        z[ii, kk, nn] = new
        redrawn += len(ii)
        margin = R.vjp64(blob, new, np.zeros((len(ii), 3)))[2]
        todo = np.zeros_like(todo)
        todo[ii, kk, nn] = margin < R.MARGIN
    return z, off, int(redrawn), rounds


def own_row_case(seed, blob, B, K, N, gates, xr=None, r_h=1.0):
    """One own-row case: gates 'open' (no ego_xy) or 'mixed' (about a third of the slots open, every K > 1 case with instances whose slot
    0 is closed and a later slot open).  xr: the ego windows [B,N+1,10] (None: N(0, 1)); r_h: the gate's radius.  Returns a dict of numpy arrays: other [B K,N+1,10], index int32 [B,K] (= i K + k), xr, ego_xy or
    None, z [B,K,N+1,6] (what the network sees, recomputed from other - xr), open [B,K], redrawn, rounds."""
    rng = np.random.default_rng(seed)
    np1 = N + 1
    want = None
    if gates == "mixed":
        want = rng.random((B, K)) < 0.36
        if K > 1:
            want[0, 0], want[0, 1:] = False, True              # slot 0 closed, the later ones open: for certain
    z, off, redrawn, rounds = draw_own_rows(rng, blob, B, K, np1, want, r_h)
    xr = rng.normal(0.0, 1.0, (B, np1, 10)) if xr is None else np.array(xr, dtype=np.float64)
    other = rng.normal(0.0, 1.0, (B, K, np1, 10))
    other[..., :6] = xr[:, None, :, :6] + z
    ego_xy, open_ = None, np.ones((B, K), dtype=bool)
    if want is not None:
        ego_xy = xr[:, 0, :2] + off
        d = other[:, :, 0, :2] - ego_xy[:, None]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        r2 = r_h * r_h
        assert not ((d2 > 0.9 * r2) & (d2 < 1.1 * r2)).any()            # no gate within 10 % of r_horiz^2
        open_ = d2 < r2
        assert np.array_equal(open_, want)
    z = other[..., :6] - xr[:, None, :, :6]                    # as the device forms it (the sum above is rounded)
    return dict(other=other.reshape(B * K, np1, 10), index=np.arange(B * K, dtype=np.int32).reshape(B, K), xr=xr, ego_xy=ego_xy, z=z,
                open=open_, redrawn=redrawn, rounds=rounds, d2=None if want is None else d2)
