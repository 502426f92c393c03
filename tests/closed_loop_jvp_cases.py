"""What tests/test_closed_loop_jvp.py (CPU) and tests/test_closed_loop_jvp_gpu.py (device) share: the seeds and shapes of the one-call forward
mode's tests, the layout of the directions as the device call takes them, and the measures -- all on tests/closed_loop_chain_ref.py."""
import numpy as np

from tests import closed_loop_chain_ref as R

K, B, SEED = 3, 65, 20231516           # tests/test_closed_loop_vjp_gpu.py's inputs: ext_inputs(65, 3, N, 20231516)
HORIZONS = (20, 7)
TAN_SEED, UPS_SEED = 41, 31
NAMES = ("tx0", "txr", "tur", "tf", "tfp")                       # the device call's directions ...
REF_KEYS = ("t_x0", "t_xr", "t_ur", "t_f", "t_fp")               # ... and closed_loop_chain_ref.tangents' names for them


def directions(ticks, n, N, T, seed=TAN_SEED):
    """{tx0, txr, tur, tf, tfp}: closed_loop_chain_ref.tangents(ticks, n, N, T, seed) under the device call's names (the layouts agree)."""
    t = R.tangents(ticks, n, N, T, seed=seed)
    return {name: t[key] for name, key in zip(NAMES, REF_KEYS)}


def reference(sys_, rec, t):
    """closed_loop_chain_ref.forward along the directions t (a dict of `directions`): (dx, du0, dX), rows in the order of sys_['which']."""
    return R.forward(sys_, rec, t["tx0"], t["txr"], t["tur"], t["tfp"], t_f=t["tf"])


def errors(dev, ref, which=None):
    """rel_err with lead 3 of (dxs, dus, dXs) against the reference's three; which: the device arrays are full-batch, take these vehicles."""
    pick = (lambda a: a) if which is None else (lambda a: a[:, which])
    return {n: R.rel_err(pick(d), r, 3) for n, d, r in zip(("dxs", "dus", "dXs"), dev, ref)}


def duality_gap(fwd, grads, t, ups, absolute=False):
    """[n, T]: |lhs - rhs| over the largest term (absolute: as it is), lhs = <G, dxs> + <H, dus> + <A, dXs>, rhs = <gx0, tx0> + <gxr, txr>
    + <gur, tur> + <gf, tf> + <gfp, tfp>, per vehicle and direction.  Every array holds the same n vehicles: fwd = (dxs, dus, dXs), grads a
    dict x0, xr, ur, f, fp, t a dict of `directions`, ups = (G, H, A)."""
    dx, du, dX = fwd
    G, H, A = ups
    lhs = np.einsum("kvtc,kvc->vt", dx, G) + np.einsum("kvtc,kvc->vt", du, H) + np.einsum("kvtnc,kvnc->vt", dX, A)
    terms = [np.einsum("vtc,vc->vt", t["tx0"], grads["x0"]), np.einsum("kvtnc,kvnc->vt", t["txr"], grads["xr"]),
             np.einsum("kvtnc,kvnc->vt", t["tur"], grads["ur"]), np.einsum("kvtnc,kvnc->vt", t["tf"], grads["f"]),
             np.einsum("kvtc,kvc->vt", t["tfp"], grads["fp"])]
    big = 1.0 if absolute else np.maximum(np.abs(np.array(terms)).max(axis=0), np.abs(lhs))
    return np.abs(lhs - np.sum(terms, axis=0)) / big


def reference_gap(sys_, rec, t, ups):
    """[n]: per referenced vehicle the float64 reference's OWN forward / reverse duality gap, |lhs - rhs| in the worst direction, from
    closed_loop_chain_ref.forward and .reverse alone.  ABSOLUTE, not over the largest term: the upstreams are unit normal, so |lhs - rhs| is
    the disagreement of the two sweeps' tangents in the units rel_err measures a tangent's error in (rows of scale max(1, .)), which the
    largest term (20 .. 100 on these inputs) has nothing to do with.  It is the figure DESIGN section 9 records for the reverse call at
    this model: 9.5e-12 for the one ill-conditioned vehicle, 3.8e-13 .. 1.7e-12 for the others."""
    which = sys_["which"]
    on = lambda a, lead: a[which] if lead == 0 else a[:, which]  # noqa: E731
    tw = dict(tx0=on(t["tx0"], 0), **{n: on(t[n], 1) for n in NAMES[1:]})
    return duality_gap(reference(sys_, rec, t), R.reverse(sys_, rec, *ups), tw, tuple(on(u, 1) for u in ups), absolute=True).max(axis=1)
