"""The float64 reference of the downwash network's optimiser step (csrc/mlp_train.hip; nn_train.py:129-157 with --SN) and the weight
families its tests run on.  Used by tests/test_mlp_train.py (where adam64 is held to torch.optim.Adam) and tests/test_mlp_train_gpu.py.

adam64    one Adam step in float64 from the given state; with round32 (the device's contract) m, v and p are each rounded to float32 once,
          in that order, and p is computed from the ROUNDED m and v.
sigma64   the largest singular value of a weight matrix, numpy's SVD of its float64 copy.
project64 the cap: every layer whose sigma exceeds it becomes float32(W * (cap / sigma)), factor and product in float64; biases untouched.
step64    adam64, then project64, then the norms of the result: what one ndp_mlp_adam_sn_device call leaves.
"""
import numpy as np

from ndp_nmpc_qd_amd import _lib, mlp_frag

LAYERS = ("W1", "W2", "W3", "W4")
REL_BAR = 2.0 ** -20      # project64 / the device leave sigma <= cap (1 + 2^-20): rounding a layer's entries to float32 moves sigma by at most
                          # 2^-24 ||W||_F <= 2^-24 * 8 sigma (rank <= 64); the bar is twice that
CLEAR = 1e-6              # every test keeps each layer's sigma at least this far (relative) from the cap: the branch is then the same on both sides


def weights(blob):
    """The four weight matrices of a blob (views)."""
    p = mlp_frag.split(blob)
    return [p[n] for n in LAYERS]


def sigma64(W):
    return float(np.linalg.svd(np.asarray(W, dtype=np.float64), compute_uv=False)[0])


def sigmas64(blob):
    return np.array([sigma64(W) for W in weights(blob)])


def assert_clear_of_cap(sig, cap):
    """An assertion on the test's INPUTS: no layer sits within 1e-6 (relative) of the cap."""
    if cap > 0:
        assert (np.abs(np.asarray(sig) / cap - 1.0) >= CLEAR).all(), (sig, cap)


def adam64(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, round32=True):
    """(p, m, v) after one step of torch.optim.Adam (no weight decay, no amsgrad), t = step + 1, evaluated in float64."""
    b1, b2 = betas
    t = step + 1
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    r = (lambda a: a.astype(np.float32)) if round32 else (lambda a: a)
    with np.errstate(under="ignore"):
        m = r(b1 * m + (1.0 - b1) * g)
        v = r(b2 * v + (1.0 - b2) * (g * g))
        m64, v64 = m.astype(np.float64), v.astype(np.float64)
        p = r(p - lr / (1.0 - b1 ** t) * (m64 / (np.sqrt(v64) / np.sqrt(1.0 - b2 ** t) + eps)))
    return p, m, v


def project64(blob, cap):
    """(blob', mask, sigma before): the cap applied to a float32 blob."""
    out = np.array(blob, dtype=np.float32, copy=True)
    before = sigmas64(out)
    assert_clear_of_cap(before, cap)
    mask = 0
    if cap > 0:
        for l, W in enumerate(weights(out)):
            if before[l] > cap:
                W[...] = (W.astype(np.float64) * (cap / before[l])).astype(np.float32)
                mask |= 1 << l
    return out, mask, before


def step64(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, cap=0.0):
    """dict(p, m, v, step, sigma, mask, skipped): one ndp_mlp_adam_sn_device call in float64.  A non-finite gradient changes nothing."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    if not np.isfinite(g).all():
        return dict(p=p.copy(), m=m.copy(), v=v.copy(), step=step, sigma=sigmas64(p), mask=0, skipped=1)
    pn, mn, vn = adam64(p, g, m, v, step, lr, betas, eps)
    pn, mask, _ = project64(pn, cap)
    return dict(p=pn, m=mn, v=vn, step=step + 1, sigma=sigmas64(pn), mask=mask, skipped=0)


def ulps(a, b, old=None):
    """|a - b| in float32 ulps, the ulp taken at the largest magnitude among a, b and (when given) the value before the step."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    mag = np.maximum(np.abs(a), np.abs(b))
    if old is not None:
        mag = np.maximum(mag, np.abs(np.asarray(old, dtype=np.float32)))
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(mag).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- weight families
FAMILIES = ("shipped", "equal", "cluster", "rank1", "zero", "wide", "gauss", "mixed")


def _with_singular_values(rng, shape, s):
    """A matrix of `shape` with the singular values s (length = the smaller side), random orthonormal factors."""
    r, c = shape
    k = min(r, c)
    U = np.linalg.qr(rng.normal(size=(r, k)))[0]
    V = np.linalg.qr(rng.normal(size=(c, k)))[0]
    return (U * np.asarray(s, dtype=np.float64)) @ V.T


def family(name):
    """A full float32 blob of the family (the shipped biases throughout: they play no part in a norm)."""
    blob = _lib.load_weights().copy()
    if name == "shipped":
        return blob
    rng = np.random.default_rng(sum(map(ord, name)))
    for l, W in enumerate(weights(blob)):
        k = min(W.shape)
        if name == "equal":            # s Q with orthonormal columns / rows: all singular values equal up to float32 rounding
            new = _with_singular_values(rng, W.shape, np.full(k, 3.0))
        elif name == "cluster":        # the top eight 1e-9 apart
            top = min(8, k)
            new = _with_singular_values(rng, W.shape, np.r_[3.0 * (1.0 + 1e-9 * np.arange(top)), np.linspace(2.9, 0.1, k - top)])
        elif name == "rank1":
            new = 5.0 * np.outer(*(x / np.linalg.norm(x) for x in (rng.normal(size=W.shape[0]), rng.normal(size=W.shape[1]))))
        elif name == "zero":
            new = np.zeros(W.shape)
        elif name == "wide":
            new = _with_singular_values(rng, W.shape, np.logspace(3, -20, k))
        elif name == "gauss":
            new = rng.normal(size=W.shape)
        elif name == "mixed":          # layers 1 and 3 far above any cap the tests use, layers 2 and 4 far below
            new = W.astype(np.float64) * (100.0 if l % 2 == 0 else 0.01)
        else:
            raise KeyError(name)
        W[...] = new.astype(np.float32)
    return blob


# ---------------------------------------------------------------------------------------------------------------- the fit
FIT_B, FIT_N, FIT_STEPS, FIT_CAP = 4, 20, 40, 5.0


def fit_case():
    """(z [B (N+1), 6] input rows, target [B (N+1), 3] = the float64 network under the shipped blob, start [17859] float32 = the shipped
    blob times (1 + 0.02 N(0, 1))): the fit of tests/test_mlp_train_gpu.py, gates open."""
    from tests import mlp_vjp_ref as R
    rng = np.random.default_rng(77)
    z = R.draw_rows(rng, (FIT_B * (FIT_N + 1),))
    shipped = family("shipped")
    target = R.vjp64(shipped, z, np.zeros((z.shape[0], 3)))[3]
    start = (shipped.astype(np.float64) * (1.0 + 0.02 * rng.normal(size=shipped.size))).astype(np.float32)
    return z, target, start
