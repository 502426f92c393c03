"""What tests/test_model_envelope_gpu.py (device) and tests/test_model_envelope.py (CPU) share: the device cases' batch size, seeds, inputs,
the oracle's twin alone over a case's two steps, and the conditions the forward cases assert."""
import numpy as np

from ndp_nmpc_qd_amd import synth
from tests.kkt_certificate import certify_batch
from tests.model_cases import model_of, oracle_cfg
from tests.step_deriv_emu import MIXED  # (bench.py's `mixed` workload)

B = 61                      # the last workgroup of the 2- and 4-wave launches is ragged
SEED = synth.SEED0 + 7200   # + N: the forward cases' batch; + 50 + N: the forms'; + 100 + N: the derivative cases'
FWD_N = (13, 20, 27, 40)
# The forward cases assert conditions that the oracle's twin alone must meet first: no status, no instance flagged by the certificate, no
# interior-point finish except at `stiff`, and there at least a quarter of the steps.  The batch seed of (model, N) is SEED + N where the
# twin meets them, else the first of SEED + N + 1000 k that does; tests/test_model_envelope.py checks every entry, and the derivative
# cases' counts, by running the twin.  asym_box at N = 40: one instance of seed SEED + 40 leaves the twin's active-set iterations for the
# interior-point loop -- that batch is a device case of its own (FALLBACK), held to the twin and certified under the interior-point bar.
FWD_SEED = {("asym_box", 40): SEED + 40 + 1000}
FALLBACK = ("asym_box", 40, SEED + 40)


def fwd_seed(name, N):
    return FWD_SEED.get((name, N), SEED + N)


def batch(case, N, seed, t=0, downwash=False):
    """The mixed workload at the case's dt, tick t."""
    return synth.make_batch(B, N=N, seed=seed, downwash=downwash, dt=model_of(case)[6], t0=0.02 * t, **MIXED)


def force(N, seed, dtype=np.float32):
    return np.random.default_rng(seed + 1).normal(0.0, 0.3, (B, N + 1, 3)).astype(dtype)


def twin_two_ticks(oracle, case, N, seed, f=None, same=False):
    """The oracle's twin alone over the two steps of a device case (same: the derivative cases' warm-up and recorded step on one set of
    inputs): per tick (status, iteration word, kept sets, instances the certificate flags)."""
    use_fd = f is not None
    twin = oracle_cfg(oracle, case, N=N, use_fd=use_fd)
    twin.qp_mode = 0
    b = batch(case, N, seed)
    X, U = b["xr"].copy(), b["ur"].copy()
    act = np.zeros((B, N, 4), dtype=np.int8)
    ticks = []
    for t in range(2):
        b = batch(case, N, seed, 0 if same else t)
        Xp, Up = X.copy(), U.copy()
        _, st, it, _ = oracle.step_batch_as(twin, b["x0"], b["xr"], b["ur"], None if f is None else f.astype(np.float64), X, U, act)
        cs = certify_batch(oracle, oracle_cfg(oracle, case, N=N, use_fd=use_fd), b["x0"], b["xr"], b["ur"], f, Xp, Up, X, U)
        ticks.append((st.copy(), it.copy(), act.copy(), sum(c["flag"] for c in cs)))
    return ticks


def n_interior_point(ticks):
    return sum(int((it > 0).sum()) for _, it, _, _ in ticks)


def clean(ticks):
    """No status and no instance flagged by the certificate, on (status, iteration word, sets, flagged) per tick."""
    return not any(st.any() for st, _, _, _ in ticks) and not any(fl for _, _, _, fl in ticks)


def forward_conditions(name, ticks):
    """The conditions test_forward_step_follows_the_model asserts."""
    n_ipm = n_interior_point(ticks)
    return clean(ticks) and (n_ipm >= 2 * B // 4 if name == "stiff" else n_ipm == 0)
