"""The horizons at which the control step's derivative passes (RtiWave::sens_out level 2, psens_out, vjp_out, vjp_out<true>, jvp_out) change
shape, and what tests/test_deriv_edges.py (host emulator) and tests/test_deriv_edges_gpu.py (device) share: the list, the counts it is derived
from, and the device cases' batch."""
import numpy as np

from ndp_nmpc_qd_amd import synth
from tests.step_deriv_emu import MIXED

# The out-passes are `lane + 64 * t` chunk loops over 10(N+1) state entries, 4N input entries, 3(N+1) force entries, 4(N+1) attitude
# entries and 6(N+1) position / velocity entries; the constraint slots (slots_for) and the instances per workgroup (geometry) follow the
# horizon too, and `14 N + 10 >= 64` picks the LDL sweep after an interior-point finish.  One reason per entry:
#    2  the smallest horizon (every loop a single, mostly idle chunk)
#    3  the last horizon that takes the plain sweep after an interior-point finish (14 N + 10 = 52)
#    4  the first that takes the LDL sweep there (66)
#    6  10(N+1) = 70: the state loops' second chunk (60 at N = 5)
#   10  slots 1 -> 2 (7N - 3 = 67); 6(N+1) = 66: a second chunk (60 at N = 9)
#   12  10(N+1) = 130: a third chunk (120 at N = 11)
#   15  4(N+1) = 64: exactly one full chunk
#   16  4N = 64: exactly one full chunk; 4(N+1) = 68: a second chunk
#   17  4N = 68: the inputs' second chunk, the kept set's second register per lane
#   19  slots 2 -> 3 (7N - 3 = 130); 10(N+1) = 200: a fourth chunk (190 at N = 18)
#   21  3(N+1) = 66: the force's second chunk (63 at N = 20); 6(N+1) = 132: a third; 4 -> 2 instances per workgroup; the sweep's second
#       re-symmetrisation
#   25  10(N+1) = 260: a fifth chunk (250 at N = 24)
#   27  the largest horizon the derivative kernels serve
# N = 20 changes nothing against 19 but is the compile-time horizon: its kernels have cases of their own in every derivative module.
DERIV_EDGE_N = (2, 3, 4, 6, 10, 12, 15, 16, 17, 19, 21, 25, 27)


def chunk_sizes(N):
    """The element counts the out-passes loop over in chunks of 64 lanes."""
    return (10 * (N + 1), 4 * N, 3 * (N + 1), 4 * (N + 1), 6 * (N + 1))


def ldl_after_interior_point(N):
    """vjp_out's and jvp_out's sweep choice after an interior-point finish."""
    return 14 * N + 10 >= 64


DEVICE_B = 37           # ragged at four instances per workgroup (37 = 9 * 4 + 1) and at two (18 * 2 + 1)


def device_case(N, seed, fused=False):
    """The device cases' inputs at horizon N: the mixed workload (neighbour windows beside it with fused: they do not move x0, xr, ur)
    and a supplied fp32 force."""
    b = synth.make_batch(DEVICE_B, N=N, seed=seed, downwash=fused, **MIXED)
    f = np.random.default_rng(seed + 1).normal(0.0, 0.3, (DEVICE_B, N + 1, 3)).astype(np.float32)
    return b, f


def small_case(N, seed, B):
    """The first B instances of device_case(N, seed): the small batches of the lowered-waves and the optional-pointer cases."""
    b, f = device_case(N, seed)
    return {k: v[:B] for k, v in b.items() if isinstance(v, np.ndarray) and v.shape[:1] == (DEVICE_B,)}, f[:B]


def twin_finishes(oracle, N, b, f):
    """The oracle's twin of the device's default QP mode over the warm-up step and the recorded step, from the reset iterate (xr, ur) and
    empty kept sets, the same inputs at both: (set finish [B] bool, pinned [B] bool) of the recorded step -- status 0, no interior-point
    iteration; an input on a bound in the final set."""
    cfg = oracle.default_cfg(N=N, use_fd=True)
    cfg.qp_mode = 0
    X, U = b["xr"].copy(), b["ur"].copy()
    act = np.zeros((b["x0"].shape[0], N, 4), dtype=np.int8)
    for _ in range(2):
        _, st, it, _ = oracle.step_batch_as(cfg, b["x0"], b["xr"], b["ur"], np.asarray(f, dtype=np.float64), X, U, act)
    ok = (st == 0) & ((it & 0xffff) == 0)
    return ok, ok & act.any(axis=(1, 2))


def pick(ok, pinned, n=6, n_pinned=2):
    """The instances a device case holds to the dense references: the first n_pinned pinned set finishes, then free ones (then further
    pinned ones) up to n."""
    p, fr = np.flatnonzero(pinned), np.flatnonzero(ok & ~pinned)
    idx = list(p[:n_pinned]) + list(fr[:n - min(n_pinned, p.size)])
    idx += list(p[n_pinned:n_pinned + n - len(idx)])
    return sorted(int(i) for i in idx)
