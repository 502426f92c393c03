"""What the reference-point tests share and what needs numpy only: the segment-tagged trajectories, the tag's decoding, the node and
tick time sequences, and access to tests/golden/ref_point_golden.npz (made by tests/golden/make_ref_point_golden.py with the
50-digit restatement tests/ref_point_ref.py)."""
import os

import numpy as np

from ndp_nmpc_qd_amd.params import nmpc_params as CP
from ndp_nmpc_qd_amd.pt_pub import TrajCoefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_point_golden.npz")

POINT_FAMILIES = ("fixture", "attitude", "yaw", "poly")      # one-segment trajectories, one query time each
N_SEGS = (1, 2, 8, 9, 16, 17, 25)                             # the `segments` family: 8 vehicles per entry
N_VEH = 8
TICK_N_SEGS = (9, 17, 25)                                     # ... of which the tick sequences run these
TAG = 0.05                                                    # segment i's constant yaw coefficient carries TAG (i + 1) rad
MARGIN = 1e-6                                                 # least branch margin of a point that is compared through q
T_HORIZON = float(CP.T_horizon)
TRACE = 3
FLOOR = 32 * 2.0 ** -53                                       # the bar's floor, for values the oracle happens to hit exactly


def bar(oracle_err):
    """The device's bar for a family whose oracle error (same metric) is oracle_err."""
    return max(8.0 * float(oracle_err), FLOOR)


def rel_err(got, want):
    """max over components of |got - want| / max(1, |want|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


def rot_of_q(q):
    """R(q) for q[..., 4] = [w, x, y, z] -> [..., 3, 3]"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def point_err(x, u, want_x, want_u, margin):
    """The metric over a batch of points x[..., 10], u[..., 4].  Where the branch margin is below MARGIN the quaternion's branch (and
    with it its sign and which entry carries the square root) is not determined by the inputs: such a point is compared through
    R(q), every other one through q itself, sign included."""
    x, u, want_x, want_u = (np.asarray(a, dtype=np.float64) for a in (x, u, want_x, want_u))
    tie = np.asarray(margin) < MARGIN
    errs = [rel_err(x[..., 0:6], want_x[..., 0:6]), rel_err(u, want_u), rel_err(x[~tie][..., 6:10], want_x[~tie][..., 6:10]),
            rel_err(rot_of_q(x[tie][..., 6:10]), rot_of_q(want_x[tie][..., 6:10]))]
    return max(errs)


def decode_tag(x):
    """The segment a point x[..., 10] was made from, read off its heading: y_b = z_b x x_c / |.| with x_c = [cos yaw, sin yaw, 0],
    so yaw = atan2(-y_b[0], y_b[1]) while z_b points up; yaw = TAG (segment + 1) + (at most 0.02 rad of untagged yaw); 0 past the
    end (hover at final_pt) -> -1."""
    R = rot_of_q(np.asarray(x)[..., 6:10])
    assert np.all(R[..., 2, 2] > 0.0)
    yaw = np.arctan2(-R[..., 0, 1], R[..., 1, 1])
    return np.rint(yaw / TAG).astype(np.int64) - 1


def segment_of(time_cum, t):
    """The segment rule on doubles (base_pt_publisher.py:93-100 with the oracle's clamp): -1 past the end."""
    time_cum = np.asarray(time_cum, dtype=np.float64)
    if t >= time_cum[-1]:
        return -1
    return max(int(np.count_nonzero(~(time_cum[:-1] > t))) - 1, 0)


def tagged_trajectories(rng, B, n_seg):
    """B vehicles, n_seg segments each with per-vehicle lengths that are multiples of 1/64 s in [1/16, 2]: min-snap / min-acceleration
    polynomials through samples of a slow, small Lissajous curve (as tests/test_ref_window_row.py builds its trajectories), untagged yaw
    within 0.01 rad, then segment i's constant yaw coefficient + TAG (i + 1).  Returns coeff[B, n_seg, 28], time_cum, time_seg, final_pt."""
    tseg = rng.integers(4, 129, size=(B, n_seg)) / 64.0
    cum = np.concatenate([np.zeros((B, 1)), np.cumsum(tseg, axis=1)], axis=1)
    w = np.zeros((B, 4, n_seg + 1))
    ph = rng.uniform(0.0, 2 * np.pi, size=(B, 4, 1))
    om = rng.uniform(0.3, 0.9, size=(B, 4, 1))
    # (continuity holds in NORMALISED time, so a 1/16 s segment beside a 2 s one multiplies the velocity by 32 and the acceleration
    # by 1024 across their boundary: centimetres of amplitude keep the thrust within the upper hemisphere, i.e. the trajectories flyable)
    amp = np.array([0.04, 0.03, 0.006, 0.01]).reshape(1, 4, 1)
    w[:] = amp * np.sin(om * cum[:, None, :] + ph)
    w[:, 2] += 1.0
    tc = TrajCoefficients.from_waypoints(w, tseg)
    coeff = np.concatenate([tc.coeff_x.reshape(B, n_seg, 8), tc.coeff_y.reshape(B, n_seg, 8), tc.coeff_z.reshape(B, n_seg, 8),
                            tc.coeff_yaw.reshape(B, n_seg, 4)], axis=2)
    coeff[:, :, 24] += TAG * (np.arange(n_seg) + 1.0)
    return np.ascontiguousarray(coeff), cum, tseg, tc.final_pt.copy()


def set_traj(eng, coeff, cum, tseg, fpt):
    eng.ref_set_trajectory(coeff[:, :, 0:8], coeff[:, :, 8:16], coeff[:, :, 16:24], coeff[:, :, 24:28], cum, tseg, fpt)


def node_times(t, N, dt):
    """t + k dt, k = 0..N, the product rounded before the sum"""
    return np.array([t + k * dt for k in range(N + 1)])


def tick_times(cum, v):
    """The clock of vehicle v (time_cum `cum`) over the tick sequence: the tick at time t appends the point at t + T_HORIZON.
    30 ticks at 20 ms from the start; a jump forward over at least three segments; 5 ticks; a jump back to near the start; 5 ticks;
    t + T_HORIZON exactly on a time_cum entry, then one ulp before and behind it; one ulp before the end; past the end; back to
    mid-trajectory; the same time twice more.  Returns the times t and what the device adds up, t + T_HORIZON."""
    n_seg = len(cum) - 1
    H = T_HORIZON
    ts = [0.003 + 0.0013 * v - H + 0.02 * i for i in range(30)]
    cur = segment_of(cum, ts[-1] + H)
    far = min(cur + 4, n_seg - 1)
    assert far >= cur + 3
    t = 0.5 * (cum[far] + cum[far + 1]) - H
    ts += [t + 0.02 * i for i in range(6)]
    t = 0.05 + 0.0017 * v - H
    ts += [t + 0.02 * i for i in range(6)]
    j = n_seg - 2
    ts += [cum[j] - H, np.nextafter(cum[j], -np.inf) - H, np.nextafter(cum[j], np.inf) - H]
    ts += [np.nextafter(cum[-1], 0.0) - H, cum[-1] + 0.5 - H]
    mid = 0.25 * cum[n_seg // 2] + 0.75 * cum[n_seg // 2 + 1] - H
    ts += [mid, mid, mid]
    ts = np.array(ts, dtype=np.float64)
    return ts, ts + H


def load():
    return np.load(GOLDEN)


def run_tick_sequence(g, n):
    """The tick sequence of the n-segment vehicles on the device, the newest list entry from three sources per tick: the list's own
    advance (ref_list_window(t), the fill kernel with its segment hint), the control tick on a second handle (the in-launch point with
    its segment cache -- or tick_pre_kernel where the process runs the two-launch form), and ref_window(t + T_horizon) node 0.
    Returns x[3, T, B, 10], u[3, T, B, 4] and the rows of the control-step kernel table the tick handle launched (a *_TICK row: the
    one-launch tick; the library falls back to the two-launch form at shapes that have no such row); the list's u row of an entry
    becomes visible five ticks later (node N - 1 of that window; the window has no u row of node N): u[0:2, i] are filled for
    i < T - 5."""
    import ndp_nmpc_qd_amd as ndp
    coeff, cum, tseg, fpt = (g[f"seg{n}_{k}"] for k in ("coeff", "tcum", "tseg", "fpt"))
    kt, ktt = g[f"seg{n}_kt"], g[f"seg{n}_ktt"]
    B, T = kt.shape
    lst, tck = ndp.BatchedNMPC(B, load_mlp=False), ndp.BatchedNMPC(B, load_mlp=False)
    N = lst.N
    step = int(round(CP.th_pred / CP.ts_nmpc))
    assert N * lst.cfg.dt == T_HORIZON and step == 5
    for e in (lst, tck):
        set_traj(e, coeff, cum, tseg, fpt)
        e.ref_list_reset()
    tck.tick_config(None)
    tck.tick_reset()
    tck.debug_rti_launched()                                   # (reading clears)
    x, u = np.full((3, T, B, 10), np.nan), np.full((3, T, B, 4), np.nan)
    for i in range(T):
        t = np.ascontiguousarray(kt[:, i])
        xa, ua = lst.ref_list_window(t)
        tck.tick(xa[:, 0, :].copy(), t=t, raise_on_status=False)
        xb, ub = tck.ref_list_window(None)
        xc, uc = lst.ref_window(np.ascontiguousarray(ktt[:, i]))
        x[0, i], x[1, i], x[2, i] = xa[:, N], xb[:, N], xc[:, 0]
        u[2, i] = uc[:, 0]
        if i >= step:
            u[0, i - step], u[1, i - step] = ua[:, N - 1], ub[:, N - 1]
    rows = sorted(tck.debug_rti_launched()[0])
    lst.close()
    tck.close()
    return x, u, rows
