"""What tests/test_plant_side_envelope_gpu.py (device) and tests/test_plant_side_envelope.py (CPU) share: the models and gate radii at
which the plant side and the closed loop are held to references (tests/model_cases.py: PLANT_CASES, LOOP_CASE, RADII), the shapes, the
seeds, the inputs, and the conditions the inputs must meet -- checked on the oracle and the float64 references alone by the CPU test,
so that a device test never finds out on the device that its inputs are no test.

Every group also has its `default` twin: the same inputs, the reference at the default model (mass 1.4844, g 9.81) or radius (1.0).  The
CPU test asserts that the twin lies at least NOTICE = 100 bars from the case's reference in the comparison's own measure: a kernel that
folded a default would miss the device test by two orders of magnitude, not by a rounding."""
import numpy as np

from ndp_nmpc_qd_amd.params import nmpc_params as CP
from tests import closed_loop_chain_ref as R
from tests import closed_loop_vjp_ref as M
from tests import formation_multi_ref as FM
from tests import formation_ref as FR
from tests import mlp_multi_deriv_ref as MM
from tests import plant_deriv_ref as P
from tests import plant_force_deriv_ref as PF
from tests.test_closed_loop_chain_gpu import _pick  # (imports without a GPU; tests/test_closed_loop_vjp.py takes it the same way)
from tests.model_cases import LOOP_CASE, PLANT_CASES, RADII, model_of, oracle_cfg  # noqa: F401

B = 65                       # one vehicle past a full 64-lane workgroup of the plant's and the closed loop's link kernels
DT = CP.ts_nmpc
NOTICE = 100.0               # the default twin differs from the case's reference by at least this many bars
MAX_SEEDS = 20               # a seed that meets its conditions is among the first MAX_SEEDS from its base


# ---------------------------------------------------------------- a. the plant's rollout derivatives
PLANT_TICKS, PLANT_SUBSTEPS, PLANT_T = 3, (1, 4), 4
_plant = {}


def plant_reference(name, sub):
    """Inputs (with a force), the complex-step Jacobian at the case's mass and g, and seeded upstreams / tangents (T = 4): computed
    once, shared, never written."""
    if (name, sub) not in _plant:
        mass, g = model_of(PLANT_CASES[name])[2:4]
        x0, u, f = P.inputs(B, PLANT_TICKS, seed=7300 + 10 * sorted(PLANT_CASES).index(name) + sub)
        rng = np.random.default_rng(7)
        T = PLANT_T
        r = dict(x0=x0, u=u, f=f, mass=mass, g=g, J=P.jacobian(x0, u, f, DT, sub, mass, g), gxs=rng.normal(size=(PLANT_TICKS, B, 10)),
                 tx0=rng.normal(size=(B, T, 10)), tu=rng.normal(size=(PLANT_TICKS, B, T, 4)), tf=rng.normal(size=(PLANT_TICKS, B, T, 3)))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _plant[name, sub] = r
    return _plant[name, sub]


# ---------------------------------------------------------------- b. the force on the plant
FORCE_SHAPES = ((7, 3), (64, 3))
# shared_case's seed per (B, K, radius): the first from force_seed_base that meets force_conditions (found by running them on the CPU;
# tests/test_plant_side_envelope.py checks every entry)
FORCE_SEED = {(7, 3, 0.75): 8134, (7, 3, 1.5): 8139, (64, 3, 1.5): 13837}
_force = {}


def force_seed_base(Bf, K, r):
    return 7400 + 100 * Bf + 10 * K + int(round(4 * r))


def force_seed(Bf, K, r):
    return FORCE_SEED.get((Bf, K, r), force_seed_base(Bf, K, r))


def force_case(blob, Bf, K, r, seed=None):
    """plant_force_deriv_ref.shared_case at the gate radius r (the redraw loop judges the rim at r)."""
    key = (Bf, K, r, seed)
    if key not in _force:
        _force[key] = PF.shared_case(force_seed(Bf, K, r) if seed is None else seed, blob, Bf, K, r2=r * r)
    return _force[key]


def force_meets(c, r):
    share, clear, both = force_conditions(c, r)
    return share >= 0.1 and clear and both


def force_conditions(c, r):
    """(share of the occupied slots whose gate at r differs from their gate at 1.0, no gate distance within 10 % of r^2, an open slot
    and a closed one at r)."""
    x, idx = c["x"], c["index"]
    _, has, d2 = PF.gather(x, idx, False)
    at_r, at_1 = d2 < r * r, d2 < 1.0
    near = has & (d2 > 0.9 * r * r) & (d2 < 1.1 * r * r)
    return float((has & (at_r != at_1)).sum()) / float(has.sum()), not near.any(), bool((has & at_r).any() and (has & ~at_r).any())


def ring_case(seed, Bf=7, K=3):
    """Every (vehicle, neighbour) pair between 0.75 and 1.0 apart horizontally, away from both rims (d^2 in 0.70 .. 0.83): the even
    vehicles sit around one point, the odd ones around another 0.875 away, and a vehicle hears vehicles of the other parity only."""
    rng = np.random.default_rng(seed)
    x = PF.draw_states(rng, Bf)
    x[:, 0:2] = rng.uniform(-0.01, 0.01, (Bf, 2))
    x[1::2, 0] += 0.875
    idx = np.empty((Bf, K), dtype=np.int32)
    for v in range(Bf):
        opp = [w for w in range(Bf) if w % 2 != v % 2]
        idx[v] = [opp[(v // 2 + k) % len(opp)] for k in range(K)]
    return x, idx


# ---------------------------------------------------------------- c. the K-neighbour prediction on windows
MULTI_SHAPE, MULTI_N, MULTI_R = (64, 3), 20, 0.75
_multi = {}


def multi_case(blob):
    """mlp_multi_deriv_ref.own_row_case with mixed gates drawn around the radius 0.75."""
    if "c" not in _multi:
        Bm, K = MULTI_SHAPE
        _multi["c"] = MM.own_row_case(7500 + 10 * Bm + K, blob, Bm, K, MULTI_N, "mixed", r_h=MULTI_R)
    return _multi["c"]


# ---------------------------------------------------------------- d. the formation rollouts
FORM_CASE = dict(mass=0.9, g=7.0, r_horiz=0.75)
FORM_TICKS, FORM_OFFSET, FORM_START_SEED, FORM_START_SIGMA = 12, 0.875, 7600, 0.01


def form_cfg(oracle, case=FORM_CASE):
    return oracle_cfg(oracle, case)


def _offset(tr, groups, offset):
    """Vehicle m of every group of `groups` flies m * offset further along x (every segment's constant coefficient and final_pt)."""
    for m in range(1, groups):
        tr["coeff_x"][m::groups, 0::8] += m * offset
        tr["final_pt"][m::groups, 0] += m * offset
    return tr


def offset_workload(multi=False, offset=FORM_OFFSET):
    """formation_ref.workload's two stacked pairs (multi: formation_multi_ref.workload's two stacked triples), every upper vehicle's path
    moved `offset` sideways: between 0.75 and 1.0 from its neighbour, so the gate is closed at 0.75 and open at 1.0."""
    return _offset(FM.workload(2), 3, offset) if multi else _offset(FR.workload(2), 2, offset)


def form_start(xr0):
    """The start state: node 0 of the first window, positions moved by a seeded N(0, 1 cm) -- a transient for the model to shape."""
    x = xr0[:, 0].copy()
    x[:, 0:3] += np.random.default_rng(FORM_START_SEED).normal(0.0, FORM_START_SIGMA, (x.shape[0], 3))
    return x


def form_reference(blob, cfg, r_horiz, multi, compensate, x_init=None):
    """The CPU loop over FORM_TICKS ticks of the offset workload at cfg and r_horiz from form_start: (tr, x_init, (states, u0, force,
    status)).  x_init: the start state to use instead (the default twins start where the case starts: the same inputs)."""
    tr = offset_workload(multi)
    xr, ur = FR.windows(tr, FORM_TICKS, cfg=cfg)
    x0 = form_start(xr[0]) if x_init is None else x_init
    if multi:
        out = FM.cpu_rollout(blob, tr, xr, ur, "all" if compensate else "blind", ticks=FORM_TICKS, cfg=cfg, r_horiz=r_horiz, x_init=x0)
    else:
        out = FR.cpu_rollout(blob, tr, xr, ur, compensate, ticks=FORM_TICKS, cfg=cfg, r_horiz=r_horiz, x_init=x0)
    return tr, x0, out


def gate_distances(states, x_init, idx):
    """d^2 [ticks, B, K] of every slot at the state every tick's force is evaluated at (the start, then the logged states but the last)."""
    idx = idx.reshape(idx.shape[0], -1)
    xs = np.concatenate([x_init[None], states[:-1]])
    d = xs[:, idx, 0:2] - xs[:, :, None, 0:2]
    return (d * d).sum(-1)


# ---------------------------------------------------------------- e. the one-call closed loop and its reverse
LOOP_K, LOOP_HORIZONS, LOOP_UPS_SEED = 3, (20, 7), 31
LOOP_SEED_BASE = 20231516     # closed_loop_chain_ref.ext_inputs' seed of the default-model tests
# (the base seed itself meets loop_conditions at LOOP_CASE at both horizons -- tests/test_plant_side_envelope.py runs them -- so there is
# no table of later seeds)
LOOP_DT_RUN = dict(N=20, K=2, dt=0.05, substeps=3)       # the run with h = dt / 3: no power of two
EDGE_HORIZONS, EDGE_K, EDGE_SEED = (2, 27, 28, 40), 2, 20231516
_loop = {}


def loop_cfg(oracle, N):
    """LOOP_CASE as an OrcCfg of horizon N with the force on."""
    return oracle_cfg(oracle, LOOP_CASE, N=N, use_fd=True)


def loop_seed(N):
    return LOOP_SEED_BASE


def loop_inputs(N, seed=None, K=LOOP_K):
    return R.ext_inputs(B, K, N, loop_seed(N) if seed is None else seed)


def loop_record(oracle, N, seed=None):
    """(inputs, the oracle's record at LOOP_CASE, its set finishes, the referenced six, the upstreams): once per (N, seed)."""
    seed = loop_seed(N) if seed is None else seed
    if (N, seed) not in _loop:
        a = loop_inputs(N, seed)
        rec = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], f=a["f"], cfg=loop_cfg(oracle, N))
        ok = R.set_finish(rec)
        _loop[N, seed] = (a, rec, ok, _pick(rec, ok), R.upstreams(LOOP_K, B, N, seed=LOOP_UPS_SEED))
    return _loop[N, seed]


def loop_conditions(oracle, N, seed=None):
    """On the oracle alone: (six referenced set finishes, one of them with a stage-0 input pinned in one tick and free in a later one;
    the vehicles that are no set finishes; the vehicles that keep their sets and iteration words under the finite-difference
    perturbations of Qd[0], Rd[3] and the mass)."""
    a, rec, ok, which, (G, H, A) = loop_record(oracle, N, seed)
    pin0 = rec["act"][:, :, 0, :].any(axis=2)
    six = len(which) == 6 and bool(ok[which].all()) and any(pin0[k, v] and (~pin0[k + 1:, v]).any() for v in which for k in range(LOOP_K - 1))
    stable = ok.copy()
    for col in (0, 13, 14):
        stable &= M.model_fd(oracle, rec, G, H, A, col, cfg=loop_cfg(oracle, N))[1]
    return six, int((~ok).sum()), stable


def loop_meets(oracle, N, seed=None):
    six, n_bad, stable = loop_conditions(oracle, N, seed)
    return six and n_bad <= B // 4 and int(stable.sum()) >= 40


# ---------------------------------------------------------------- the comparisons' own measures (device tests and their default twins)
def force_reference(blob, c, r, gate=True, scale=1.0, T=2):
    """The float64 reference of group b on a shared-state case at radius r, with the seeded upstream and directions the device test
    uses: dict gf, tx, tw and rz (g_z), rw (g_w), rd [T] (df), rf (the force), open."""
    from ndp_nmpc_qd_amd import mlp_frag
    x, idx = c["x"], c["index"]
    Bf, K = idx.shape
    rng = np.random.default_rng(3 * Bf + K)
    gf, tx = rng.normal(size=(Bf, 3)), rng.normal(size=(Bf, T, 10))
    tw = (np.asarray(blob, dtype=np.float64)[None] * 0.1 * rng.normal(size=(T, mlp_frag.NPARAM))).astype(np.float32)
    tw[0] = 0.0
    rz, _, rw, margin = PF.vjp64(blob, x, idx, gf, gate, scale, r2=r * r)
    return dict(gf=gf, tx=tx, tw=tw, rz=rz, rw=rw, margin=margin, rd=[PF.jvp64(blob, x, idx, tx[:, t], tw[t], gate, scale, r2=r * r) for t in range(T)],
                rf=PF.force64(blob, x, idx, gate, scale, r2=r * r), open=PF.gather(x, idx, gate, r * r)[1])


def _rows(a, b, axis):
    return float((np.abs(a - b).max(axis=axis) / np.maximum(1.0, np.abs(b).max(axis=axis))).max())


def force_errors(gz, gw, df, f, ref):
    """tests/test_plant_force_deriv_gpu.py's measures: the worst parameter group of g_w, g_z per slot, df and f per vehicle."""
    from tests import mlp_vjp_ref as MV
    return dict(gw=max(MV.group_errors(gw, ref["rw"]).values()), gz=_rows(gz, ref["rz"], 2),
                df=max(_rows(df[:, t], ref["rd"][t], 1) for t in range(len(ref["rd"]))), f=_rows(f, ref["rf"], 1))


def multi_reference(blob, c, r, T=2):
    """Group c's reference on an own-row case with the gates taken at radius r: dict gf, tz, tw, rz, rw, rd [T], open."""
    from ndp_nmpc_qd_amd import mlp_frag
    Bm, K, np1 = c["z"].shape[:3]
    rng = np.random.default_rng(3 * Bm + K)
    gf = rng.normal(size=(Bm, np1, 3))
    tz = rng.normal(size=(Bm, T, K, np1, 6))
    tw = (np.asarray(blob, dtype=np.float64)[None] * 0.1 * rng.normal(size=(T, mlp_frag.NPARAM))).astype(np.float32)
    tw[0] = 0.0
    open_ = c["d2"] < r * r
    rz, rw, margin = MM.vjp64(blob, c["z"], open_, gf)
    return dict(gf=gf, tz=tz, tw=tw, rz=rz, rw=rw, margin=margin, rd=[MM.jvp64(blob, c["z"], open_, tz[:, t], tw[t]) for t in range(T)], open=open_)


def multi_errors(gz, gw, df, ref):
    """tests/test_downwash_multi_deriv_gpu.py's measures."""
    from tests import mlp_vjp_ref as MV
    return dict(gw=max(MV.group_errors(gw, ref["rw"]).values()), gz=_rows(gz, ref["rz"], 3),
                df=max(_rows(df[:, t], ref["rd"][t], 2) for t in range(len(ref["rd"]))))


LEAVES = ("x0", "xr", "ur", "f", "fp")


def loop_leaf_errors(g, ref):
    """closed_loop_chain_ref.rel_err per leaf; g and ref: dicts with the rows of the referenced vehicles (x0 [n,..], the others [K,n,..])."""
    return {n: R.rel_err(g[n], ref[n], 1 if n == "x0" else 2) for n in LEAVES}


def loop_model_errors(oracle, sys_, rec, ups, gm, cfg, leaf_bar, step_bar):
    """(worst |gm - ref| over its bar for columns 0..14, the same for column 15) on the referenced vehicles (gm [n,16], their rows): per
    tick the step link's bar step_bar max(1, |g|max) for columns 0..14; column 15 is linear in gfp, which is held to leaf_bar:
    leaf_bar max(1, |gfp|max) sum_k |fp_k|_1 / m at cfg's mass (tests/test_closed_loop_vjp_gpu.py's docstring)."""
    from tests.fixed_set_ref import scale
    tot, per = M.model_reverse(oracle, sys_, rec, *ups, cfg=cfg)
    _, gfp = M.sweep_upstreams(sys_, rec, *ups)
    e14 = e15 = 0.0
    for j, v in enumerate(sys_["which"]):
        bar = sum(step_bar * scale(per[k, j, :15]) for k in range(sys_["K"]))
        e14 = max(e14, float(np.abs(gm[j, :15] - tot[j, :15]).max()) / bar)
        bar15 = leaf_bar * scale(gfp[:, j]) * float(np.abs(rec["fp"][:, v]).sum()) / cfg.mass
        e15 = max(e15, abs(gm[j, 15] - tot[j, 15]) / bar15)
    return e14, e15, tot
