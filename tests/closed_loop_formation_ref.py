"""The float64 reference of the FORMATION's closed loop -- tests/closed_loop_chain_ref.py's ext form with the force on the plant made from
the vehicles' actual states at every tick -- in plain numpy, composed from that module (the step and the plant link) and
tests/plant_force_deriv_ref.py (the force's adjoint and its scatter):

    fp_k = force(x_k; w)      (u0_k, X_k) = step_k(x_k, xr_k, ur_k, f_k)      x_{k+1} = plant(x_k, u0_k, fp_k)
    L = sum_k <G_k, x_{k+1}> + <H_k, u0_k> + <A_k, X_k> + <Fu_k, fp_k>

The record of a flight has `fp` = the logged forces, so closed_loop_chain_ref.systems serves unchanged; the formation's index rides along
as rec["index"].  The same PARTIAL derivative: linearisation points, final sets and gates held fixed.  The vehicles couple through the
index, so `which` must be a union of whole components of the index graph: the inputs are formation_multi_ref.workload's stacked triples.
Also the numpy restatement of ndp_closed_loop_formation_config's reverse lists and of ndp_plant_force_scatter_device's ordered sums.
tests/test_closed_loop_formation.py holds this module to central differences; tests/test_closed_loop_formation_gpu.py holds the device to it.
Every function takes the model (an oracle cfg, as closed_loop_chain_ref.systems does), the gate's radius and the step sizes where they
enter; model_reverse is the formation's model gradient, graph_inputs a B = 130 index graph with a hub, and link_counts the count behind
a derived bar: tests/closed_loop_formation_cases.py and the two tests/test_closed_loop_formation_envelope*.py use them."""
import numpy as np

from ndp_nmpc_qd_amd.params import downwash_params as DP
from tests import closed_loop_chain_ref as R
from tests import formation_multi_ref as FM
from tests import formation_ref as FR
from tests import mlp_vjp_ref as MV
from tests import plant_force_deriv_ref as PF

K = 3
# dz: the triples' vertical spacing.  At formation_multi_ref's 0.5 the margins are too small (closed_loop_chain_ref.ndp_inputs moved to
# 0.6 for that reason).  Here a vehicle sits in four slots at three states each, and the smallest |pre-activation| of a row is ~1e-4 for
# most relative states: (dz, offsets, seed) are the best of a search over dz 0.55..0.8, three offset scales and seeds 0..59 on the oracle's
# flight, judged by tests/test_closed_loop_formation.py's conditions on all three cases (smallest open margin 2.0e-4, 2.0e-4, 1.4e-4).
DZ, SEED, POS, VEL, F_SIGMA = 0.7, 50, 0.005, 0.01, 0.1


def _around(tr, N, ticks, seed, pos, vel, cfg=None):
    """What inputs and graph_inputs share: the windows of tr at horizon N (cfg: at that model -- the flatness map reads mass and g), the
    seeded x_0 offsets and controller force, the shipped weights."""
    from ndp_nmpc_qd_amd import _lib
    from oracle import oracle as O
    if cfg is None:
        cfg = O.default_cfg(N=N)
    assert cfg.N == N
    xr, ur = FR.windows(tr, ticks, cfg=cfg)
    B = xr.shape[1]
    rng = np.random.default_rng(seed)
    x0 = xr[0][:, 0].copy()
    x0[:, 0:3] += rng.normal(0.0, pos, (B, 3))
    x0[:, 3:6] += rng.normal(0.0, vel, (B, 3))
    return dict(x0=x0, xr=np.ascontiguousarray(xr[:ticks]), ur=np.ascontiguousarray(ur[:ticks]),
                f=rng.normal(0.0, F_SIGMA, (ticks, B, N + 1, 3)).astype(np.float32), index=tr["other_index"], blob=_lib.load_weights())


def inputs(triples, N, ticks=K, seed=SEED, dz=DZ, pos=POS, vel=VEL, cfg=None, tr=None):
    """formation_multi_ref.workload's stacked triples (K = 2 slots: the two others of the triple), their windows at horizon N, x_0 the
    first window's node 0 plus a seeded offset (positions ~ N(0, pos), velocities ~ N(0, vel)), a seeded fp32 force ~ N(0, F_SIGMA) the
    controller sees, the shipped weights.  cfg: the model of the windows (None: the default's); tr: another workload of triples."""
    return _around(FM.workload(triples=triples, dz=dz) if tr is None else tr, N, ticks, seed, pos, vel, cfg)


GRAPH_B, GRAPH_SEVEN = 130, (0, 1, 63, 64, 65, 128, 129)


def graph_index(B=GRAPH_B):
    """int32 [B,3]: the seven's rows, every other row -1.  Vehicle 64 is the hub (heard through seven slots, from all three 64-lane
    workgroups), 1 is heard by none, 63 names the hub twice, 65 has a self slot, 128 a slot >= B (empty, as -1 is)."""
    idx = np.full((B, 3), -1, dtype=np.int32)
    for v, row in ((0, (64, 129, 63)), (1, (64, 0, -1)), (63, (64, 64, -1)), (64, (129, 0, -1)), (65, (64, 65, 129)),
                   (128, (64, B + 5, 0)), (129, (64, -1, 128))):
        idx[v] = row
    return idx


def graph_inputs(N, ticks=K, seed=SEED, dz=DZ, pos=POS, vel=VEL, cfg=None):
    """B = 130 (two full 64-lane workgroups and two lanes), K = 3 slots: the seven vehicles of GRAPH_SEVEN fly ONE figure-eight (vehicle
    0's), dz apart in z in that order (formation_multi_ref.workload's way of stacking a triple), and are one component of graph_index;
    the other 123 fly their own figure-eights with every slot -1.  x_0, f and the weights as `inputs`."""
    from ndp_nmpc_qd_amd import synth
    tr = synth.figure_eight_traj(GRAPH_B, seed=FM.SEED, n_seg=FR.N_SEG, t_seg=FR.T_SEG, omega_range=(0.5, 1.0))
    for m, v in enumerate(GRAPH_SEVEN[1:], start=1):
        for k in ("coeff_x", "coeff_y", "coeff_z", "coeff_yaw", "time_cum", "time_seg", "final_pt"):
            tr[k][v] = tr[k][GRAPH_SEVEN[0]]
        tr["coeff_z"][v, 0::8] += m * dz
        tr["final_pt"][v, 2] += m * dz
    tr["other_index"] = graph_index()
    return _around(tr, N, ticks, seed, pos, vel, cfg)


def force(blob, x, index, net64, gate=True, scale=1.0, r_horiz=DP.r_horiz):
    """The force on the plant [B,3] float64: the oracle's fp32 network per slot summed in float64 (what the device runs), or -- net64, for
    finite differences -- the float64 network plant_force_deriv_ref differentiates.  A slot < 0 or >= B is empty on both paths."""
    if net64:
        return PF.force64(blob, x, index, gate, scale, r_horiz ** 2)
    return FM.true_force_multi(np.asarray(blob, dtype=np.float32), x, index, gate, scale, r_horiz=r_horiz)


def nominal_cpu(oracle, a, net64=False, restart=None, blob=None, gate=True, scale=1.0, dt=R.DT, substeps=R.SUBSTEPS, cfg=None,
                r_horiz=DP.r_horiz):
    """closed_loop_chain_ref.nominal_cpu's ext form with fp_k = force(x_k): reset to (xr_0, ur_0), one warm-up step on tick 0's inputs,
    then the ticks.  a: inputs()' dict (blob: another set of weights).  restart: a record whose pre-step iterate and kept set every tick
    starts from.  cfg: the model of controller and plant (an OrcCfg of this horizon; None: the default's), r_horiz: the plant gate's radius.
    Returns the record (closed_loop_chain_ref's layout, fp = the logged forces, index = the formation's)."""
    x0, xr, ur, f, index = a["x0"], a["xr"], a["ur"], a["f"], a["index"]
    blob = a["blob"] if blob is None else blob
    ticks, B, N = xr.shape[0], x0.shape[0], xr.shape[2] - 1
    cfg = R.twin_cfg(oracle, N, cfg)
    X, U, act = xr[0].copy(), ur[0].copy(), np.zeros((B, N, 4), dtype=np.int8)
    if restart is None:
        oracle.step_batch_as(cfg, x0, xr[0], ur[0], np.asarray(f[0], dtype=np.float64), X, U, act)
    x = np.array(x0, dtype=np.float64)
    rec = {k: [] for k in ("x", "force", "Xpre", "Upre", "act_pre", "act", "u0", "X", "st", "it", "fp")}
    for k in range(ticks):
        if restart is not None:
            X, U, act = restart["Xpre"][k].copy(), restart["Upre"][k].copy(), restart["act_pre"][k].copy()
        fk, fp = np.asarray(f[k], dtype=np.float64), np.ascontiguousarray(force(blob, x, index, net64, gate, scale, r_horiz))
        rec["x"].append(x.copy()); rec["force"].append(fk); rec["Xpre"].append(X.copy()); rec["Upre"].append(U.copy())
        rec["act_pre"].append(act.copy()); rec["fp"].append(fp)
        u0, st, it, _ = oracle.step_batch_as(cfg, x, xr[k], ur[k], fk, X, U, act)
        x = oracle.plant_step(cfg, x.copy(), u0, fp, dt, substeps)
        rec["act"].append(act.copy()); rec["u0"].append(u0); rec["X"].append(X.copy()); rec["st"].append(st); rec["it"].append(it)
    rec["x"].append(x.copy())
    rec = {k: np.stack(v) for k, v in rec.items()}
    rec.update(xr=np.asarray(xr), ur=np.asarray(ur), other=None, idx=None, blob=blob, index=index)
    return rec


def loss(rec, G, H, A, Fu=None):
    """[B]: closed_loop_chain_ref.loss plus <Fu_k, fp_k> (Fu [K,B,3] or None)."""
    return R.loss(rec, G, H, A) + (0.0 if Fu is None else (Fu * rec["fp"]).sum(axis=(0, 2)))


def components(index):
    """The components of the index graph (undirected), each a sorted list of vehicles, in order of their smallest member."""
    B = index.shape[0]
    root = list(range(B))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v
    for v in range(B):
        for o in index[v]:
            if 0 <= o < B:
                root[find(v)] = find(int(o))
    out = {}
    for v in range(B):
        out.setdefault(find(v), []).append(v)
    return sorted(out.values())


def conditions(rec, which, gate=True, r_horiz=DP.r_horiz):
    """What the inputs must give at every state where the force is evaluated (rec["x"][:-1]): dict of min open margin, failing slots
    (plant_force_deriv_ref.failing: margin under MARGIN or a gate distance within 10 % of r_horiz^2), open slots per component of `which`,
    and set finishes of `which`.  r_horiz: the radius of the gate and of the rim that fails a slot."""
    index, blob, r2 = rec["index"], rec["blob"], r_horiz ** 2
    comps = [c for c in components(index) if set(c) & set(which)]
    assert all(set(c) <= set(which) for c in comps), "`which` must be a union of whole components of the index graph"
    margin, fail, open_per = np.inf, 0, []
    for x in rec["x"][:-1]:
        _, op, _ = PF.gather(x, index, gate, r2)
        m = PF.vjp64(blob, x, index, np.zeros((x.shape[0], 3)), gate, 1.0, r2)[3]
        if op[which].any():
            margin = min(margin, float(m[which][op[which]].min()))
        fail += int(PF.failing(blob, x, index, r2=r2)[which].sum())
        open_per.append([int(op[c].sum()) for c in comps])
    return dict(margin=margin, failing=fail, open_per=np.array(open_per), set_finish=R.set_finish(rec)[which])


def reverse(sys_, rec, G, H, A, Fu=None, gate=True, scale=1.0, r_horiz=DP.r_horiz, scatter=None):
    """closed_loop_chain_ref.reverse's loop with the force's adjoint (plant_force_deriv_ref.vjp64) and its scatter added into gx_next:
    the gradient of sum over `which` of L in every leaf.  G, H, A, Fu: full-batch arrays (Fu [K,B,3] the upstream of the logged force, or
    None).  Returns x0 [n,10], xr, ur, f as closed_loop_chain_ref.reverse, gF [K,n,3] the force's total
    gradient, gz [K,n,Kn,6], w [17859] and w_tick [K,17859] (w = its sum), and the sweep's own per-tick gu0 [K,n,4] = H_k + gu_p (the
    step's upstream) and gfp [K,n,3] (the plant link's, WITHOUT Fu_k): what model_reverse takes; rows in the order of `which`.  The model
    and the step sizes are sys_'s (closed_loop_chain_ref.systems(..., dt, substeps, cfg)); r_horiz: the gate's radius.  scatter: another
    (gz, index, B) -> g_x in place of plant_force_deriv_ref.scatter -- the deliberately WRONG references of the notice checks."""
    scatter = PF.scatter if scatter is None else scatter
    which, ticks, N = sys_["which"], sys_["K"], sys_["N"]
    n, B, index = len(which), rec["x"].shape[1], rec["index"]
    out = dict(xr=np.zeros((ticks, n, N + 1, 10)), ur=np.zeros((ticks, n, N, 4)), f=np.zeros((ticks, n, N + 1, 3)), gF=np.zeros((ticks, n, 3)),
               gz=np.zeros((ticks, n, index.shape[1], 6)), w=np.zeros(MV.mlp_frag.NPARAM), w_tick=np.zeros((ticks, MV.mlp_frag.NPARAM)),
               gu0=np.zeros((ticks, n, 4)), gfp=np.zeros((ticks, n, 3)))
    gx_next = np.zeros((n, 10))
    for k in reversed(range(ticks)):
        gx_p, gu_p, gfp = R.plant_link(sys_, k, G[k][which] + gx_next)
        gF = gfp if Fu is None else Fu[k][which] + gfp
        out["gu0"][k], out["gfp"][k] = H[k][which] + gu_p, gfp
        gx0, out["xr"][k], out["ur"][k], out["f"][k] = R.step_link(sys_, k, out["gu0"][k], A[k][which])
        full = np.zeros((B, 3))
        full[which] = gF
        gz, _, gw, _ = PF.vjp64(rec["blob"], rec["x"][k], index, full, gate, scale, r_horiz ** 2)
        gx_next = gx_p + gx0 + scatter(gz, index, B)[which]
        out["gF"][k], out["gz"][k] = gF, gz[which]
        out["w"] += gw
        out["w_tick"][k] = gw
    out["x0"] = gx_next
    return out


def model_reverse(oracle, sys_, rec, ref, A, cfg=None):
    """closed_loop_vjp_ref.model_reverse for the formation, on the upstreams of `ref` = reverse(...)'s own sweep (its gu0 carries the
    neighbours' adjoints through gx_f): (total [n,16], per_tick [K,n,16]).  Columns 0..14: fixed_set_ref.model_grad_ref of tick k at
    gu0_k and A_k; column 15 = -(1/m) <gfp_k, fp_k> with gfp_k the plant link's alone (Fu_k is the upstream of the force as a VALUE: the
    force does not depend on the mass).  cfg: the model (None: the default's)."""
    from tests import fixed_set_ref as F
    which, ticks, N = sys_["which"], sys_["K"], sys_["N"]
    cfg = oracle.default_cfg(N=N, use_fd=True) if cfg is None else cfg
    per = np.zeros((ticks, len(which), 16))
    for k in range(ticks):
        for j, v in enumerate(which):
            g, _ = F.model_grad_ref(oracle, cfg, rec["x"][k][v], rec["xr"][k][v], rec["ur"][k][v], rec["force"][k][v], rec["Xpre"][k][v],
                                    rec["Upre"][k][v], rec["act"][k][v], ref["gu0"][k][j], A[k][v], None)
            per[k, j, :15] = g[:15]
            per[k, j, 15] = -(ref["gfp"][k][j] @ rec["fp"][k][v]) / cfg.mass
    return per.sum(axis=0), per


def link_counts(index, open_):
    """[ticks+1, B] int: how many open network links (slot, tick) have their adjoint g_z in the upstream of x_k of vehicle v, for
    open_ [ticks,B,Kn] (plant_force_deriv_ref.gather's, per tick): the links of tick k that touch v -- its own slots and the slots that
    name it, self slots in neither -- each with what reaches its ego vehicle's x_{k+1} (g_z is linear in gF_k = Fu_k + gfp_k of the
    ego), and what reaches v's own x_{k+1}.  Row `ticks` is zero.  A leaf row of tick k (and its model-gradient share) sees counts[k+1],
    g_x0 counts[0]."""
    ticks, B, Kn = open_.shape
    S = [[frozenset() for _ in range(B)] for _ in range(ticks + 1)]
    for k in reversed(range(ticks)):
        for v in range(B):
            s = set(S[k + 1][v])
            for w in range(B):
                for j in range(Kn):
                    o = int(index[w, j])
                    if open_[k, w, j] and 0 <= o < B and o != w and v in (w, o):
                        s.add((w, j, k))
                        s |= S[k + 1][w]
            S[k][v] = frozenset(s)
    return np.array([[len(S[k][v]) for v in range(B)] for k in range(ticks + 1)])


# ---------------------------------------------------------------- the reverse lists and the ordered scatter, restated
def reverse_lists(index):
    """ndp_closed_loop_formation_config's rule: (offset int32 [B+1], edge int32 [offset[B]]); vehicle v's list edge[offset[v]:offset[v+1]]
    holds e = w K + j for every slot with index[w][j] == v, ascending; empty (o < 0 or o >= B) and self (o == w) slots are in no list."""
    B, Kn = index.shape
    lists = [[] for _ in range(B)]
    for e in range(B * Kn):
        w, o = e // Kn, int(index.reshape(-1)[e])
        if 0 <= o < B and o != w:
            lists[o].append(e)
    offset = np.zeros(B + 1, dtype=np.int32)
    offset[1:] = np.cumsum([len(x) for x in lists])
    return offset, np.array([e for x in lists for e in x], dtype=np.int32)


def scatter_lists(gz, index, keep=None):
    """plant_force_deriv_ref.scatter through the reverse lists: [v][0:6] = sum over v's list of gz[e] - sum over v's own slots that are
    neither empty nor self.  keep(v, q, e): whether entry q (edge e) of v's list is summed (None: all -- then equal to the scatter up to
    rounding; anything else is a WRONG scatter for the notice checks)."""
    B, Kn = index.shape
    offset, edge = reverse_lists(index)
    flat = np.asarray(gz, dtype=np.float64).reshape(B * Kn, 6)
    has = (index >= 0) & (index < B) & (index != np.arange(B)[:, None])
    gx = np.zeros((B, 10))
    gx[:, :6] = -(np.asarray(gz, dtype=np.float64) * has[:, :, None]).sum(axis=1)
    for v in range(B):
        for q, e in enumerate(edge[offset[v]:offset[v + 1]]):
            if keep is None or keep(v, q, int(e)):
                gx[v, :6] += flat[e]
    return gx


def scatter_ordered(gz, index):
    """ndp_plant_force_scatter_device's sums in float64, in its order: g_x [B,10]; [v][0:6] = (sum over v's list, in list order, of gz[e])
    - (sum in slot order of v's own slots that are neither empty nor self), each sum from its first term as it is (an empty one: +0),
    then one subtraction; columns 6..9 zero."""
    B, Kn = index.shape
    offset, edge = reverse_lists(index)
    flat = np.asarray(gz, dtype=np.float64).reshape(B * Kn, 6)
    gx = np.zeros((B, 10))
    for v in range(B):
        terms_in = [flat[e] for e in edge[offset[v]:offset[v + 1]]]
        terms_own = [flat[v * Kn + j] for j in range(Kn) if 0 <= index[v, j] < B and index[v, j] != v]
        s = [np.zeros(6), np.zeros(6)]
        for i, terms in enumerate((terms_in, terms_own)):
            if terms:
                acc = terms[0].copy()
                for t in terms[1:]:
                    acc = acc + t
                s[i] = acc
        gx[v, :6] = s[0] - s[1]
    return gx


def hand_index(B, Kn=3):
    """A hand-made index int32 [B,Kn] (B >= 8): vehicle 0 a hub heard by all, vehicle 1 heard by none, self slots, -1 and >= B entries,
    the same index twice in one row."""
    idx = np.full((B, Kn), -1, dtype=np.int32)
    for v in range(B):
        idx[v, 0] = 0                                  # everybody hears the hub (the hub itself: a self slot)
        idx[v, 1] = (v + 2) if v + 2 < B else 2        # a chain that never names vehicle 1
        idx[v, 2] = v if v % 3 == 0 else (-1 if v % 3 == 1 else B + v)      # self, empty, out of range
    idx[2] = (5, 5, 0)                                 # the same index twice in one row
    idx[3] = (3, 3, -1)                                # self twice and an empty slot: in no list
    idx[1, 1] = 4 if B > 4 else 0
    assert not (idx[np.arange(B) != 1] == 1).any() and not (idx[1] == 1).any()
    return idx
