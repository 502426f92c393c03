"""What tests/test_closed_loop_formation_envelope.py (CPU) and tests/test_closed_loop_formation_envelope_gpu.py (device) share: the cases
at which the formation's one-call closed loop is held to tests/closed_loop_formation_ref.py beyond the stacked triples at three ticks --
their shape, gate, scale, model, step sizes -- and each case's (dz, seed), picked by a bounded search on the oracle's flight.

A case's inputs are a test only where they meet `meets` (the conditions of tests/test_closed_loop_formation.py at the case's gate, scale,
model and step sizes); the conditions move with every one of those, so each case has its own pair.  PICK holds the first pair of the
search order (dz in DZS, then seeds 0 .. MAX_SEEDS - 1) that meets them; the CPU test runs the search again and asserts the table, so a
device test never finds out on the device that its inputs are no test."""
import numpy as np

from tests import closed_loop_chain_ref as R
from tests import closed_loop_formation_ref as C
from tests import mlp_vjp_ref as MV
from tests import model_cases as MC
from tests import plant_force_deriv_ref as PF
from tests import plant_side_cases as PS

NOTICE = PS.NOTICE           # a wrong reference differs from the right one by at least this many bars
MAX_SEEDS = 40               # a seed that meets its conditions is among the first MAX_SEEDS (plant_side_cases' convention)
DZS = (0.7, 0.8, 0.6, 0.5)   # closed_loop_formation_ref.DZ first
HUB = 64
SEVEN = list(C.GRAPH_SEVEN)
MODEL_CASE = dict(MC.LOOP_CASE, **PS.FORM_CASE)      # LOOP_CASE's cost weights and box, FORM_CASE's mass, gravity and gate radius

_D = dict(gate=True, scale=1.0, dt=R.DT, substeps=R.SUBSTEPS, model=None, r_horiz=1.0)
CASES = {
    # the graph (B = 130, N = 7): one component of seven vehicles across three workgroups, 123 isolated ones
    "graph": dict(_D, kind="graph", N=7, ticks=3),
    "graph_off": dict(_D, kind="graph", N=7, ticks=3, gate=False, scale=0.5),
    # the stacked triples (B = 6, N = 20)
    "scale": dict(_D, kind="triples", N=20, ticks=3, scale=1.7),
    "ticks4": dict(_D, kind="triples", N=20, ticks=4),
    "sub1": dict(_D, kind="triples", N=20, ticks=2, substeps=1),
    "sub16": dict(_D, kind="triples", N=20, ticks=2, substeps=16),
    "dt005": dict(_D, kind="triples", N=20, ticks=2, dt=PS.LOOP_DT_RUN["dt"], substeps=PS.LOOP_DT_RUN["substeps"]),
    # another model and gate radius on the horizontally offset triples: slots closed at 0.75 that are open at 1.0
    "model": dict(_D, kind="offset", N=20, ticks=3, model=MODEL_CASE, r_horiz=MC.radius_of(MODEL_CASE)),
}
# the prefixes of the existing flight (closed_loop_formation_ref.inputs(2, 20) at its own DZ, SEED): its conditions carry
PREFIX = {"ticks1": dict(_D, kind="triples", N=20, ticks=1), "ticks2": dict(_D, kind="triples", N=20, ticks=2)}
# name -> (dz, seed), what `search` returns (tests/test_closed_loop_formation_envelope.py asserts every entry)
PICK = {"graph": (0.7, 6), "graph_off": (0.7, 6), "scale": (0.7, 1), "ticks4": (0.7, 19), "sub1": (0.7, 1), "sub16": (0.7, 1),
        "dt005": (0.7, 1), "model": (0.7, 1)}


def case_of(name):
    return CASES[name] if name in CASES else PREFIX[name]


def cfg_of(oracle, case):
    """The case's model as an OrcCfg of its horizon with the force on (None: the default model)."""
    return None if case["model"] is None else MC.oracle_cfg(oracle, case["model"], N=case["N"], use_fd=True)


def which_of(case):
    return SEVEN if case["kind"] == "graph" else list(range(6))


def inputs_of(oracle, name, pick=None):
    """The case's inputs at `pick` = (dz, seed) (None: the table's; a prefix case: the existing flight's)."""
    case = case_of(name)
    dz, seed = (PICK.get(name, (C.DZ, C.SEED)) if pick is None else pick)
    cfg = cfg_of(oracle, case)
    if case["kind"] == "graph":
        return C.graph_inputs(case["N"], case["ticks"], seed=seed, dz=dz, cfg=cfg)
    tr = None
    if case["kind"] == "offset":
        # plant_side_cases.offset_workload moves vehicle m of a triple m * FORM_OFFSET sideways: at 0.75 every slot is closed, and a
        # component without an open slot is no test of the sweep.  Here the top vehicle alone moves FORM_OFFSET: the lower two stay
        # stacked (open at both radii), and the four slots between them and the top one are 0.875 apart -- closed at 0.75, open at 1.0
        tr = C.FM.workload(2, dz=dz)
        tr["coeff_x"][2::3, 0::8] += PS.FORM_OFFSET
        tr["final_pt"][2::3, 0] += PS.FORM_OFFSET
    a = C.inputs(2, case["N"], max(case["ticks"], C.K) if name in PREFIX else case["ticks"], seed=seed, dz=dz, cfg=cfg, tr=tr)
    return {k: (v[:case["ticks"]] if k in ("xr", "ur", "f") else v) for k, v in a.items()}


def record_of(oracle, name, a, **kw):
    case = case_of(name)
    return C.nominal_cpu(oracle, a, gate=case["gate"], scale=case["scale"], dt=case["dt"], substeps=case["substeps"],
                         cfg=cfg_of(oracle, case), r_horiz=case["r_horiz"], **kw)


def conditions_of(name, rec):
    """closed_loop_formation_ref.conditions at the case's gate and radius on a record (the oracle's or the device's), and -- the model
    case -- `band`: the slots closed at the case's radius and open at 1.0 whose distance is outside the 10 % band of BOTH radii, at
    every tick."""
    case = case_of(name)
    c = C.conditions(rec, which_of(case), gate=case["gate"], r_horiz=case["r_horiz"])
    if case["kind"] == "offset":
        r2 = case["r_horiz"] ** 2
        band, clear = [], True
        for x in rec["x"][:-1]:
            _, has, d2 = PF.gather(x, rec["index"], False)
            band.append(int((has & (d2 >= r2) & (d2 < 1.0)).sum()))
            clear = clear and not (has & (((d2 > 0.9 * r2) & (d2 < 1.1 * r2)) | ((d2 > 0.9) & (d2 < 1.1)))).any()
        c.update(band=min(band), clear=clear)
    return c


def meets(name, c):
    """Every open margin >= MARGIN, no slot fails, every component has an open slot at every tick, every referenced vehicle a status-0
    set finish; the model case: a slot closed at its radius and open at 1.0, clear of both rims.  No row is left out: the cap on rows
    left out of a comparison is zero."""
    ok = c["margin"] >= MV.MARGIN and c["failing"] == 0 and bool((c["open_per"] >= 1).all()) and bool(c["set_finish"].all())
    if "band" in c:
        ok = ok and c["band"] >= 1 and c["clear"]
    return ok


def search(oracle, name):
    """(dz, seed, candidates tried): the first pair of the search order whose oracle flight meets the case's conditions."""
    tried = 0
    for dz in DZS:
        for seed in range(MAX_SEEDS):
            tried += 1
            a = inputs_of(oracle, name, (dz, seed))
            if meets(name, conditions_of(name, record_of(oracle, name, a))):
                return dz, seed, tried
    raise AssertionError(f"{name}: none of {tried} (dz, seed) pairs meets the conditions")


def ups_of(case, n, seed=31):
    """Seeded normal upstreams (G, H, A, Fu) over the case's ticks."""
    G, H, A = R.upstreams(case["ticks"], n, case["N"], seed=seed)
    return G, H, A, np.random.default_rng(seed + 1).normal(size=(case["ticks"], n, 3))


# ---------------------------------------------------------------- the comparisons' own measures and bars (none from the code under test)
def rows_err(dev, ref, lead):
    """closed_loop_chain_ref.rel_err before its last max: per row (everything behind the first `lead` axes) the worst |dev - ref| over
    max(1, |ref|max of the row); shape ref.shape[:lead]."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    shp = ref.shape[:lead] + (-1,)
    return np.abs(dev - ref).reshape(shp).max(axis=-1) / np.maximum(1.0, np.abs(ref).reshape(shp).max(axis=-1))


def open_of(name, rec):
    """[ticks,B,Kn] bool: the slots open at every state the force is evaluated at, at the case's gate and radius."""
    case = case_of(name)
    return np.stack([PF.gather(x, rec["index"], case["gate"], case["r_horiz"] ** 2)[1] for x in rec["x"][:-1]])


def bars_of(name, rec):
    """The bars of a case's comparisons, rows in the order of which_of: dict x0 [n], tick [ticks,n] (a tick's gxr, gur, gf rows, its
    model-gradient share and its gfp), w, and links (the counts behind a derived bar, for the report).
      BAR["ext"]   what no network adjoint reaches: the last tick's rows (every row of a 1-tick run)
      BAR["ndp"]   everything else and g_w: ten times a three-tick chain's measurement
      derived      ONLY a row of the hub or of a 4-tick run may exceed BAR["ndp"]: there the bar is NET_BAR (1e-5 per fp32 network
                   link, the project's figure) times closed_loop_formation_ref.link_counts -- the open links whose adjoints enter that
                   row over the flight, counted from the index and the record's gates; g_w of a 4-tick run: all its open links."""
    from tests.test_closed_loop_chain_gpu import BAR, NET_BAR
    case, which = case_of(name), which_of(case_of(name))
    ticks, op = case["ticks"], open_of(name, rec)
    counts = C.link_counts(rec["index"], op)
    derived = np.array([ticks == 4 or (case["kind"] == "graph" and v == HUB) for v in which])

    def bar(k):            # of what the upstream of x_k reaches
        c = counts[k][which]
        return np.where(derived & (c > 0), NET_BAR * c, BAR["ndp"])
    tick = np.stack([np.full(len(which), BAR["ext"]) if k == ticks - 1 else bar(k + 1) for k in range(ticks)])
    n_links = int(op[:, which].sum())
    return dict(x0=bar(0), tick=tick, w=NET_BAR * n_links if ticks == 4 else BAR["ndp"], links=counts[:, which], n_links=n_links)


def compare(name, oracle, rec, sys_, dev, ref, A, step_bar):
    """Every comparison of a case in one place -- the device test's, and the CPU notice checks' with a deliberately wrong reference as
    `dev`.  dev: dict x0 [n,10], xr, ur, f [ticks,n,..], w [17859] or None, gmodel [n,16] or None (rows of which_of); ref:
    closed_loop_formation_ref.reverse's on rec.  Returns {group: (worst measured, worst measured / bar)} for the groups ext (last tick's
    leaves), x0, leaves (earlier ticks), w, m14, m15.  m14: per vehicle |dev - ref| over sum_k bar_k scale(per[k]), bar_k = step_bar
    where the upstream is ext-class; m15: tests/test_closed_loop_vjp_gpu.py's closed form per tick, sum_k bar_k max(1, |gfp_k|max)
    |fp_k|_1 / m with bar_k the bar that holds gfp_k (a zero bar: exact equality)."""
    from tests.fixed_set_ref import scale
    case, which = case_of(name), which_of(case_of(name))
    ticks, b = case["ticks"], bars_of(name, rec)
    out = {}

    def put(group, err, bar):
        err, bar = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(err))
        over = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
        old = out.get(group, (0.0, 0.0))
        out[group] = (max(old[0], float(err.max())), max(old[1], float(over.max())))
    put("x0", rows_err(dev["x0"], ref["x0"], 1), b["x0"])
    for leaf in ("xr", "ur", "f"):
        e = rows_err(dev[leaf], ref[leaf], 2)
        put("ext", e[-1], b["tick"][-1])
        if ticks > 1:
            put("leaves", e[:-1], b["tick"][:-1])
    if dev.get("w") is not None:
        put("w", rows_err(dev["w"], ref["w"], 0), b["w"])
    if dev.get("gmodel") is not None:
        cfg = cfg_of(oracle, case) or oracle.default_cfg(N=case["N"], use_fd=True)
        tot, per = dev["model_ref"] if "model_ref" in dev else C.model_reverse(oracle, sys_, rec, ref, A, cfg=cfg)
        gm = dev["gmodel"]
        for j, v in enumerate(which):
            kbar = [step_bar if k == ticks - 1 else b["tick"][k][j] for k in range(ticks)]
            put("m14", np.abs(gm[j, :15] - tot[j, :15]).max(), sum(kbar[k] * scale(per[k, j, :15]) for k in range(ticks)))
            put("m15", abs(gm[j, 15] - tot[j, 15]),
                sum(b["tick"][k][j] * scale(ref["gfp"][k, j]) * float(np.abs(rec["fp"][k, v]).sum()) for k in range(ticks)) / cfg.mass)
    return out
