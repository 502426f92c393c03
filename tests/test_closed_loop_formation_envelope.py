"""The formation's closed loop beyond stacked triples at three ticks, without a GPU: the cases of tests/closed_loop_formation_cases.py
(a graph with a hub across three workgroups, a vehicle heard by none, self, duplicate and >= B slots; gate off and plant_scale != 1;
1, 2 and 4 ticks; other substeps and dt; another model and gate radius) meet their conditions on the oracle's flight at the (dz, seed)
the bounded search finds; the reference sweep with its new parameters and closed_loop_formation_ref.model_reverse against central
differences on the graph; the reverse lists of the graph's index; and, for every comparison the device test makes, a plausible WRONG
reference lies at least NOTICE = 100 bars from the right one, so that a device that computed it would be seen.
The device side: tests/test_closed_loop_formation_envelope_gpu.py."""
import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import closed_loop_formation_cases as CC
from tests import closed_loop_formation_ref as C
from tests import fixed_set_ref as F
from tests import mlp_vjp_ref as MV
from tests.test_closed_loop_chain_gpu import BAR, STEP_BAR  # (imports without a GPU, as tests/plant_side_cases.py takes _pick)
from tests.test_closed_loop_formation import FD_BAR, H32, H64

_cache = {}


def reference(oracle, name):
    """A case's inputs, oracle record, systems, upstreams and reference sweep: computed once per session, shared, never written."""
    if name not in _cache:
        case = CC.case_of(name)
        a = CC.inputs_of(oracle, name)
        rec = CC.record_of(oracle, name, a)
        which, cfg = CC.which_of(case), CC.cfg_of(oracle, case)
        sys_ = R.systems(oracle, rec, which, dt=case["dt"], substeps=case["substeps"], cfg=cfg)
        ups = CC.ups_of(case, a["x0"].shape[0])
        ref = C.reverse(sys_, rec, *ups, gate=case["gate"], scale=case["scale"], r_horiz=case["r_horiz"])
        model = C.model_reverse(oracle, sys_, rec, ref, ups[2], cfg=cfg)
        _cache[name] = dict(case=case, a=a, rec=rec, which=which, cfg=cfg, sys=sys_, ups=ups, ref=ref, model=model)
    return _cache[name]


def _as_dev(ref, model=None, w=True):
    """A reference sweep in the layout `compare` takes as the device's."""
    d = dict(x0=ref["x0"], xr=ref["xr"], ur=ref["ur"], f=ref["f"], w=ref["w"] if w else None)
    if model is not None:
        d["gmodel"] = model[0]
    return d


# ---- 1. the conditions, and the table of the search
@pytest.mark.parametrize("name", list(CC.CASES) + list(CC.PREFIX))
def test_every_case_meets_its_conditions_at_the_pair_the_search_finds(oracle, name):
    """The conditions of test_the_inputs_meet_their_conditions_on_the_oracle on the oracle's flight at the case's gate, scale, model and
    step sizes: every open margin >= mlp_vjp_ref.MARGIN, no failing slot, an open slot per component at every tick, every referenced
    vehicle a status-0 set finish; nothing is left out of a comparison (the cap is zero).  The case's (dz, seed) is the first pair the
    bounded search meets them at; the two prefix cases fly the existing flight."""
    case = CC.case_of(name)
    if name in CC.CASES:
        dz, seed, tried = CC.search(oracle, name)
        print(f"{name}: the search's pair is (dz {dz}, seed {seed}), candidate {tried} of at most {len(CC.DZS) * CC.MAX_SEEDS}")
        assert (dz, seed) == CC.PICK[name] and seed < CC.MAX_SEEDS
    r = reference(oracle, name)
    which = r["which"]
    assert sorted(sum((c for c in C.components(r["a"]["index"]) if set(c) & set(which)), [])) == sorted(which)
    c = CC.conditions_of(name, r["rec"])
    print(f"{name}: smallest open margin {c['margin']:.2e}, open slots per tick and component {c['open_per'].tolist()}, "
          f"largest plant force {np.abs(r['rec']['fp'][:, which]).max():.1f} N" + (f", band slots {c['band']}" if "band" in c else ""))
    assert CC.meets(name, c), c
    assert c["margin"] >= MV.MARGIN and c["failing"] == 0 and (c["open_per"] >= 1).all() and c["set_finish"].all()
    assert np.abs(r["rec"]["fp"][:, which]).max() > 1.0
    if case["kind"] == "graph":
        assert (r["rec"]["fp"][:, [v for v in range(C.GRAPH_B) if v not in which]] == 0).all()
        # the self slot is evaluated (the network at z = 0) and the >= B slot is empty
        op = CC.open_of(name, r["rec"])
        assert op[:, 65, 1].all() and not op[:, 128, 1].any()
    if case["kind"] == "offset":
        # closed at this radius, open at the default one: the default-radius flight feels another force
        op, op1 = CC.open_of(name, r["rec"]), np.stack([C.PF.gather(x, r["rec"]["index"], True, 1.0)[1] for x in r["rec"]["x"][:-1]])
        assert (op1 & ~op).any(axis=(1, 2)).all() and c["band"] >= 1 and c["clear"]


def test_the_o_ge_B_slot_is_empty_on_the_fp32_force_path(oracle):
    """formation_ref.true_force takes the device's full index rule: a slot >= B is empty, as -1 is -- the fp32 force with the slot in
    place equals the force with -1 there, bit for bit, gate on and off."""
    r = reference(oracle, "graph")
    idx = r["a"]["index"].copy()
    assert idx[128, 1] == C.GRAPH_B + 5
    idx[128, 1] = -1
    x = r["rec"]["x"][1]
    for gate in (True, False):
        f0, f1 = C.force(r["a"]["blob"], x, r["a"]["index"], False, gate), C.force(r["a"]["blob"], x, idx, False, gate)
        assert np.array_equal(f0, f1) and np.abs(f0[128]).max() > 0
        # (and the float64 path agrees: NET_BAR per network output of max(1, |f|), three slots summed)
        assert np.abs(f0 - C.force(r["a"]["blob"], x, idx, True, gate)).max() <= 3 * C.FM.NET_BAR * max(1.0, np.abs(f0).max())


# ---- 2. the reverse lists of the graph
def test_the_reverse_lists_of_the_graph_index():
    """The hub's list is exactly the seven edges that name it, ascending, from all three 64-lane blocks; vehicles 1 and 65 are named by
    nobody else (65's self slot is in no list); the duplicate row gives two entries."""
    idx = C.graph_index()
    B, Kn = idx.shape
    offset, edge = C.reverse_lists(idx)
    lists = [edge[offset[v]:offset[v + 1]].tolist() for v in range(B)]
    hub = [0 * Kn + 0, 1 * Kn + 0, 63 * Kn + 0, 63 * Kn + 1, 65 * Kn + 0, 128 * Kn + 0, 129 * Kn + 0]
    assert lists[CC.HUB] == hub == sorted(hub) and len(hub) == 7 > Kn
    assert {e // Kn // 64 for e in hub} == {0, 1, 2}
    assert lists[1] == [] and lists[65] == [] and idx[65, 1] == 65
    assert lists[CC.HUB].count(63 * Kn) == 1 and lists[CC.HUB].count(63 * Kn + 1) == 1
    assert lists[0] == [1 * Kn + 1, 64 * Kn + 1, 128 * Kn + 2] and lists[129] == [0 * Kn + 1, 64 * Kn + 0, 65 * Kn + 2]
    assert lists[63] == [0 * Kn + 2] and lists[128] == [129 * Kn + 2]
    assert sum(len(x) for x in lists) == 15 and all(not lists[v] for v in range(B) if v not in CC.SEVEN)
    assert 128 * Kn + 1 not in edge                                  # the >= B slot is in no list
    assert C.components(idx)[0] == CC.SEVEN and len(C.components(idx)) == 1 + 123
    rng = np.random.default_rng(2)
    gz = rng.normal(size=(B, Kn, 6))
    assert np.abs(C.scatter_lists(gz, idx) - C.PF.scatter(gz, idx, B)).max() <= 1e-13
    assert np.abs(C.scatter_ordered(gz, idx) - C.PF.scatter(gz, idx, B)).max() <= 1e-13


# ---- 3. central differences on the graph, gate off, scale 0.5
def test_graph_sweep_and_model_gradient_match_central_differences(oracle):
    """The graph case at gate off, scale 0.5, L summed over the seven: central differences over the float64-network flight, every tick
    of every perturbed run restarted from the nominal record, in two entries of x_0, one each of a tick's xr, ur and f, one weight per
    parameter group, Qd[0] and the mass -- column 14 + column 15 of model_reverse against closed_loop_vjp_ref.model_fd's scheme (one
    handle has one mass: controller and plant move together) with fp_k recomputed from the perturbed flight -- within FD_BAR of
    max(1, |g|); every one of the seven keeps its sets and iteration words in every run."""
    from ndp_nmpc_qd_amd import mlp_frag
    name = "graph_off"
    case = CC.case_of(name)
    a = CC.inputs_of(oracle, name)
    blob = np.asarray(a["blob"], dtype=np.float64)
    rec = CC.record_of(oracle, name, a, net64=True, blob=blob)
    which, ticks, N = CC.SEVEN, case["ticks"], case["N"]
    c = CC.conditions_of(name, rec)
    assert c["set_finish"].all() and c["failing"] == 0
    G, H, A = R.upstreams(ticks, C.GRAPH_B, N, seed=5)
    Fu = np.random.default_rng(6).normal(size=(ticks, C.GRAPH_B, 3))
    sys_ = R.systems(oracle, rec, which)
    g = C.reverse(sys_, rec, G, H, A, Fu, gate=case["gate"], scale=case["scale"])
    tot, _ = C.model_reverse(oracle, sys_, rec, g, A)
    rng = np.random.default_rng(9)
    entries = [("x0", None, (int(rng.integers(0, 6)),)), ("x0", None, (int(rng.integers(6, 10)),))]
    for k, leaf in zip(rng.permutation(ticks), ("xr", "ur", "f")):
        at = tuple(int(rng.integers(0, s)) for s in a[leaf][k].shape[1:])
        entries.append((leaf, int(k), (1,) + at[1:] if leaf == "xr" and at[0] == 0 else at))
    entries += [("w", None, (o + int(rng.integers(0, int(np.prod(s)))),)) for o, s in mlp_frag.offsets().values()]
    entries += [("Qd", None, (0,)), ("mass", None, ())]
    base = R.twin_cfg(oracle, N)
    stable, worst = np.ones(len(which), dtype=bool), 0.0
    for leaf, k, at in entries:
        val = base.Qd[0] if leaf == "Qd" else base.mass
        h = 1e-5 * val if leaf in ("Qd", "mass") else H32 if leaf in ("f", "w") else H64
        L = []
        for sgn in (1.0, -1.0):
            p = dict(a, x0=a["x0"].copy(), xr=a["xr"].copy(), ur=a["ur"].copy(), f=a["f"].astype(np.float64))
            w, cfg = blob.copy(), F.copy_cfg(base)
            if leaf == "w":
                w[at] += sgn * h
            elif leaf == "Qd":
                cfg.Qd[0] = val + sgn * h
            elif leaf == "mass":
                cfg.mass = val + sgn * h
            else:
                (p[leaf] if k is None else p[leaf][k])[(which,) + at] += sgn * h
            r = CC.record_of(oracle, name, p, net64=True, restart=rec, blob=w) if leaf not in ("Qd", "mass") else \
                C.nominal_cpu(oracle, p, net64=True, restart=rec, blob=w, gate=case["gate"], scale=case["scale"], cfg=cfg)
            stable &= R.set_finish(r)[which] & (r["act"] == rec["act"]).all(axis=(0, 2, 3))[which]
            L.append(C.loss(r, G, H, A, Fu)[which].sum())
        fd = (L[0] - L[1]) / (2 * h)
        if leaf == "Qd":
            ref = tot[:, 0].sum()
        elif leaf == "mass":
            ref = tot[:, 14].sum() + tot[:, 15].sum()
        else:
            got = g[leaf] if k is None else g[leaf][k]
            ref = got[at] if leaf == "w" else got[(slice(None),) + at].sum()
        err = abs(fd - ref) / max(1.0, abs(ref))
        worst = max(worst, err)
        print(f"{leaf} {k} {at}: fd {fd:.9e} reference {ref:.9e} err {err:.2e}")
        assert err <= FD_BAR, (leaf, k, at, fd, ref, err)
    assert stable.all()
    assert np.abs(tot[:, 15]).max() > 1e-3 and np.abs(g["gz"]).max() > 1e-3
    print(f"{len(entries)} entries, worst |fd - g| / max(1, |g|) = {worst:.2e}")


# ---- 4. the notice checks
def _notice(tag, fig, groups):
    """Print every group's figure of a wrong reference; the groups named must lie at least NOTICE bars away."""
    print(f"{tag}: " + " ".join(f"{k} {v[0]:.2e} ({v[1]:.1e} bars)" for k, v in fig.items()))
    for k in groups:
        assert fig[k][1] >= CC.NOTICE, (tag, k, fig[k])


@pytest.mark.parametrize("name", ["graph", "graph_off"])
def test_a_wrong_gather_is_noticed_on_the_graph(oracle, name):
    """The hub's list cut to its first K entries, and the gather restricted to edges from the vehicle's own 64-lane block: each, as a
    reference on the oracle's record, differs from the right one by >= NOTICE bars in g_x0 and g_w, with the bars the device test uses
    (the hub's rows: the derived bar); the other groups' figures are printed (the model gradient's scale hides a missing edge)."""
    r = reference(oracle, name)
    case, Kn = r["case"], 3
    kw = dict(gate=case["gate"], scale=case["scale"], r_horiz=case["r_horiz"])
    wrongs = {"the hub's list cut to K entries": lambda v, q, e: q < Kn, "edges of the own 64-block only": lambda v, q, e: e // Kn // 64 == v // 64}
    for tag, keep in wrongs.items():
        bad = C.reverse(r["sys"], r["rec"], *r["ups"], scatter=lambda gz, idx, B: C.scatter_lists(gz, idx, keep), **kw)
        model = C.model_reverse(oracle, r["sys"], r["rec"], bad, r["ups"][2], cfg=r["cfg"])
        fig = CC.compare(name, oracle, r["rec"], r["sys"], _as_dev(bad, model), r["ref"], r["ups"][2], STEP_BAR)
        _notice(f"{name}, {tag}", fig, ("x0", "w"))
        assert fig["ext"][0] == 0.0
    b = CC.bars_of(name, r["rec"])
    print(f"{name}: links behind the rows of the seven, per tick {b['links'].tolist()}; all open links {b['n_links']}")


@pytest.mark.parametrize("name", ["graph_off", "scale"])
def test_a_dropped_scale_is_noticed(oracle, name):
    """The reverse sweep with `scale` taken as 1 on the record flown at the case's scale: >= NOTICE bars away in g_x0, the earlier ticks'
    leaves, g_w and d_gmodel's columns 0..14 (column 15 is linear in gfp_k of the last tick too, which the scale does not reach)."""
    r = reference(oracle, name)
    case = r["case"]
    assert case["scale"] != 1.0
    bad = C.reverse(r["sys"], r["rec"], *r["ups"], gate=case["gate"], scale=1.0, r_horiz=case["r_horiz"])
    model = C.model_reverse(oracle, r["sys"], r["rec"], bad, r["ups"][2], cfg=r["cfg"])
    fig = CC.compare(name, oracle, r["rec"], r["sys"], _as_dev(bad, model), r["ref"], r["ups"][2], STEP_BAR)
    _notice(f"{name}, scale taken as 1 instead of {case['scale']}", fig, ("x0", "leaves", "w", "m14", "m15"))


def test_the_default_radius_and_the_default_model_are_noticed(oracle):
    """The model case's record under the reference at the DEFAULT gate radius (the slots closed at 0.75 taken as open) and under the
    systems and model gradient of the DEFAULT model: each >= NOTICE bars away."""
    name = "model"
    r = reference(oracle, name)
    case = r["case"]
    bad = C.reverse(r["sys"], r["rec"], *r["ups"], gate=case["gate"], scale=case["scale"], r_horiz=1.0)
    model = C.model_reverse(oracle, r["sys"], r["rec"], bad, r["ups"][2], cfg=r["cfg"])
    fig = CC.compare(name, oracle, r["rec"], r["sys"], _as_dev(bad, model), r["ref"], r["ups"][2], STEP_BAR)
    _notice("model, the gate radius taken as 1.0", fig, ("x0", "leaves", "w", "m14", "m15"))
    sys0 = R.systems(oracle, r["rec"], r["which"])
    bad = C.reverse(sys0, r["rec"], *r["ups"], gate=case["gate"], scale=case["scale"], r_horiz=case["r_horiz"])
    model = C.model_reverse(oracle, sys0, r["rec"], bad, r["ups"][2])
    fig = CC.compare(name, oracle, r["rec"], r["sys"], _as_dev(bad, model), r["ref"], r["ups"][2], STEP_BAR)
    _notice("model, the default model's systems", fig, ("ext", "x0", "leaves", "w", "m14", "m15"))


@pytest.mark.parametrize("name", ["graph", "graph_off", "scale", "ticks4", "ticks1", "model"])
def test_fu_in_column_15_is_noticed(oracle, name):
    """Column 15 formed from gF_k = Fu_k + gfp_k instead of gfp_k: >= NOTICE of column 15's bar away."""
    r = reference(oracle, name)
    tot = r["model"][0].copy()
    for k in range(r["case"]["ticks"]):
        for j, v in enumerate(r["which"]):
            tot[j, 15] -= (r["ups"][3][k][v] @ r["rec"]["fp"][k][v]) / (r["cfg"] or oracle.default_cfg(N=r["case"]["N"])).mass
    fig = CC.compare(name, oracle, r["rec"], r["sys"], dict(_as_dev(r["ref"]), gmodel=tot, model_ref=r["model"]), r["ref"], r["ups"][2], STEP_BAR)
    _notice(f"{name}, Fu_k in column 15", fig, ("m15",))
    assert fig["m14"][0] == 0.0


@pytest.mark.parametrize("name", ["graph", "ticks2", "ticks4", "sub1"])
def test_a_tick_missing_from_the_weight_sum_is_noticed(oracle, name):
    """g_w summed without its first or its last tick's share: >= NOTICE bars of g_w's bar away (4 ticks: also without a middle one)."""
    r = reference(oracle, name)
    ticks = r["case"]["ticks"]
    assert np.abs(r["ref"]["w_tick"].sum(axis=0) - r["ref"]["w"]).max() <= 1e-12 * np.abs(r["ref"]["w"]).max()
    for k in sorted({0, ticks - 1, ticks // 2}):
        bad = dict(_as_dev(r["ref"]), w=r["ref"]["w"] - r["ref"]["w_tick"][k])
        fig = CC.compare(name, oracle, r["rec"], r["sys"], bad, r["ref"], r["ups"][2], STEP_BAR)
        _notice(f"{name}, g_w without tick {k}", fig, ("w",))


def test_the_derived_bars_are_counted_not_fitted(oracle):
    """Where BAR["ndp"] gives way: only rows of the hub and of the 4-tick run, and there NET_BAR times the links counted from the index
    and the record's gates.  The counts this file's cases give are stated here and in DESIGN section 9."""
    from tests.test_closed_loop_chain_gpu import NET_BAR
    for name in ("graph", "graph_off", "ticks4", "scale"):
        r = reference(oracle, name)
        b = CC.bars_of(name, r["rec"])
        print(f"{name}: links per tick and vehicle {b['links'].tolist()}, open links {b['n_links']}, x0 bars {b['x0'].tolist()}")
        hub = [j for j, v in enumerate(r["which"]) if r["case"]["kind"] == "graph" and v == CC.HUB]
        for j in range(len(r["which"])):
            rows = np.concatenate([b["x0"][j:j + 1], b["tick"][:-1, j]])
            if j in hub or r["case"]["ticks"] == 4:
                want = np.concatenate([b["links"][0, j:j + 1], b["links"][1:-1, j]])
                assert np.array_equal(rows, np.where(want > 0, NET_BAR * want, BAR["ndp"]))
            else:
                assert (rows == BAR["ndp"]).all()
        assert (b["tick"][-1] == BAR["ext"]).all() and (b["links"][-1] == 0).all()
    g = CC.bars_of("graph", reference(oracle, "graph")["rec"])
    # every slot of the seven is open (one figure-eight): 15 links between two vehicles and the self slot per tick.  The hub's x_0
    # hears the 9 links of tick 0 that touch it, and through their ego vehicles all 15 of tick 1 and of tick 2: 39; its x_1 24, x_2 9
    assert g["links"][:, CC.SEVEN.index(CC.HUB)].tolist() == [39, 24, 9, 0] and g["n_links"] == 3 * 16
    # a triple's vehicle at 4 ticks: the 4 links of its own tick that touch it, and all 6 of its triple at every later tick
    t4 = CC.bars_of("ticks4", reference(oracle, "ticks4")["rec"])
    assert t4["links"][:, 0].tolist() == [22, 16, 10, 4, 0] and (t4["links"] == t4["links"][:, :1]).all()
    assert t4["n_links"] == 4 * 12 and t4["w"] == NET_BAR * 48
