"""The formation's one-call closed loop and its reverse mode on the device beyond stacked triples at three ticks (run with -m gpu), with
the helpers of tests/test_closed_loop_formation_gpu.py on the cases of tests/closed_loop_formation_cases.py:

  graph      B = 130, N = 7, K = 3 slots, 3 ticks: seven coupled vehicles {0, 1, 63, 64, 65, 128, 129} across three 64-lane workgroups
             -- a hub (64) heard through seven slots, a vehicle heard by none (1), the same index twice (63), a self slot (65), a slot
             >= B (128) -- and 123 isolated vehicles; gate on at scale 1, and gate off at scale 0.5
  scale      the B = 6 triples (N = 20) at gate on, plant_scale 1.7
  ticks      1, 2 and 4 ticks at B = 6: cl_accumulate's `first` flags (1 tick: the tail rounds the single tick's g_w as it is; 2: the
             loop's first accumulation is its last; 4: a middle acc + gw)
  steps      substeps 1 and 16, and dt 0.05 with substeps 3, at 2 ticks
  model      mass 0.9, gravity 7.0, LOOP_CASE's cost weights and box, r_horiz 0.75, the top vehicle of each triple 0.875 m aside
  failed hub the graph at gate off with a NaN velocity in the hub's x_0

Every run asserts the case's conditions on the DEVICE's record before any comparison (tests/test_closed_loop_formation_envelope.py asserts
them on the oracle's and shows that a plausible wrong reference lies >= 100 bars away).  The forward is bit-equal to the host loop of
plant_force_multi_device, update_device and ndp_plant_step_device; every leaf of the referenced vehicles, g_w and d_gmodel are held to
closed_loop_formation_ref.reverse / model_reverse on the device's record; the graph's 123 isolated vehicles are bit-equal to
closed_loop_vjp_device with d_fp = zeros in gx0, gxr, gur, gf and gmodel, with column 15 exactly 0.

Bars (closed_loop_formation_cases.bars_of / compare; none from the code under test), imported from tests/test_closed_loop_chain_gpu.py:
  BAR["ext"]  what no network adjoint reaches: the last tick's gxr, gur, gf (all of them at 1 tick)
  BAR["ndp"]  everything else and g_w
  derived     only the hub's rows and the rows of the 4-tick run may exceed BAR["ndp"]: NET_BAR = 1e-5 per open network link whose
              adjoint enters the row (closed_loop_formation_ref.link_counts on the index and the record's gates): the hub's g_x0 39
              links, its tick-0 rows 24, its tick-1 rows 9; at 4 ticks g_x0 22, tick 0's rows 16, tick 1's 10, tick 2's 4, g_w 48
  d_gmodel    columns 0..14: |dev - ref| over sum_k bar_k max(1, |per-tick row|max), bar_k = STEP_BAR where the upstream is ext-class
              (the last tick, a 1-tick run), else the tick's leaf bar; column 15: sum_k bar_k max(1, |gfp_k|max) |fp_k|_1 / m with bar_k
              the bar that holds gfp_k
MEASURED on the first device run (MI355X; rel_err, in brackets the worst share of the row's bar; every test prints its figures again):
  case       gx0               last tick (ext)    earlier ticks      g_w               gmodel 0..14       column 15
  graph      4.5e-07 (0.066)   3.3e-14 (0.0027)   1.2e-07 (0.018)    2.0e-07 (0.030)   7.2e-09 (5.4e-04)  7.2e-07 (0.0077)
  graph_off  2.9e-07 (0.043)   5.4e-14 (0.0044)   2.1e-08 (0.0031)   2.0e-07 (0.031)   9.2e-10 (6.9e-05)  1.8e-07 (0.0020)
  scale      6.2e-07 (0.092)   1.1e-14 (8.5e-04)  1.5e-07 (0.022)    1.9e-07 (0.028)   4.0e-09 (3.0e-04)  2.2e-06 (0.018)
  ticks1     4.4e-07 (0.066)   1.8e-14 (0.0015)   --                 2.0e-07 (0.030)   1.2e-14 (1.2e-05)  2.8e-17 (6.0e-07)
  ticks2     4.2e-07 (0.063)   2.9e-14 (0.0024)   1.1e-07 (0.017)    2.4e-07 (0.036)   6.5e-09 (9.6e-04)  4.3e-07 (0.017)
  ticks4     9.9e-07 (0.0045)  2.3e-14 (0.0019)   1.3e-07 (0.0022)   3.3e-07 (6.9e-04) 7.4e-09 (2.5e-05)  1.8e-06 (8.1e-04)
  sub1       5.0e-07 (0.075)   3.1e-14 (0.0025)   1.2e-07 (0.018)    2.0e-07 (0.029)   2.6e-09 (3.9e-04)  5.1e-07 (0.018)
  sub16      5.0e-07 (0.075)   3.2e-14 (0.0026)   1.2e-07 (0.018)    2.0e-07 (0.029)   2.6e-09 (3.9e-04)  5.1e-07 (0.018)
  dt005      5.3e-07 (0.079)   3.5e-14 (0.0028)   1.1e-07 (0.017)    1.7e-07 (0.025)   3.2e-09 (4.7e-04)  7.2e-07 (0.014)
  model      4.4e-07 (0.066)   1.3e-14 (0.0010)   4.8e-08 (0.0072)   2.2e-07 (0.033)   4.1e-09 (3.1e-04)  5.5e-07 (0.013)
No row exceeded BAR["ndp"] = 6.7e-06 -- the hub's and the 4-tick run's included (worst: ticks4 gx0 9.9e-07) -- so the derived bars were
not needed; they stay, as the only sanctioned way past BAR["ndp"].  Worst over its bar per group: ext 0.0044, gx0 0.092, earlier ticks
0.022, g_w 0.036, gmodel 0..14 9.6e-04, column 15 0.018.  11 tests, 11 s on the device including the float64 references."""
import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import closed_loop_formation_cases as CC
from tests import closed_loop_formation_ref as C
from tests import mlp_vjp_ref as MV
from tests import model_cases as MC
from tests import test_closed_loop_formation_gpu as T
from tests.deriv_gpu import _dev, _t, ndp  # noqa: F401
from tests.test_closed_loop_chain_gpu import BAR, STEP_BAR

pytestmark = pytest.mark.gpu

VALUES = ("xs", "us", "fps", "Xs", "status")
LEAVES = ("gx0", "gxr", "gur", "gf", "gmodel")


@pytest.fixture(scope="module")
def shared():
    cache = {}
    yield cache
    for r in cache.values():
        r["eng"].close()


def _kw(case):
    return dict(gate=case["gate"], scale=case["scale"], dt=case["dt"], substeps=case["substeps"])


def full(ndp, oracle, name, cache, nan_at=None):
    """Everything a case's checks share, computed once and left unchanged: the inputs, the device's record from the host loop, one run of
    the one call and of its reverse call with every output, the conditions on the device's record (asserted HERE, before anything is
    compared) and the reference sweep on that record.  nan_at: a vehicle whose x_0 velocity is NaN (no conditions, no reference)."""
    key = (name, nan_at)
    if key in cache:
        return cache[key]
    case = CC.case_of(name)
    a = CC.inputs_of(oracle, name)
    if nan_at is not None:
        a = dict(a, x0=a["x0"].copy())
        a["x0"][nan_at, 3] = np.nan
    N, ticks, n, which = case["N"], case["ticks"], a["x0"].shape[0], CC.which_of(case)
    ekw = {} if case["model"] is None else MC.engine_kw(case["model"])
    eng = T._engine(ndp, a, N, index=None, **ekw)
    rec = T._loop(eng, a, a["index"], ticks=ticks, **_kw(case))
    after_loop = T._state(eng)
    eng.close()
    eng = T._engine(ndp, a, N, **ekw)
    if case["model"] is not None:
        assert (eng.cfg.mass, eng.cfg.gravity, eng.cfg.r_horiz) == (case["model"]["mass"], case["model"]["g"], case["r_horiz"])
    t, vals = T._forward(eng, a, N, ticks=ticks, **_kw(case))
    after_fwd = T._state(eng)
    ups = CC.ups_of(case, n)
    grads = T._reverse(eng, t, N, ups)
    r = dict(case=case, a=a, n=n, N=N, ticks=ticks, which=which, rec=rec, eng=eng, t=t, vals=vals, ups=ups, grads=grads,
             after_loop=after_loop, after_fwd=after_fwd)
    cache[key] = r
    if nan_at is None:
        c = CC.conditions_of(name, rec)
        print(f"{name}: on the device's record the smallest open margin is {c['margin']:.2e}, open slots {c['open_per'].tolist()}")
        assert CC.meets(name, c), (name, c)
        cfg = CC.cfg_of(oracle, case)
        r["sys"] = R.systems(oracle, rec, which, dt=case["dt"], substeps=case["substeps"], cfg=cfg)
        r["ref"] = C.reverse(r["sys"], rec, *ups, gate=case["gate"], scale=case["scale"], r_horiz=case["r_horiz"])
    return r


def _forward_is_the_host_loops(r):
    rec, v = r["rec"], r["vals"]
    assert np.array_equal(v["xs"], rec["x"][1:], equal_nan=True) and np.array_equal(v["us"], rec["u0"], equal_nan=True)
    assert np.array_equal(T._bits(v["fps"]), T._bits(rec["fp"]))
    assert np.array_equal(v["Xs"], rec["X"], equal_nan=True) and np.array_equal(v["status"], rec["st"])
    for x, y in zip(r["after_fwd"], r["after_loop"]):
        assert np.array_equal(x, y, equal_nan=True)
    for k in range(r["ticks"]):
        X, U, A = (T._np(s) for s in r["eng"].closed_loop_tape_slot(r["t"]["tape"], k))
        assert np.array_equal(X, rec["Xpre"][k], equal_nan=True) and np.array_equal(U, rec["Upre"][k], equal_nan=True)
        assert np.array_equal(A, rec["act_pre"][k])
    assert np.array_equal(r["grads"]["status_check"], rec["st"])


def _held_to_the_reference(oracle, name, r):
    """Every comparison of closed_loop_formation_cases.compare on the device's record: each figure printed, then each held to its bar."""
    g, which = r["grads"], r["which"]
    dev = dict(x0=g["gx0"][which], xr=g["gxr"][:, which], ur=g["gur"][:, which], f=g["gf"][:, which], w=g["gw"], gmodel=g["gmodel"][which])
    fig = CC.compare(name, oracle, r["rec"], r["sys"], dev, r["ref"], r["ups"][2], STEP_BAR)
    b = CC.bars_of(name, r["rec"])
    print(f"{name}: " + " ".join(f"{k} {v[0]:.3e} ({v[1]:.2e} of its bar)" for k, v in fig.items())
          + f"; bars x0 {b['x0'].max():.1e} leaves {b['tick'][:-1].max() if r['ticks'] > 1 else 0:.1e} w {b['w']:.1e}")
    ge = MV.group_errors(g["gw"], r["ref"]["w"])
    print(f"{name}: weights by parameter group " + " ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert np.abs(r["vals"]["fps"][:, which]).max() > 1.0 and np.abs(r["ref"]["gz"]).max() > 1e3 * BAR["ndp"]
    for k, v in fig.items():
        assert v[1] <= 1.0, (name, k, v)
    return fig


def _check(ndp, oracle, shared, name):
    r = full(ndp, oracle, name, shared)
    _forward_is_the_host_loops(r)
    return r, _held_to_the_reference(oracle, name, r)


def _isolated_equal_the_ext_form(r):
    """The header's promise: a vehicle outside every list and with no slot of its own is closed_loop_vjp_device's with d_fp = zeros,
    bit for bit, in gx0, gxr, gur, gf and gmodel; its fps and its column 15 are exactly 0."""
    import torch
    eng, t, n, N, ticks, case = r["eng"], r["t"], r["n"], r["N"], r["ticks"], r["case"]
    rest = [v for v in range(n) if v not in r["which"]]
    assert len(rest) == 123 and (r["a"]["index"][rest] == -1).all()
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=_dev())  # noqa: E731
    e = dict(gx0=z(n, 10), gxr=z(ticks, n, N + 1, 10), gur=z(ticks, n, N, 4), gf=z(ticks, n, N + 1, 3), gmodel=z(n, 16))
    ups = [_t(u) for u in r["ups"][:3]]
    torch.cuda.synchronize()
    eng.closed_loop_vjp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["tape"], f=t["f"],
                               fp=torch.zeros(ticks, n, 3, dtype=torch.float64, device=_dev()), gxs=ups[0], gus=ups[1], gXs=ups[2],
                               dt=case["dt"], substeps=case["substeps"], **e)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(T._bits(r["vals"]["fps"][:, rest]), np.zeros((ticks, len(rest), 3), dtype=np.int64))
    for k, want in e.items():
        got, want = r["grads"][k], T._np(want)
        got, want = (got[rest], want[rest]) if k in ("gx0", "gmodel") else (got[:, rest], want[:, rest])
        assert np.isfinite(want).all() and np.array_equal(T._bits(got), T._bits(want)), k
    assert (r["grads"]["gmodel"][rest, 15] == 0).all()


# ---- 1. the graph at gate on, scale 1
def test_graph_hub_across_workgroups_self_duplicate_and_out_of_range_slots(ndp, oracle, shared):
    """The graph case: forward bit-equal to the host loop; all leaves of the seven (the vehicle heard by none and the one with a self
    slot among them), g_w at B = 130 and d_gmodel (column 15 formed before gfps[k] is added) held to the reference; the 123 isolated
    vehicles bit-equal to the ext form."""
    r, _ = _check(ndp, oracle, shared, "graph")
    _isolated_equal_the_ext_form(r)
    assert (r["vals"]["status"] == 0)[:, r["which"]].all()


# ---- 2. gate and scale
def test_graph_at_gate_off_and_half_scale(ndp, oracle, shared):
    """The graph case at gate off, plant_scale 0.5: the comparisons of test 1 (a reverse sweep that dropped the scale is 1e4 bars away)."""
    r, _ = _check(ndp, oracle, shared, "graph_off")
    _isolated_equal_the_ext_form(r)


def test_triples_at_a_scale_above_one(ndp, oracle, shared):
    """The B = 6 triples at gate on, plant_scale 1.7, at the seed the search found for that scale."""
    _check(ndp, oracle, shared, "scale")


# ---- 3. ticks
@pytest.mark.parametrize("name", ["ticks1", "ticks2", "ticks4"])
def test_one_two_and_four_ticks(ndp, oracle, shared, name):
    """cl_accumulate's `first` flags away from 3 ticks.  1 and 2 ticks are prefixes of the existing flight; 4 has its own seed.  At 1 tick
    no network adjoint reaches gxr, gur, gf or d_gmodel (held to the ext-class bars), and g_w is the single tick's fp32 g_w: bit-equal
    to plant_force_multi_vjp_device on gF_0 = gfps[0] + gfp_0, gfp_0 taken from closed_loop_vjp_device on the same flight."""
    import torch
    r, fig = _check(ndp, oracle, shared, name)
    # a second reverse call on the same engine finds the fp64 accumulator as the first one left it, not as hipMalloc did: a sum that
    # began from a stale accumulator would pass once on fresh (zero) memory and differ here
    again = T._reverse(r["eng"], r["t"], r["N"], r["ups"])
    for k in T.OUTS:
        assert np.array_equal(T._bits(again[k]), T._bits(r["grads"][k])), k
    if name != "ticks1":
        return
    assert "leaves" not in fig
    eng, t, n, N = r["eng"], r["t"], r["n"], r["N"]
    gfp = torch.full((1, n, 3), -7.0, dtype=torch.float64, device=_dev())
    torch.cuda.synchronize()
    eng.closed_loop_vjp_device(t["x0"], t["xr"], t["ur"], t["xs"], t["us"], t["tape"], f=t["f"], fp=t["fps"], gxs=_t(r["ups"][0]),
                               gus=_t(r["ups"][1]), gXs=_t(r["ups"][2]), gfp=gfp)
    eng.synchronize()
    gF = _t(r["ups"][3][0] + T._np(gfp)[0])
    gw = torch.full((MV.mlp_frag.NPARAM,), -7.0, dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    eng.plant_force_multi_vjp_device(t["x0"], _t(np.ascontiguousarray(r["a"]["index"], dtype=np.int32)), gF, gw=gw, gate=True, scale=1.0)
    eng.synchronize()
    torch.cuda.synchronize()
    assert np.abs(T._np(gw)).max() > 0 and np.array_equal(T._bits(r["grads"]["gw"]), T._bits(T._np(gw)))


# ---- 4. substeps and dt
@pytest.mark.parametrize("name", ["sub1", "sub16", "dt005"])
def test_other_substeps_and_dt(ndp, oracle, shared, name):
    """substeps 1 and 16, and dt 0.05 with substeps 3 (h = dt / 3: no power of two), at 2 ticks: values bit-equal to the host loop at the
    same step sizes; leaves, g_w and d_gmodel held to the reference with the plant's Jacobians at those step sizes."""
    _check(ndp, oracle, shared, name)


# ---- 5. another model and gate radius
def test_another_model_and_gate_radius(ndp, oracle, shared):
    """Mass 0.9, gravity 7.0, LOOP_CASE's cost weights and box, r_horiz 0.75 on triples whose top vehicle flies 0.875 m aside: on the
    device's record at least one slot per tick is closed at 0.75 and open at 1.0, clear of both rims; the comparisons of test 1 (the
    references at the default radius and at the default model are >= 1e4 bars away)."""
    r, _ = _check(ndp, oracle, shared, "model")
    c = CC.conditions_of("model", r["rec"])
    assert c["band"] >= 1 and c["clear"]
    top = [2, 5]
    assert (r["vals"]["fps"][:, top] == 0).all() and (r["grads"]["gmodel"][top, 15] == 0).all()


# ---- 6. a failed hub
def test_a_failed_hub_takes_the_seven_and_nobody_else(ndp, oracle, shared):
    """The graph at gate off with a NaN velocity in the hub's x_0 (the suite's NaN-input pattern): the hub's status words are nonzero and
    d_status_check tells; every one of the seven hears the hub, so every member's d_gx0 holds a NaN; d_gw is finite; the 123 isolated
    vehicles' values and gradients are the clean run's, bit for bit."""
    clean = full(ndp, oracle, "graph_off", shared)
    r = full(ndp, oracle, "graph_off", shared, nan_at=CC.HUB)
    v, g, seven = r["vals"], r["grads"], r["which"]
    rest = [w for w in range(r["n"]) if w not in seven]
    assert (v["status"][:, CC.HUB] != 0).all() and np.array_equal(g["status_check"], v["status"])
    assert np.isnan(g["gx0"][CC.HUB]).all() and np.isnan(g["gx0"][seven]).any(axis=1).all()
    assert np.isfinite(g["gw"]).all()
    for k in VALUES:
        assert np.array_equal(v[k][:, rest], clean["vals"][k][:, rest]), k
    for k in LEAVES:
        a, b = (g[k][rest], clean["grads"][k][rest]) if k in ("gx0", "gmodel") else (g[k][:, rest], clean["grads"][k][:, rest])
        assert np.isfinite(b).all() and np.array_equal(T._bits(a), T._bits(b)), k
