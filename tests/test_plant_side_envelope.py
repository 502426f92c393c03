"""The plant side and the closed loop at models other than the reference's constants, CPU side: the new parameter paths of the
references (a cfg through tests/closed_loop_chain_ref.py and tests/closed_loop_vjp_ref.py, a radius through
tests/plant_force_deriv_ref.py, tests/mlp_multi_deriv_ref.py and the formation loops) held to finite differences and to duality BEFORE
the device is held to them, the conditions the inputs of tests/test_plant_side_envelope_gpu.py must meet, checked on the oracle and the
float64 references alone, and -- the point of the module -- that every device comparison NOTICES its model: the reference at the default
model or radius on the same inputs lies at least NOTICE = 100 bars from the reference at the case's, in the comparison's own measure.

Bars (all the project's own): finite differences 1e-6 of max(1, |g|) (tests/test_closed_loop_chain.py), duality of the force's
reference 1e-12 (tests/test_plant_force_deriv.py); the bars the notices are multiples of are the device module's, restated there with
their sources.  Measured notices, in bars: plant gf 1.0e12 / 4.5e11 and dxs 7.9e11 / 3.5e11 (light_lowg / m09; gx0 and gu do not
depend on the model and are asserted so), forward rows 1.8e12 / 5.8e11; force on the plant at 0.75: g_w 1.5e5, g_z 9.4e5, df 3.4e6, f
1.1e6, at 1.5: g_w 5.6e4, the others 1e5 (a whole row appearing or vanishing is 1 in the measure); windows at 0.75: g_w 7.3e4, g_z
1.8e6, df 2.5e6; formation positions 4.2e3 .. 1.2e4 (radius) and 1.9e3 .. 4.5e3 (model); closed loop, over N = 20, N = 7 and the dt = 0.05 run: leaves 8.7e9 .. 8.6e10,
model gradient 3.2e8 .. 4.5e8 (columns 0..14) and 2.7e9 .. 1.2e10 (column 15), values u0 4.0e6 .. 5.3e6, x 1.0e5 .. 3.0e5, X 8.8e5 ..
1.1e6 of VALUE_ATOL.  The references' own checks at LOOP_CASE: the reverse sweep against the oracle's
differences 6.8e-9, the model gradient 9.7e-10 (mass), both of FD_BAR."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import closed_loop_chain_ref as R
from tests import closed_loop_vjp_ref as M
from tests import model_cases as MC
from tests import plant_deriv_ref as P
from tests import plant_force_deriv_ref as PF
from tests import plant_side_cases as C

FD_BAR = 1e-6                     # tests/test_closed_loop_chain.py's and tests/test_closed_loop_vjp.py's
# the device module's bars, from where it takes them (these modules import without a GPU)
from tests.test_closed_loop_chain_gpu import BAR as _CHAIN_BAR, NET_BAR, PLANT_BAR, STEP_BAR, VALUE_ATOL  # noqa: E402
from tests.test_formation_rollout_gpu import POS_BAR  # noqa: E402

LEAF_BAR = _CHAIN_BAR["ext"]
assert (PLANT_BAR, NET_BAR, STEP_BAR) == (1e-13, 1e-5, 1e-9) and abs(POS_BAR - 2.17e-6) < 1e-12 and abs(LEAF_BAR - 1.24e-11) < 1e-17


@pytest.fixture(scope="module")
def blob():
    return _lib.load_weights()


# ---------------------------------------------------------------- the cases
def test_a_case_carries_its_radius_to_the_engine_alone(oracle):
    case = dict(C.FORM_CASE)
    kw = MC.engine_kw(case)
    assert kw == dict(mass=0.9, gravity=7.0, r_horiz=0.75) and MC.radius_of(case) == 0.75 and MC.radius_of({}) == 1.0
    cfg = MC.oracle_cfg(oracle, case)
    assert (cfg.mass, cfg.g) == (0.9, 7.0) and not hasattr(cfg, "r_horiz")
    assert float(_lib.default_cfg().r_horiz) == MC.R_HORIZ0 and _lib.default_cfg(**kw).r_horiz == 0.75
    for r in MC.RADII:
        assert r * r == float(np.float32(r * r)) and r != MC.R_HORIZ0          # the squares are exact, in either precision
    assert MC.model_of(MC.LOOP_CASE)[2:4] == (0.9, 7.0) and MC.model_of(MC.LOOP_CASE)[6] == MC.DT0
    assert {k: MC.model_of(v)[2:4] for k, v in MC.PLANT_CASES.items()} == dict(light_lowg=(0.6, 7.0), m09=(0.9, 9.81))


# ---------------------------------------------------------------- the references' new parameter paths
@pytest.fixture(scope="module")
def loop7(oracle):
    """N = 7 at LOOP_CASE: the record, the six, the upstreams, the systems and the reverse sweep at that cfg."""
    a, rec, ok, which, ups = C.loop_record(oracle, 7)
    cfg = C.loop_cfg(oracle, 7)
    sys_ = R.systems(oracle, rec, which, cfg=cfg)
    return dict(a=a, rec=rec, ok=ok, which=which, ups=ups, cfg=cfg, sys=sys_, g=R.reverse(sys_, rec, *ups))


def test_composed_reverse_sweep_at_the_loop_model_against_the_oracles_loop(oracle, loop7):
    """Two entries of every leaf at every tick: central differences of L over the oracle's closed loop AT LOOP_CASE (steps 1e-6, 2^-14
    on the float32 leaf f), every tick restarted from the recorded iterate and kept set, within FD_BAR of max(1, |g|) on the referenced
    vehicles that keep their sets in every run (at least five of the six)."""
    a, rec, which, (G, H, A), g, cfg = (loop7[k] for k in ("a", "rec", "which", "ups", "g", "cfg"))
    K, N = C.LOOP_K, 7
    row = {v: j for j, v in enumerate(which)}
    rng = np.random.default_rng(9)
    entries = []
    for name, k in [("x0", None)] + [(n, k) for k in range(K) for n in ("xr", "ur", "fp", "f")]:
        base = a[name] if k is None else a[name][k]
        for _ in range(2):
            at = tuple(int(rng.integers(0, s)) for s in base.shape[1:])
            entries.append((name, k, (1,) + at[1:] if name == "xr" and at[0] == 0 else at))
    stable, worst = loop7["ok"].copy(), 0.0
    fds = []
    for name, k, at in entries:
        h = 2.0 ** -14 if name == "f" else 1e-6
        L = []
        for sgn in (1.0, -1.0):
            p = {n: np.array(a[n], dtype=np.float64) for n in ("x0", "xr", "ur", "fp", "f")}
            (p[name] if k is None else p[name][k])[(slice(None),) + at] += sgn * h
            r = R.nominal_cpu(oracle, p["x0"], p["xr"], p["ur"], p["fp"], f=p["f"], restart=rec, cfg=cfg)
            stable &= R.set_finish(r) & (r["act"] == rec["act"]).all(axis=(0, 2, 3))
            L.append(R.loss(r, G, H, A))
        fds.append((L[0] - L[1]) / (2 * h))
    vs = [v for v in which if stable[v]]
    assert len(vs) >= 5, vs
    for (name, k, at), fd in zip(entries, fds):
        got = g[name] if k is None else g[name][k]
        ref = np.array([got[(row[v],) + at] for v in vs])
        err = float((np.abs(fd[vs] - ref) / np.maximum(1.0, np.abs(ref))).max())
        worst = max(worst, err)
        assert err <= FD_BAR, (name, k, at, err)
    print(f"{len(entries)} entries on {len(vs)} vehicles, worst |fd - g| / max(1, |g|) = {worst:.2e}")


def test_model_gradient_at_the_loop_model_against_the_oracles_loop(oracle, loop7):
    """model_reverse(cfg) against model_fd around THAT model's values in Qd[0], Rd[3] and the mass (column 14 + column 15: one handle has
    one mass), within FD_BAR of max(1, |g|) on the six, all of which keep their sets."""
    rec, which, (G, H, A), cfg = (loop7[k] for k in ("rec", "which", "ups", "cfg"))
    tot, _ = M.model_reverse(oracle, loop7["sys"], rec, G, H, A, cfg=cfg)
    assert not tot[:, 6].any() and np.abs(tot[:, 15]).max() > 1e-3
    for col, got in ((0, tot[:, 0]), (13, tot[:, 13]), (14, tot[:, 14] + tot[:, 15])):
        fd, stable = M.model_fd(oracle, rec, G, H, A, col, cfg=cfg)
        assert stable[which].all(), (col, stable[which])
        err = np.abs(fd[which] - got) / np.maximum(1.0, np.abs(got))
        print(f"column {col}: worst |fd - g| / max(1, |g|) = {err.max():.2e}, |g|max {np.abs(got).max():.2e}")
        assert err.max() <= FD_BAR and np.abs(got).max() > 1e-6, (col, err)
    # the perturbation is around the given model: at the default model's mass the same difference is another number
    fd_def, _ = M.model_fd(oracle, rec, G, H, A, 14)
    assert np.abs(fd_def[which] - (tot[:, 14] + tot[:, 15])).max() > 1e-3


@pytest.mark.parametrize("r", MC.RADII)
def test_force_reference_modes_are_dual_at_both_radii(blob, r):
    """<gf, df> = <g_x, tx> + <g_w, tw> with the gate at r, to 1e-12 (tests/test_plant_force_deriv.py's tolerance); force64's gate is
    vjp64's: a closed slot has no g_z."""
    c = C.force_case(blob, 7, 3, r)
    x, idx = c["x"], c["index"]
    rng = np.random.default_rng(6)
    gf, tx = rng.normal(size=(x.shape[0], 3)), rng.normal(size=x.shape)
    tw = np.asarray(blob, dtype=np.float64) * 0.1 * rng.normal(size=mlp_frag.NPARAM)
    for scale in (1.0, 0.7):
        gz, gx, gw, _ = PF.vjp64(blob, x, idx, gf, True, scale, r2=r * r)
        df = PF.jvp64(blob, x, idx, tx, tw, True, scale, r2=r * r)
        lhs, rhs = float((gf * df).sum()), float((gx * tx).sum() + (gw * tw).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)
        op = PF.gather(x, idx, True, r * r)[1]
        assert not gz[~op].any() and np.abs(gz[op]).max(axis=1).min() > 0
        f1 = PF.force64(blob, x, idx, True, scale, r2=r * r)
        assert not f1[~op.any(axis=1)].any() and np.abs(f1[op.any(axis=1)]).max(axis=1).min() > 0


# ---------------------------------------------------------------- the conditions on the inputs
@pytest.mark.parametrize("N", C.LOOP_HORIZONS)
def test_closed_loop_inputs_meet_their_conditions_on_the_oracle(oracle, N):
    """Six referenced set finishes, one with a stage-0 input pinned in one tick and free later; at most B // 4 vehicles that are no set
    finishes; at least 40 of the 65 stable under the finite-difference perturbations.  The seed is LOOP_SEED_BASE itself, the first of
    the MAX_SEEDS a search would have tried."""
    seed = C.loop_seed(N)
    assert seed == C.LOOP_SEED_BASE and C.MAX_SEEDS == 20 and C.loop_meets(oracle, N)
    six, n_bad, stable = C.loop_conditions(oracle, N)
    print(f"N={N}: seed {seed}, referenced {C.loop_record(oracle, N)[3]}, {n_bad} no set finishes, {int(stable.sum())} of {C.B} stable")
    assert six and n_bad <= C.B // 4 and stable.sum() >= 40


@pytest.mark.parametrize("r", MC.RADII)
@pytest.mark.parametrize("Bf,K", C.FORCE_SHAPES)
def test_force_redraw_loop_terminates_and_the_radius_moves_a_tenth_of_the_gates(blob, Bf, K, r):
    seed, base = C.force_seed(Bf, K, r), C.force_seed_base(Bf, K, r)
    assert 0 <= seed - base < C.MAX_SEEDS == 20
    for s in range(base, seed):                                                  # the seed is the FIRST that meets the conditions
        assert not C.force_meets(C.force_case(blob, Bf, K, r, seed=s), r), s
    c = C.force_case(blob, Bf, K, r)
    share, clear, both = C.force_conditions(c, r)
    print(f"B = {Bf} K = {K} r = {r}: seed {seed}, {c['rounds']} rounds, {c['redrawn']} states redrawn, {share:.3f} of the occupied slots differ from r = 1")
    assert c["rounds"] <= PF.MAX_ROUNDS and not PF.failing(blob, c["x"], c["index"], r2=r * r).any()
    assert share >= 0.1 and clear and both


def test_ring_case_lies_between_the_radii():
    x, idx = C.ring_case(3)
    _, has, d2 = PF.gather(x, idx, False)
    assert has.all() and d2.min() > 1.1 * 0.5625 and d2.max() < 0.9 and not (idx == np.arange(7)[:, None]).any()


@pytest.mark.parametrize("multi", [False, True])
def test_formation_workload_stays_between_the_radii(oracle, blob, multi):
    """The upper vehicles' paths are offset by FORM_OFFSET in (0.75, 1): on the oracle's rollout at FORM_CASE no slot's gate distance comes
    within 10 % of 0.75^2 (nor of 1, the default twin's), every adjacent slot lies between the two, and every status is 0."""
    assert 0.75 < C.FORM_OFFSET < 1.0
    for comp in (True, False):
        tr, x0, (states, _, force, st) = C.form_reference(blob, C.form_cfg(oracle), 0.75, multi, comp)
        d2 = C.gate_distances(states, x0, tr["other_index"])
        assert d2.shape[0] == C.FORM_TICKS and not st.any() and not force.any()
        for r2 in (0.5625, 1.0):
            assert not ((d2 > 0.9 * r2) & (d2 < 1.1 * r2)).any(), (r2, d2.min(), d2.max())
        near = d2[:, :, 0] if not multi else d2.min(axis=2)
        assert (near > 0.5625).all() and (near < 1.0).all()


# ---------------------------------------------------------------- the cases notice
def _notice(name, err, bar):
    print(f"{name}: the default twin lies {err / bar:.3g} bars away")
    assert err >= C.NOTICE * bar, (name, err, bar)


@pytest.mark.parametrize("sub", C.PLANT_SUBSTEPS)
@pytest.mark.parametrize("name", sorted(MC.PLANT_CASES))
def test_plant_cases_notice_their_model(name, sub):
    """gf and the tangent of the states differ from the default model's by more than 100 plant bars; the forward rows too.  gx0 and gu
    do NOT depend on mass or g (the acceleration enters the dynamics additively): asserted, so that nobody reads their passing as a
    check of the model -- the model reaches the plant's derivatives through gf and tf alone, and the forward rows."""
    r = C.plant_reference(name, sub)
    J0 = P.jacobian(r["x0"], r["u"], r["f"], C.DT, sub)
    here, there = P.vjp(r["J"], r["gxs"]), P.vjp(J0, r["gxs"])
    for n, a, b in zip(("gx0", "gu"), here[:2], there[:2]):
        assert P.within_bar(a, b)[0], n
    _notice(f"{name} substeps {sub} gf", P.within_bar(there[2], here[2])[1], PLANT_BAR)
    _notice(f"{name} substeps {sub} dxs", P.within_bar(P.jvp(J0, r["tx0"], r["tu"], r["tf"]), P.jvp(r["J"], r["tx0"], r["tu"], r["tf"]))[1], PLANT_BAR)
    xs = P.rollout(r["x0"], r["u"], r["f"], C.DT, sub, r["mass"], r["g"])
    _notice(f"{name} substeps {sub} forward rows", P.within_bar(P.rollout(r["x0"], r["u"], r["f"], C.DT, sub), xs)[1], PLANT_BAR)
    # mass and g are noticed one by one: m09 keeps g, and light_lowg's g moves the rows beyond what its mass does
    if name == "light_lowg":
        only_mass = P.rollout(r["x0"], r["u"], r["f"], C.DT, sub, r["mass"], MC.G0)
        _notice(f"{name} substeps {sub} forward rows, g alone", P.within_bar(only_mass, xs)[1], PLANT_BAR)


@pytest.mark.parametrize("r", MC.RADII)
@pytest.mark.parametrize("Bf,K", C.FORCE_SHAPES)
def test_force_cases_notice_their_radius(blob, Bf, K, r):
    c = C.force_case(blob, Bf, K, r)
    here, there = C.force_reference(blob, c, r), C.force_reference(blob, c, MC.R_HORIZ0)
    e = C.force_errors(there["rz"], there["rw"], np.stack(there["rd"], axis=1), there["rf"], here)
    for n, v in e.items():
        _notice(f"B = {Bf} K = {K} r = {r} {n}", v, NET_BAR)


def test_window_case_notices_its_radius(blob):
    c = C.multi_case(blob)
    here, there = C.multi_reference(blob, c, C.MULTI_R), C.multi_reference(blob, c, MC.R_HORIZ0)
    assert np.array_equal(here["open"], c["open"]) and (here["open"] != there["open"]).sum() >= 0.05 * here["open"].size
    assert here["margin"].min() >= PF.R.MARGIN
    for n, v in C.multi_errors(there["rz"], there["rw"], np.stack(there["rd"], axis=1), here).items():
        _notice(f"windows at r = {C.MULTI_R} {n}", v, NET_BAR)


@pytest.mark.parametrize("multi", [False, True])
def test_formation_cases_notice_their_radius_and_their_model(oracle, blob, multi):
    for comp in (True, False):
        _, x0, here = C.form_reference(blob, C.form_cfg(oracle), 0.75, multi, comp)
        _, _, wide = C.form_reference(blob, C.form_cfg(oracle), MC.R_HORIZ0, multi, comp, x_init=x0)
        _, _, other = C.form_reference(blob, None, 0.75, multi, comp, x_init=x0)
        dpos = lambda a, b: float(np.abs(a[0][:, :, 0:3] - b[0][:, :, 0:3]).max())  # noqa: E731
        assert np.abs(wide[2]).max() > 0.5                                       # newtons of downwash where the default radius hears
        _notice(f"formation multi {multi} compensate {comp} radius", dpos(wide, here), POS_BAR)
        _notice(f"formation multi {multi} compensate {comp} model", dpos(other, here), POS_BAR)


@pytest.mark.parametrize("which_run", list(C.LOOP_HORIZONS) + ["dt"])
def test_closed_loop_cases_notice_their_model(oracle, which_run):
    """Every closed-loop comparison of the device module has its default twin: N = 20 and N = 7 at the default plant tick, and the run
    with dt = 0.05 and 3 substeps (K = 2 at N = 20, the plant's Jacobians at that dt and substeps).  The reverse sweep and the model
    gradient with the systems built at the DEFAULT model on the same record, against those at LOOP_CASE: every leaf more than 100 leaf
    bars apart, the model gradient more than 100 of its bars (both column groups).  And the values, the one comparison of the device
    module against code that shares nothing with it: u0, x and X of the referenced six in the oracle's own loop at the default model
    on the same inputs lie more than 100 VALUE_ATOL from those at LOOP_CASE."""
    if which_run == "dt":
        run = C.LOOP_DT_RUN
        N, K, dt, sub = run["N"], run["K"], run["dt"], run["substeps"]
    else:
        N, K, dt, sub = which_run, C.LOOP_K, R.DT, R.SUBSTEPS
    a, rec, _, which, ups = C.loop_record(oracle, N)
    cfg, dflt = C.loop_cfg(oracle, N), oracle.default_cfg(N=N, use_fd=True)
    if which_run == "dt":
        a = {k: (v if k == "x0" else v[:K]) for k, v in a.items()}
        ups = tuple(u[:K] for u in ups)
        rec = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], f=a["f"], dt=dt, substeps=sub, cfg=cfg)
        assert R.set_finish(rec)[which].all()
    sys1, sys0 = (R.systems(oracle, rec, which, dt=dt, substeps=sub, cfg=c) for c in (cfg, dflt))
    for n, v in C.loop_leaf_errors(R.reverse(sys0, rec, *ups), R.reverse(sys1, rec, *ups)).items():
        _notice(f"closed loop {which_run} leaf {n}", v, LEAF_BAR)
    tot0, _ = M.model_reverse(oracle, sys0, rec, *ups, cfg=dflt)
    e14, e15, _ = C.loop_model_errors(oracle, sys1, rec, ups, tot0, cfg, LEAF_BAR, STEP_BAR)
    _notice(f"closed loop {which_run} model gradient, columns 0..14", e14, 1.0)
    _notice(f"closed loop {which_run} model gradient, column 15", e15, 1.0)
    rec0 = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], f=a["f"], dt=dt, substeps=sub)
    for n in ("u0", "x", "X"):
        _notice(f"closed loop {which_run} values {n}", float(np.abs(rec0[n][:, which] - rec[n][:, which]).max()), VALUE_ATOL)
