"""ndp_step_jvp_model_device (rti_mjvp_kernel<20> / <0>, RtiWave::jvp_out<true>) on the device where its own code paths differ (run with
-m gpu): every horizon of tests/deriv_edges.py's DERIV_EDGE_N (the chunk edges of the two parking loops rho_x -> CX over 10(N+1) entries and
rho_u -> CU over 4N, and of the per-direction reads), interior-point finishes (the in-place parking), other models, finite differences
of the device's own step in the model, and eight directions.  CPU side (the twins on the float64 reference, every seed and count this
module relies on): tests/test_step_model_jvp_edges.py.

B = deriv_edges.DEVICE_B = 37, the mixed workload with a supplied fp32 force, the seeds SEEDS[N] of tests/test_deriv_edges_gpu.py (N = 13
and 20, which that table does not have: SEED_13_20 below); every output buffer carries two guard rows.

The data twins.  With (X+, U+) the iterate after the recorded step, a model direction and the data direction beside it build ONE
right-hand side in jvp_out:
    r'  (columns 10..13)                 tur_k[i] = -(r'_i / Rd_i) (U+_k[i] - ur_k[i])
    q'_r, r < 6, where Qd_r > 0          txr_k[r] = -(q'_r / Qd_r) (X+_k[r] - xr_k[r]),  k = 0..N
    m'  (column 14), with a force        tf_k     = -(m' / m) f_k
so rti_mjvp_kernel along the left and rti_jvp_kernel (held to the dense reference at all these horizons by
tests/test_deriv_edges_gpu.py) along the right give the same tangent -- also where there is no dense reference, after an interior-point
finish.

Bars.  The dense reference: 1e-9 of max(1, |z'|max) (tests/test_step_model_jvp_gpu.py's).  Duality with ndp_step_vjp_model_device: 1e-10
of the largest term on set finishes, 1e-6 on interior-point finishes.  The twins: 1e-10 of max(1, |z'|max) on set finishes (the project's
bar for its linear identities); on interior-point finishes the two kernels recompute the step separately (allowed 1e-12 apart) and the
last Newton system may amplify that, so the bar is max(1e-10, 10 x floor), the floor measured on rti_jvp_kernel ALONE: the data twins
built from (X+, U+) against those built from (X+, U+) with every entry multiplied by 1 + 1e-12 xi (xi = a seeded +-1), worst over the
status-0 instances; a bar above 1e-6 so formed fails the test.  Finite differences: 1e-6 of max(1, |z'|max)
(tests/test_step_model_jvp.py's bar for the same comparison on the oracle).  No bar here comes from rti_mjvp_kernel's output."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import model_jvp_ref as MR
from tests.deriv_edges import DERIV_EDGE_N, DEVICE_B, device_case, pick
from tests.deriv_gpu import MIXED, _dev, _jvp, _mjvp, _recorded_step, _t, _tangents, _tt, _vjp, ndp  # noqa: F401
from tests.fixed_set_ref import copy_cfg, scale
from tests.model_cases import CASES, DERIV_CASES, engine_kw, model_of, oracle_cfg
from tests.test_deriv_edges_gpu import IPM_DUALITY_BAR, SEEDS, SET_DUALITY_BAR, _finishes, _guards_intact
from tests.test_kernel_table_gpu import SENS_BAR, geometry

pytestmark = pytest.mark.gpu

B, T, GUARD = DEVICE_B, 2, 2
TWIN_FLOOR_FACTOR, TWIN_BAR_CEILING, TWIN_WIGGLE = 10.0, 1e-6, 1e-12

# qp_mode 1 (every instance iterates in the interior-point loop): the two sweep choices after such a finish (3, 4), the chunk edges of both
# parking loops (6, 12: 10(N+1) = 70, 130; 17: 4N = 68), the <20> kernel, and two instances per workgroup (21).  The batch seed: SEEDS[N]
# where the CPU oracle at qp_mode 1 finishes at least B // 2 of the 37 instances with status 0 over the warm-up and the recorded step, else
# the first seed from SEED0 + 5000 + 100 N on that does (N = 20 has no entry in SEEDS).  tests/test_step_model_jvp_edges.py checks every
# entry by that rule.
IPM_N = (3, 4, 6, 12, 17, 20, 21)
IPM_SEEDS = {3: SEEDS[3], 4: SEEDS[4], 6: SEEDS[6], 12: SEEDS[12], 17: SEEDS[17], 20: synth.SEED0 + 7000, 21: SEEDS[21]}

# Other models: (case, N) -> the batch seed, chosen as SEEDS was: the first seed from SEED0 + 2000 + 100 N on for which the oracle's twin at
# that model finishes at least 6 of the 37 instances in the active set and at least 2 of those with an input on a bound.  "set_model": a
# handle created at the default model and moved by ndp_set_model to `distinct`'s Qd, Rd and mass (model_cases.CASES["distinct"]: the box,
# dt and g stay the default's).  tests/test_step_model_jvp_edges.py checks every entry by that rule.
MODEL_N = (20, 13)
MODEL_SEEDS = {("distinct", 20): synth.SEED0 + 4000, ("distinct", 13): synth.SEED0 + 3300, ("zero_w", 20): synth.SEED0 + 4000,
               ("zero_w", 13): synth.SEED0 + 3300, ("set_model", 13): synth.SEED0 + 3300}
SET_MODEL_N = 13

# Finite differences of the device's step in the model: unit directions in Qd[0], Qd[8], Rd[2] and the mass, the relative step of
# tests/test_step_model_jvp.py's difference test, on the instances whose status, final set and iteration word are the recorded step's in
# all eight perturbed runs; at least FD_MIN of the 37 (the oracle alone: checked on the CPU).
FD_N, FD_COLS, FD_REL, FD_BAR, FD_MIN = 13, (0, 8, 12, 14), 1e-5, 1e-6, 12
SEED_13_20 = synth.SEED0 + 300      # N = 13 and 20 are not in SEEDS: tests/test_step_model_jvp_gpu.py's batch seed (its twin: 37 set finishes)

# Eight directions in one call: N = 27 (SEEDS[27]) and the <20> kernel (tests/test_step_model_jvp_gpu.py's batch seed).
T8_SEEDS = {27: SEEDS[27], 20: SEED_13_20}


# ---------------------------------------------------------------- what both sides share (no GPU in here)
def case_batch(case, N, seed):
    """deriv_edges.device_case at the case's dt (the same arrays at the default model)."""
    b = synth.make_batch(B, N=N, seed=seed, dt=model_of(case)[6], **MIXED)
    f = np.random.default_rng(seed + 1).normal(0.0, 0.3, (B, N + 1, 3)).astype(np.float32)
    return b, f


def twin_steps(oracle, cfg, b, f, qp_mode=0):
    """The oracle alone over a device case's warm-up and recorded step (from the reset iterate and empty kept sets, the same inputs at
    both): status, iteration word and final set of the recorded step, the iterate and set it started from, and the new iterate."""
    cfg = copy_cfg(cfg)
    cfg.qp_mode = qp_mode
    X, U = b["xr"].copy(), b["ur"].copy()
    act = np.zeros((b["x0"].shape[0], cfg.N, 4), dtype=np.int8)
    for _ in range(2):
        Xl, Ul, actl = X.copy(), U.copy(), act.copy()
        _, st, it, _ = oracle.step_batch_as(cfg, b["x0"], b["xr"], b["ur"], np.asarray(f, dtype=np.float64), X, U, act)
    return dict(st=st, it=it, act=act, Xl=Xl, Ul=Ul, actl=actl, X=X, U=U)


def set_finishes(s):
    """(set finish [B], pinned set finish [B]) of twin_steps' dict (or of _recorded_step's)."""
    ok = (s["st"] == 0) & ((s["it"] & 0xffff) == 0)
    return ok, ok & s["act"].any(axis=(1, 2))


def twin_model_directions(seed, n, Qd, Rd, mass):
    """tmodel [n,3,16]: direction 0 = r' alone, 1 = q'_r on the rows r < 6 with a positive weight, 2 = m' alone; each entry the size of the
    model entry it moves (x 0.5 .. 2, either sign)."""
    rng = np.random.default_rng(seed)
    Qd, Rd = np.asarray(Qd, dtype=np.float64), np.asarray(Rd, dtype=np.float64)
    draw = lambda *s: rng.uniform(0.5, 2.0, s) * rng.choice([-1.0, 1.0], s)  # noqa: E731
    tm = np.zeros((n, 3, 16))
    tm[:, 0, 10:14] = Rd * draw(n, 4)
    tm[:, 1, :6] = Qd[:6] * draw(n, 6)                   # (an unweighted row: 0, it has no twin)
    tm[:, 2, 14] = mass * draw(n)
    return tm


def data_twins(tm, Xp, Up, xr, ur, f, Qd, Rd, mass):
    """The data directions (txr, tur, tf) [n,3,...] equivalent to twin_model_directions' tm at the new iterate (Xp, Up)."""
    Qd, Rd = np.asarray(Qd, dtype=np.float64), np.asarray(Rd, dtype=np.float64)
    n, N = Up.shape[:2]
    txr, tur, tf = np.zeros((n, 3, N + 1, 10)), np.zeros((n, 3, N, 4)), np.zeros((n, 3, N + 1, 3))
    tur[:, 0] = -(tm[:, 0, None, 10:14] / Rd) * (Up - ur)
    txr[:, 1, :, :6] = -(tm[:, 1, None, :6] / np.where(Qd[:6] > 0, Qd[:6], 1.0)) * (Xp[:, :, :6] - xr[:, :, :6])
    tf[:, 2] = -(tm[:, 2, 14] / mass)[:, None, None] * np.asarray(f, dtype=np.float64)
    return txr, tur, tf


def distance(got, ref):
    """max |got - ref| over (du0, dX, dU) of max(1, |ref|max), per instance and direction [n,T]."""
    n, nt = ref[0].shape[:2]
    flat = lambda xs: np.concatenate([np.asarray(x).reshape(n, nt, -1) for x in xs], axis=2)  # noqa: E731
    g, r = flat(got[:3]), flat(ref[:3])
    return np.abs(g - r).max(axis=2) / np.maximum(1.0, np.abs(r).max(axis=2))


def perturbed_models(Qd, Rd, mass):
    """{(column, sign): (engine keywords, step)}: the model with entry FD_COLS[.] moved by +- FD_REL of itself."""
    out = {}
    for col in FD_COLS:
        val = Qd[col] if col < 10 else Rd[col - 10] if col < 14 else mass
        for sgn in (1.0, -1.0):
            q, r, m = list(map(float, Qd)), list(map(float, Rd)), float(mass)
            if col < 10:
                q[col] = val + sgn * FD_REL * val
            elif col < 14:
                r[col - 10] = val + sgn * FD_REL * val
            else:
                m = val + sgn * FD_REL * val
            out[col, sgn] = (dict(Qd=q, Rd=r, mass=m), FD_REL * val)
    return out


# ---------------------------------------------------------------- the device side
def _model_duality_gap(a, j, g, tan, tm):
    """|<gz, JVP(theta', t)> - <VJP(gz), t> - sum_{j<15} gmodel[j] theta'_j| per instance, worst over the directions, of the largest |term|
    (at least 1)."""
    gap = np.zeros(B)
    flat = lambda xs: np.concatenate([x.reshape(B, -1) for x in xs], axis=1)  # noqa: E731
    for k in range(tm.shape[1]):
        lhs = [g[0] * j[0][:B, k], g[1] * j[1][:B, k], g[2] * j[2][:B, k]]
        rhs = [x[:B] * t[:, k] for x, t in zip(a[:4], tan)] + [a[6][:B, :15] * tm[:, k, :15]]
        mag = np.maximum(1.0, np.abs(flat(lhs + rhs)).max(axis=1))
        gap = np.maximum(gap, np.abs(flat(lhs).sum(axis=1) - flat(rhs).sum(axis=1)) / mag)
    return gap


def _calls(r, b, f, seed, model, extra=None):
    """From one recorded step's engine (closed here): the model direction alone and beside data directions (T = 2), the adjoint with the
    model gradient for a seeded upstream, the three twin directions along rti_mjvp_kernel and along rti_jvp_kernel, the latter once more
    from the wiggled iterate, and (extra: tmodel [B,n,16]) further model directions.  Every output with GUARD rows behind the batch."""
    eng, a, N = r["eng"], (r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"]), r["eng"].N
    Qd, Rd, mass = model
    rng = np.random.default_rng(seed + 6)
    c = dict(N=N, b=b, f=f, r=r, waves=eng.debug_rti_launched()[1])
    c["tm"] = rng.normal(size=(B, T, 16))
    c["tan"] = _tangents(seed + 7, B, N, T)
    c["g"] = (rng.normal(size=(B, 4)), rng.normal(size=(B, N + 1, 10)), rng.normal(size=(B, N, 4)))
    c["model"] = _mjvp(eng, *a, c["tm"], f=r["force"], guard=GUARD)
    c["mixed"] = _mjvp(eng, *a, c["tm"], f=r["force"], guard=GUARD, **_tt(c["tan"]))
    c["grad"] = _vjp(eng, *a, f=r["force"], model=True, guard=GUARD, **dict(zip(("gu0", "gX", "gU"), (_t(x) for x in c["g"]))))
    c["twin_tm"] = tw = twin_model_directions(seed + 8, B, Qd, Rd, mass)
    xi = np.random.default_rng(seed + 9)
    wig = lambda v: v * (1.0 + TWIN_WIGGLE * xi.choice([-1.0, 1.0], v.shape))  # noqa: E731
    data = lambda X, U: dict(zip(("txr", "tur", "tf"), (_t(v) for v in data_twins(tw, X, U, b["xr"], b["ur"], f, Qd, Rd, mass))))  # noqa: E731
    c["twin_m"] = _mjvp(eng, *a, tw, f=r["force"], guard=GUARD)
    c["twin_d"] = _jvp(eng, *a, 3, f=r["force"], guard=GUARD, **data(r["X"], r["U"]))
    c["twin_w"] = _jvp(eng, *a, 3, f=r["force"], guard=GUARD, **data(wig(r["X"]), wig(r["U"])))
    if extra is not None:
        c["extra_tm"], c["extra"] = extra, _mjvp(eng, *a, extra, f=r["force"], guard=GUARD)
    c["tape"] = tuple(v.cpu().numpy() for v in r["tape"])
    eng.close()
    return c


def _dense(c, oracle, cfg):
    """The dense systems with their model columns of the 6 pick()ed set finishes (2 pinned), built once."""
    ok, pinned = _finishes(c["r"])
    assert ok.sum() >= 6 and pinned.sum() >= 2, (c["N"], int(ok.sum()), int(pinned.sum()))
    b, f, r, (Xl, Ul, _) = c["b"], c["f"], c["r"], c["tape"]
    c["idx"] = pick(ok, pinned)
    c["sys"] = {i: MR.model_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), Xl[i], Ul[i], r["act"][i])
                for i in c["idx"]}
    return c


@pytest.fixture(scope="module")
def medge(ndp, oracle):
    """Per (horizon, qp_mode), built when first asked for: the recorded step at the default model and _calls' outputs; qp_mode 0: the
    dense systems of 6 set finishes beside them.  Every engine is closed in _calls."""
    cache = {}

    def get(N, qp_mode=0):
        if (N, qp_mode) not in cache:
            seed = IPM_SEEDS[N] if qp_mode else SEEDS[N]
            b, f = device_case(N, seed)
            r = _recorded_step(ndp, b, f=f, **(dict(qp_mode=1) if qp_mode else {}))
            c = _calls(r, b, f, seed, model_of({})[:3])
            cache[N, qp_mode] = c if qp_mode else _dense(c, oracle, oracle.default_cfg(N=N, use_fd=True))
        return cache[N, qp_mode]

    return get


@pytest.fixture(scope="module")
def mcase(ndp, oracle):
    """Per (model, N), built when first asked for: as medge's at the model, with three unit directions more (columns 6, 3 and 8).
    "set_model": a default handle moved there by ndp_set_model before its first step."""
    cache = {}

    def get(name, N):
        if (name, N) not in cache:
            seed = MODEL_SEEDS[name, N]
            moved = name == "set_model"
            case = CASES["distinct"] if moved else DERIV_CASES[name]
            Qd, Rd, mass = model_of(case)[:3]
            b, f = case_batch(case, N, seed)
            if moved:
                r = _recorded_step(ndp, b, f=f, prepare=lambda eng: eng.set_model(Qd=Qd, Rd=Rd, mass=mass))
            else:
                r = _recorded_step(ndp, b, f=f, **engine_kw(case))
            units = np.ascontiguousarray(np.broadcast_to(np.eye(16)[[6, 3, 8]][None], (B, 3, 16)))
            cache[name, N] = _dense(_calls(r, b, f, seed, (Qd, Rd, mass), extra=units), oracle, oracle_cfg(oracle, case, N=N, use_fd=True))
        return cache[name, N]

    return get


def _the_recompute_is_the_step(c, names=("model", "mixed", "twin_m", "twin_d", "twin_w", "extra")):
    for k in names:
        if k in c:
            assert _guards_intact(c[k], B), k
            assert np.array_equal(c[k][4][:B], c["r"]["st"]), k
    assert _guards_intact(c["grad"], B) and np.array_equal(c["grad"][5][:B], c["r"]["st"])


def _held_to_the_dense_reference(c, what):
    """The model direction alone and beside the data directions on the 6 checked set finishes: 1e-9 of max(1, |z'|max) of model_jvp_apply;
    the facts that hold exactly; duality with the model adjoint on every set finish of the batch."""
    r, tm, tan, m, x = c["r"], c["tm"], c["tan"], c["model"], c["mixed"]
    _the_recompute_is_the_step(c)
    worst = worst_mixed = 0.0
    for i in c["idx"]:
        for k in range(T):
            for got, data, mixed in ((m, (), False), (x, tuple(t[i, k] for t in tan), True)):
                ref = MR.model_jvp_apply(c["sys"][i], tm[i, k], *data)
                e = max(np.max(np.abs(g[i, k] - y)) for g, y in zip(got[:3], ref)) / max(scale(y) for y in ref)
                worst, worst_mixed = (worst, max(worst_mixed, e)) if mixed else (max(worst, e), worst_mixed)
    ok = r["st"] == 0
    fin, pinned = _finishes(r)
    gap = _model_duality_gap(c["grad"], x, c["g"], tan, tm)
    print(f"{what}: worst distance from the dense reference: model direction {worst:.3e}, with the data's {worst_mixed:.3e} (bar 1e-9); "
          f"duality gap on {int(fin.sum())} set finishes ({int(pinned.sum())} pinned) {gap[fin].max():.3e} (bar 1e-10)")
    assert worst <= SENS_BAR and worst_mixed <= SENS_BAR, (what, worst, worst_mixed)
    assert not m[1][:B][ok][:, :, 0].any() and np.array_equal(x[1][:B][ok][:, :, 0], tan[0][ok])
    for o in (m, x):
        dU = o[2][:B]
        assert np.array_equal(o[0][:B][ok], dU[ok][:, :, 0])
        assert not dU[fin][np.broadcast_to((r["act"][fin] != 0)[:, None], dU[fin].shape)].any()
        assert all(np.isfinite(v[:B][ok]).all() for v in o[:3])
    assert np.abs(m[1][:B][ok]).max() > 1e-6
    assert gap[fin].max() <= SET_DUALITY_BAR, (what, gap[fin].max())


def _twins_held(c, what):
    """rti_mjvp_kernel along the three model directions against rti_jvp_kernel along their data twins, on every status-0 instance."""
    r = c["r"]
    _the_recompute_is_the_step(c, ("twin_m", "twin_d", "twin_w"))
    ok = r["st"] == 0
    fin = _finishes(r)[0]
    ipm = ok & ~fin
    assert ok.any()
    ref = tuple(v[:B] for v in c["twin_d"][:3])
    d = distance(tuple(v[:B] for v in c["twin_m"][:3]), ref)
    floor = distance(tuple(v[:B] for v in c["twin_w"][:3]), ref)[ok].max()
    moved = np.abs(ref[1][ok]).max(axis=(0, 2, 3))
    assert (moved > 1e-6).all(), (what, moved)           # (each of the three directions moves the step)
    bar = max(SET_DUALITY_BAR, TWIN_FLOOR_FACTOR * floor)
    print(f"{what}: model directions against their data twins: {int(fin.sum())} set finishes "
          f"{d[fin].max() if fin.any() else 0.0:.3e} (bar 1e-10); {int(ipm.sum())} interior-point finishes "
          f"{d[ipm].max() if ipm.any() else 0.0:.3e}, floor of rti_jvp_kernel alone {floor:.3e}, bar {bar:.3e}")
    assert np.isfinite(d[ok]).all()
    if fin.any():
        assert d[fin].max() <= SET_DUALITY_BAR, (what, d[fin].max(axis=0))
    if ipm.any():
        assert bar <= TWIN_BAR_CEILING, (what, floor)
        assert d[ipm].max() <= bar, (what, d[ipm].max(axis=0), bar)


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_model_directions_match_the_dense_reference_at_the_edge_horizons(medge, N):
    """rti_mjvp_kernel<0> at horizon N (4 instances per workgroup up to N = 19, 2 from N = 21), T = 2, the model direction alone and beside
    data directions: on 6 seeded status-0 set finishes (2 pinned) du0, dX, dU within 1e-9 of max(1, |z'|max) of model_jvp_apply; on every
    status-0 instance dX_0 exactly 0 or tx0 and du0 = dU_0, on every set finish the pinned rows of dU exactly 0; status_check is the
    step's; the guard rows behind the ragged batch keep their fill; on every set finish of the 37 duality with
    ndp_step_vjp_model_device on the same tape within 1e-10 of the largest term."""
    c = medge(N)
    assert c["waves"] == geometry(N)[0]
    _held_to_the_dense_reference(c, f"N={N}")


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_model_directions_equal_their_data_twins_at_the_edge_horizons(medge, N):
    """The three twins (module docstring) at horizon N in the default QP mode, on every status-0 instance: 1e-10 of max(1, |z'|max) on set
    finishes, the measured-floor bar on interior-point finishes (where the device has any)."""
    _twins_held(medge(N), f"N={N}")


@pytest.mark.parametrize("N", IPM_N)
def test_twins_and_duality_after_interior_point_finishes(medge, N):
    """qp_mode 1: the step is CX|CU itself and rho is parked in place, rows 6..9 kept for the q+ parking.  At least B // 2 instances
    finish with status 0, every one of them in the interior-point loop; outputs finite, pinned rows of dU exactly 0, duality with the
    model adjoint within 1e-6 (test_duality_on_interior_point_finishes_either_side_of_the_sweep_switch's facts, here through
    rti_mjvp_kernel and rti_wvjp_kernel along random model and data directions); then the twins under the measured-floor bar."""
    c = medge(N, 1)
    r = c["r"]
    assert c["waves"] == geometry(N)[0]
    _the_recompute_is_the_step(c)
    ok = r["st"] == 0
    assert ok.sum() >= B // 2 and ((r["it"] & 0xffff)[ok] > 0).all(), int(ok.sum())
    for k in ("model", "mixed", "twin_m", "twin_d"):
        assert all(np.isfinite(v[:B][ok]).all() for v in c[k][:3]), k
        dU = c[k][2][:B]
        assert not dU[ok][np.broadcast_to((r["act"][ok] != 0)[:, None], dU[ok].shape)].any(), k
    assert all(np.isfinite(v[:B][ok]).all() for v in c["grad"][:4] + c["grad"][6:])
    gap = _model_duality_gap(c["grad"], c["mixed"], c["g"], c["tan"], c["tm"])
    print(f"N={N} qp_mode=1: duality gap with the model adjoint on {int(ok.sum())} interior-point finishes {gap[ok].max():.3e} (bar 1e-6)")
    assert gap[ok].max() <= IPM_DUALITY_BAR, (N, gap[ok].max())
    _twins_held(c, f"N={N} qp_mode=1")


# ---------------------------------------------------------------- other models
@pytest.mark.parametrize("N", MODEL_N)
@pytest.mark.parametrize("name", list(DERIV_CASES))
def test_other_models_match_the_dense_reference_and_their_twins(mcase, name, N):
    """`distinct` (no two weights equal, Qd[6] = 7, the asymmetric box, dt 0.05, g 7.0, mass 0.9) and `zero_w` (velocity and attitude
    unweighted) at N = 20 and 13: the dense reference at the model and duality with the model adjoint as at the edge horizons; a unit
    direction in column 6 gives exact zeros (also where Qd[6] = 7); unit directions in columns 3 and 8 match the reference, and in zero_w,
    where those rows carry no weight, they do move the step; the twins on the rows with a positive weight."""
    c = mcase(name, N)
    assert c["waves"] == geometry(N)[0]
    _held_to_the_dense_reference(c, f"{name} N={N}")
    ok = c["r"]["st"] == 0
    u = tuple(v[:B] for v in c["extra"][:3])
    assert all(not v[ok][:, 0].any() for v in u)
    worst = 0.0
    for i in c["idx"]:
        for k in (1, 2):
            ref = MR.model_jvp_apply(c["sys"][i], c["extra_tm"][i, k])
            worst = max(worst, max(np.max(np.abs(g[i, k] - y)) for g, y in zip(u, ref)) / max(scale(y) for y in ref))
    print(f"{name} N={N}: unit directions in columns 3 and 8 against the dense reference {worst:.3e}; |dX|max "
          f"{np.abs(u[1][ok][:, 1]).max():.3e} / {np.abs(u[1][ok][:, 2]).max():.3e}")
    assert worst <= SENS_BAR, (name, N, worst)
    if name == "zero_w":
        assert model_of(DERIV_CASES[name])[0][3] == 0.0 and model_of(DERIV_CASES[name])[0][8] == 0.0
        assert np.abs(u[1][ok][:, 1]).max() > 1e-9 and np.abs(u[1][ok][:, 2]).max() > 1e-9
        assert not c["twin_tm"][:, 1, 3:6].any() and c["twin_tm"][:, 1, :3].all()
    _twins_held(c, f"{name} N={N}")


def test_a_handle_moved_by_set_model_matches_the_dense_reference_at_that_model(mcase):
    """N = 13: a handle created at the default model and moved by ndp_set_model to `distinct`'s Qd, Rd and mass before its first step: the
    kernel reads Qd[7 + a] from its parameters, Qd and Rd out of LDS and 1 / m^2 as the handle now has them -- the dense reference at that
    model within 1e-9, duality and the twins as everywhere."""
    c = mcase("set_model", SET_MODEL_N)
    _held_to_the_dense_reference(c, f"set_model N={SET_MODEL_N}")
    _twins_held(c, f"set_model N={SET_MODEL_N}")


# ---------------------------------------------------------------- finite differences of the device's own step
def test_device_finite_differences_in_the_model(ndp):
    """N = 13: the central difference of (u0, X, U) over handles that differ only in Qd[0], Qd[8], Rd[2] or the mass by +- 1e-5 of the
    entry, each started from the recorded step's iterate and kept set, against rti_mjvp_kernel's tangent along the unit direction --
    within 1e-6 of max(1, |z'|max) on the instances whose status, final set and iteration word are the recorded step's in all eight
    runs; at least 12 of the 37."""
    import torch
    N = FD_N
    b, f = device_case(N, SEED_13_20)
    r = _recorded_step(ndp, b, f=f)
    units = np.ascontiguousarray(np.broadcast_to(np.eye(16)[list(FD_COLS)][None], (B, len(FD_COLS), 16)))
    tang = _mjvp(r["eng"], r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"], units, f=r["force"], guard=GUARD)
    Xl, Ul, actl = (v.cpu().numpy() for v in r["tape"])
    r["eng"].close()
    assert _guards_intact(tang, B) and np.array_equal(tang[4][:B], r["st"])
    Qd, Rd, mass = model_of({})[:3]

    def step(kw):
        eng = ndp.BatchedNMPC(B, N=N, disturbance=True, **kw)
        eng.reset(b["xr"], b["ur"])
        eng.set_iterate(Xl, Ul)
        eng.set_active_set(actl)
        u0 = torch.empty(B, 4, dtype=torch.float64, device=_dev())
        eng.update_device(r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], u0, f=r["force"])
        eng.synchronize()
        X, U = eng.get_iterate()
        st, it = eng.status()
        out = (u0.cpu().numpy(), X, U, st, it, eng.active_set()[1])
        eng.close()
        return out

    runs = {k: (step(kw), h) for k, (kw, h) in perturbed_models(Qd, Rd, mass).items()}
    stable = r["st"] == 0
    for o, _ in runs.values():
        stable &= (o[3] == r["st"]) & (o[4] == r["it"]) & (o[5] == r["act"]).all(axis=(1, 2))
    assert stable.sum() >= FD_MIN, int(stable.sum())
    worst = {}
    for k, col in enumerate(FD_COLS):
        (p, h), (m, _) = runs[col, 1.0], runs[col, -1.0]
        fd = tuple(((x - y) / (2 * h))[:, None] for x, y in zip(p[:3], m[:3]))
        got = tuple(v[:B][:, k:k + 1] for v in tang[:3])
        assert np.abs(got[1][stable]).max() > 1e-9                     # (a tangent that is there to be compared)
        worst[col] = distance(fd, got)[stable].max()
    print(f"N={N}: central differences of the device's step against the tangent on {int(stable.sum())} instances, by column: "
          + ", ".join(f"{c}: {w:.3e}" for c, w in worst.items()) + " (bar 1e-6)")
    assert max(worst.values()) <= FD_BAR, worst


# ---------------------------------------------------------------- eight directions
@pytest.mark.parametrize("N", list(T8_SEEDS))
def test_eight_directions_in_one_call_are_eight_calls_bit_for_bit(ndp, N):
    """n_tan = 8 at the step level, model and data directions together, at N = 27 and on the <20> kernel: one call equals eight calls of
    one direction, bit for bit; nothing is written behind the batch."""
    b, f = device_case(N, T8_SEEDS[N])
    r = _recorded_step(ndp, b, f=f)
    eng, a = r["eng"], (r["t"]["x0"], r["t"]["xr"], r["t"]["ur"], r["tape"])
    tm = np.random.default_rng(N + 40).normal(size=(B, 8, 16))
    tan = _tangents(N + 41, B, N, 8)
    eight = _mjvp(eng, *a, tm, f=r["force"], guard=GUARD, **_tt(tan))
    ones = [_mjvp(eng, *a, np.ascontiguousarray(tm[:, d:d + 1]), f=r["force"], guard=GUARD,
                  **_tt(tuple(np.ascontiguousarray(t[:, d:d + 1]) for t in tan))) for d in range(8)]
    eng.close()
    assert _guards_intact(eight, B) and all(_guards_intact(o, B) for o in ones)
    ok = r["st"] == 0
    assert ok.sum() >= 30 and all(np.isfinite(v[:B][ok]).all() for v in eight[:3])
    for d, one in enumerate(ones):
        for x, y in zip(eight[:3], one[:3]):
            assert np.array_equal(x[:B, d], y[:B, 0], equal_nan=True), d
        assert np.array_equal(eight[3], one[3], equal_nan=True) and np.array_equal(eight[4], one[4])
    assert len({eight[1][:B][ok][:, d].tobytes() for d in range(8)}) == 8      # (eight different tangents)
