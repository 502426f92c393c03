"""What tests/test_step_model_jvp_edges_gpu.py rests on, without a GPU: the three data twins of the model directions proved on the float64
reference itself, and every seed and count condition of the device module by the oracle alone -- the qp_mode 1 seeds, the other models'
seeds, and the instances whose set does not move under the finite-difference steps."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import fixed_set_ref as F
from tests import model_jvp_ref as MR
from tests import test_step_model_jvp_edges_gpu as G
from tests.deriv_edges import DERIV_EDGE_N, DEVICE_B, device_case, pick
from tests.model_cases import CASES, DERIV_CASES, model_of, oracle_cfg
from tests.test_deriv_edges_gpu import SEEDS

TWIN_BAR = 1e-10


@pytest.mark.parametrize("N", [2, 6, 17, 27])
def test_the_model_directions_and_their_data_twins_are_one_tangent_on_the_reference(oracle, N):
    """The oracle's set-finish systems of the device case at N (3 instances, 2 of them pinned), (X+, U+) = the linearisation point plus the
    dense system's solution: model_jvp_apply along r', along q'_r (r < 6) and along m' against fixed_set_ref.jvp_apply along the
    equivalent tur, txr and tf -- one right-hand side each, so equal to rounding: 1e-10 of max(1, |z'|max)."""
    b, f = device_case(N, SEEDS[N])
    cfg = oracle.default_cfg(N=N, use_fd=True)
    s = G.twin_steps(oracle, cfg, b, f)
    ok, pinned = G.set_finishes(s)
    idx = pick(ok, pinned, n=3, n_pinned=2)
    assert len(idx) == 3 and sum(bool(pinned[i]) for i in idx) >= 2
    Qd, Rd, mass = model_of({})[:3]
    tm = G.twin_model_directions(SEEDS[N] + 8, DEVICE_B, Qd, Rd, mass)
    nzx = (N + 1) * 10
    worst = np.zeros(3)
    for i in idx:
        c = MR.model_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f[i].astype(np.float64), s["Xl"][i], s["Ul"][i], s["act"][i])
        Xp = s["Xl"][i] + c["sol"][:nzx].reshape(N + 1, 10)
        Up = s["Ul"][i] + c["sol"][nzx:c["nz"]].reshape(N, 4)
        assert np.max(np.abs(Xp - s["X"][i])) <= 1e-9 and np.max(np.abs(Up - s["U"][i])) <= 1e-9     # (the oracle's step is that solution)
        txr, tur, tf = G.data_twins(tm[i:i + 1], Xp[None], Up[None], b["xr"][i:i + 1], b["ur"][i:i + 1], f[i:i + 1], Qd, Rd, mass)
        for k in range(3):
            model = MR.model_jvp_apply(c, tm[i, k])
            data = F.jvp_apply(c, None, txr[0, k], tur[0, k], tf[0, k])[:3]
            sc = max(F.scale(y) for y in data)
            assert max(np.abs(y).max() for y in data) > 1e-6, (i, k)
            worst[k] = max(worst[k], max(np.max(np.abs(x - y)) for x, y in zip(model, data)) / sc)
    print(f"N={N}: model direction against its data twin on the reference: r' {worst[0]:.3e}, q' {worst[1]:.3e}, m' {worst[2]:.3e}")
    assert worst.max() <= TWIN_BAR, worst


def test_the_case_batch_is_the_device_case_at_the_default_model():
    for N in (13, 20):
        (b, f), (b2, f2) = G.case_batch({}, N, G.SEED_13_20), device_case(N, G.SEED_13_20)
        assert all(np.array_equal(b[k], b2[k]) for k in ("x0", "xr", "ur")) and np.array_equal(f, f2)


@pytest.mark.parametrize("N", list(G.T8_SEEDS))
def test_the_eight_direction_batches_finish_by_the_twin(oracle, N):
    """The device's eight-direction cases want at least 30 of the 37 instances with status 0: the oracle's twin finishes every one."""
    b, f = device_case(N, G.T8_SEEDS[N])
    s = G.twin_steps(oracle, oracle.default_cfg(N=N, use_fd=True), b, f)
    assert (s["st"] == 0).sum() >= 30, int((s["st"] == 0).sum())


def _ipm_ok(oracle, N, seed):
    b, f = device_case(N, seed)
    s = G.twin_steps(oracle, oracle.default_cfg(N=N, use_fd=True), b, f, qp_mode=1)
    return int((s["st"] == 0).sum()), bool(((s["it"] & 0xffff)[s["st"] == 0] > 0).all())


@pytest.mark.parametrize("N", G.IPM_N)
def test_the_interior_point_seeds_by_the_oracle_alone(oracle, N):
    """IPM_SEEDS[N] of the device module: SEEDS[N] where the oracle at qp_mode 1 finishes at least B // 2 of the 37 instances with status 0
    over the warm-up and the recorded step, else the first seed from SEED0 + 5000 + 100 N on that does; and every such finish iterated."""
    need = DEVICE_B // 2
    seed = G.IPM_SEEDS[N]
    n, iterated = _ipm_ok(oracle, N, seed)
    assert n >= need and iterated, (N, n)
    if N in SEEDS:
        if seed != SEEDS[N]:
            assert _ipm_ok(oracle, N, SEEDS[N])[0] < need
    if seed != SEEDS.get(N):
        first = synth.SEED0 + 5000 + 100 * N
        assert seed >= first and all(_ipm_ok(oracle, N, s)[0] < need for s in range(first, seed))
    assert set(G.IPM_SEEDS) == set(G.IPM_N) == {3, 4, 6, 12, 17, 20, 21}


def _model_counts(oracle, name, N, seed):
    case = CASES["distinct"] if name == "set_model" else DERIV_CASES[name]
    b, f = G.case_batch(case, N, seed)
    ok, pinned = G.set_finishes(G.twin_steps(oracle, oracle_cfg(oracle, case, N=N, use_fd=True), b, f))
    return int(ok.sum()), int(pinned.sum())


@pytest.mark.parametrize("name,N", list(G.MODEL_SEEDS))
def test_the_other_models_seeds_by_the_twin(oracle, name, N):
    """MODEL_SEEDS of the device module, by the rule SEEDS was chosen by: the first seed from SEED0 + 2000 + 100 N on for which the oracle's
    twin at the model finishes at least 6 of the 37 instances in the active set, at least 2 of them with an input on a bound."""
    good = lambda c: c[0] >= 6 and c[1] >= 2  # noqa: E731
    seed, first = G.MODEL_SEEDS[name, N], synth.SEED0 + 2000 + 100 * N
    counts = _model_counts(oracle, name, N, seed)
    print(f"{name} N={N}: {counts[0]} set finishes, {counts[1]} pinned")
    assert good(counts), (name, N, counts)
    assert seed >= first and not any(good(_model_counts(oracle, name, N, s)) for s in range(first, seed))
    assert set(G.MODEL_SEEDS) == {(n, N) for n in DERIV_CASES for N in G.MODEL_N} | {("set_model", G.SET_MODEL_N)}
    assert G.MODEL_N == (20, 13)


def test_enough_instances_keep_their_set_under_the_finite_difference_steps(oracle):
    """The device's finite-difference test (N = 13, columns 0, 8, 12, 14, +- 1e-5 of the entry), by the oracle alone: from the recorded
    step's iterate and kept set, at least FD_MIN of the 37 instances finish with the recorded step's status, set and iteration word in
    all eight perturbed runs; on those the oracle's central difference is the reference's tangent within the device test's bar."""
    N = G.FD_N
    assert (N, G.FD_COLS, G.FD_REL, G.FD_BAR, G.FD_MIN) == (13, (0, 8, 12, 14), 1e-5, 1e-6, 12)
    b, f = device_case(N, G.SEED_13_20)
    cfg = oracle.default_cfg(N=N, use_fd=True)
    cfg.qp_mode = 0
    s = G.twin_steps(oracle, cfg, b, f)
    f64 = f.astype(np.float64)

    def step(c):
        X, U, act = s["Xl"].copy(), s["Ul"].copy(), s["actl"].copy()
        _, st, it, _ = oracle.step_batch_as(c, b["x0"], b["xr"], b["ur"], f64, X, U, act)
        return X, U, st, it, act

    base = step(cfg)
    assert all(np.array_equal(x, y) for x, y in zip(base, (s["X"], s["U"], s["st"], s["it"], s["act"])))
    stable = G.set_finishes(s)[0].copy()
    runs = {}
    for key, (kw, h) in G.perturbed_models(*model_of({})[:3]).items():
        c = F.copy_cfg(cfg)
        for j in range(10):
            c.Qd[j] = kw["Qd"][j]
        for j in range(4):
            c.Rd[j] = kw["Rd"][j]
        c.mass = kw["mass"]
        runs[key] = (step(c), h)
        o = runs[key][0]
        stable &= (o[2] == s["st"]) & (o[3] == s["it"]) & (o[4] == s["act"]).all(axis=(1, 2))
    assert stable.sum() >= G.FD_MIN, int(stable.sum())
    worst = 0.0
    for i in np.flatnonzero(stable)[:4]:
        c = MR.model_system(oracle, cfg, b["x0"][i], b["xr"][i], b["ur"][i], f64[i], s["Xl"][i], s["Ul"][i], s["act"][i])
        for col in G.FD_COLS:
            (p, h), (m, _) = runs[col, 1.0], runs[col, -1.0]
            _, rX, rU = MR.model_jvp_apply(c, np.eye(16)[col])
            sc = max(F.scale(rX), F.scale(rU))
            worst = max(worst, np.max(np.abs((p[0][i] - m[0][i]) / (2 * h) - rX)) / sc, np.max(np.abs((p[1][i] - m[1][i]) / (2 * h) - rU)) / sc)
    print(f"N={N}: {int(stable.sum())} of {DEVICE_B} instances keep status, set and iteration word; the oracle's central difference "
          f"against the reference's tangent {worst:.3e} (bar 1e-6)")
    assert worst <= G.FD_BAR


def test_the_device_modules_horizons_and_bars():
    """What the device module's cases are parametrised over, and that its bars are the project's."""
    params = lambda t: {m.args[0]: list(m.args[1]) for m in getattr(t, "pytestmark", []) if m.name == "parametrize"}  # noqa: E731
    assert tuple(params(G.test_model_directions_match_the_dense_reference_at_the_edge_horizons)["N"]) == DERIV_EDGE_N
    assert tuple(params(G.test_model_directions_equal_their_data_twins_at_the_edge_horizons)["N"]) == DERIV_EDGE_N
    assert tuple(params(G.test_twins_and_duality_after_interior_point_finishes)["N"]) == G.IPM_N
    assert params(G.test_eight_directions_in_one_call_are_eight_calls_bit_for_bit)["N"] == [27, 20]
    assert (G.SENS_BAR, G.SET_DUALITY_BAR, G.IPM_DUALITY_BAR, G.FD_BAR) == (1e-9, 1e-10, 1e-6, 1e-6)
    assert (G.TWIN_FLOOR_FACTOR, G.TWIN_BAR_CEILING, G.TWIN_WIGGLE, G.B, G.GUARD) == (10.0, 1e-6, 1e-12, 37, 2)
