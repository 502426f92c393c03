"""The control step's five derivative passes at the horizons where their shape changes (tests/deriv_edges.py: DERIV_EDGE_N), without a GPU:
the list derived by arithmetic, the device's code on the host wave emulator (tests/step_deriv_emu.cpp) against the dense fixed-set references
(tests/fixed_set_ref.py) and against itself by duality, interior-point finishes either side of the sweep switch, the device cases' seeds
against the oracle's twin, and the ledger of recompute-kernel launches.  The device side: tests/test_deriv_edges_gpu.py."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth
from tests import test_deriv_edges_gpu as G
from tests import test_kernel_table_gpu as K
from tests.deriv_edges import DERIV_EDGE_N, chunk_sizes, device_case, ldl_after_interior_point, small_case, twin_finishes
from tests.fixed_set_ref import jvp_apply, jvp_system, model_grad_ref, psens_apply, scale, sens_ref, vjp_apply
from tests.step_deriv_emu import MIXED, _emu_step, _jvp, _psens, _tape, _vjp, step_emu  # noqa: F401
from tests.test_kernel_table import slots_for

B, T = 3, 2
EMU_BAR, DUALITY_BAR = 1e-10, 1e-11


# ---------------------------------------------------------------- the list
def _shape(N):
    """Everything of the derivative passes that follows the horizon: the chunk counts of the five loops, the constraint slots, the
    instances per workgroup, the sweep after an interior-point finish."""
    return tuple((n + 63) // 64 for n in chunk_sizes(N)) + (slots_for(N), K.geometry(N)[0], ldl_after_interior_point(N))


def test_the_edge_list_holds_every_horizon_where_a_count_changes():
    """Every N in 2..27 whose shape differs from N - 1's is in DERIV_EDGE_N or is 20 (the compile-time horizon, covered by the existing
    modules); so are the smallest and the largest horizon and the two exactly-full chunks, 4(N+1) = 64 and 4N = 64."""
    assert tuple(sorted(set(DERIV_EDGE_N))) == DERIV_EDGE_N and DERIV_EDGE_N[0] == 2 and DERIV_EDGE_N[-1] == 27
    changes = [N for N in range(3, 28) if _shape(N) != _shape(N - 1)]
    assert changes == [4, 6, 10, 12, 16, 17, 19, 21, 25], changes          # (the issue's table, recomputed)
    assert set(changes) <= set(DERIV_EDGE_N) | {20}
    assert chunk_sizes(15)[3] == 64 and chunk_sizes(16)[1] == 64 and {15, 16} <= set(DERIV_EDGE_N)
    assert not ldl_after_interior_point(3) and ldl_after_interior_point(4) and {3, 4} <= set(DERIV_EDGE_N)
    assert slots_for(27) == 3 and slots_for(28) == 4                       # (27: the largest horizon the derivative kernels serve)
    assert chunk_sizes(20)[2] == 63                                        # (the force at N = 20: one lane short of a full chunk)


def test_the_references_block_product_is_the_dense_systems(oracle):
    """fixed_set_ref.system_times (what the data columns are differenced with) against system()'s dense K and right-hand side, on random
    vectors, with pins, at a small and the largest horizon: equal to rounding."""
    from tests.fixed_set_ref import fixed_of, system, system_times
    for N in (3, 27):
        b = synth.make_batch(1, N=N, seed=synth.SEED0 + 41, **MIXED)
        rng = np.random.default_rng(N)
        cfg = oracle.default_cfg(N=N, use_fd=True)
        qp = oracle.linearize(cfg, b["x0"][0], b["xr"][0], b["ur"][0], rng.normal(size=(N + 1, 3)), *_tape(b, 0, rng, N)[:2])
        act = np.zeros((N, 4), dtype=np.int8)
        act[0, 1], act[N - 1, 3], act[1, 0] = 1, -1, 1
        fixed = fixed_of(qp, act) + [(13, 0.25)]
        Kd, rhs, _ = system(qp, fixed)
        v = rng.normal(size=Kd.shape[0])
        got, rhs2 = system_times(qp, fixed, v)
        assert np.array_equal(rhs, rhs2)
        assert np.max(np.abs(got - Kd @ v)) <= 1e-12 * np.max(np.abs(Kd @ v))


# ---------------------------------------------------------------- the five passes on the host emulator
_cases = {}


def _case(oracle, lib, N):
    """B mixed instances at horizon N with a supplied force, all five passes from one tape each (the same step: the same final set), and
    one dense system per instance for every reference.  Built once per horizon.  The workload alone pins an input at stage 0 at most (and
    none at N = 2), so instance 1's input reference lies 1 rad/s outside the bounds at the last stage (a roll rate above the upper
    bound) and, from N = 17, at stage 16 (a yaw rate below the lower one): the step pins them, and the case asserts that a set finish
    has a pin at every horizon, one at the last stage, and from N = 17 one in the inputs' second chunk (4 k + i >= 64)."""
    if N in _cases:
        return _cases[N]
    from tests.emu import emu
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=True)
    b["ur"][1, N - 1, 0] = cfg.ubu[0] + 1.0
    if N >= 17:
        b["ur"][1, 16, 2] = cfg.lbu[2] - 1.0
    ocfg = oracle.default_cfg(N=N, use_fd=True)
    rng = np.random.default_rng(500 + N)
    out = []
    for i in range(B):
        X, U, act = _tape(b, i, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32)
        tan = (rng.normal(size=(T, 10)), rng.normal(size=(T, N + 1, 10)), rng.normal(size=(T, N, 4)), rng.normal(size=(T, N + 1, 3)))
        g = (rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4)))
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        s = _emu_step(lib, cfg, 2, b["x0"][i], b["xr"][i], b["ur"][i], X, U, act, f=f)
        p = _psens(lib, *args)
        a = _vjp(lib, *args, *g, model=True)
        j = _jvp(lib, *args, *tan)
        for o in (p, a, j):                               # every pass recomputes the same step
            assert all(np.array_equal(x, y) for x, y in zip(s[:6], o[:6]))
        assert s[3] == 0
        d = dict(i=i, s=s, p=p, a=a, j=j, tan=tan, g=g, A=s[5].reshape(N, 4), set_finish=not s[4] & 0xffff)
        if d["set_finish"]:
            f64 = f.astype(np.float64)
            d["qp"] = oracle.linearize(ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64, X, U)
            d["sys"] = jvp_system(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64, X, U, d["A"])
            d["gm"] = model_grad_ref(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64, X, U, d["A"], *g)
        out.append(d)
    assert sum(d["set_finish"] for d in out) >= 2
    pins = [d["A"] != 0 for d in out if d["set_finish"]]
    assert any(A.any() for A in pins) and any(A[N - 1].any() for A in pins), N
    assert N < 17 or any(A.ravel()[64:].any() for A in pins), N
    assert N < 4 or any(A[0].any() for A in pins), N                     # (stage 0: the parameter sensitivities' pinned rows)
    _cases[N] = out
    return out


def _held(got, ref, s, what, N, d, worst):
    err = np.max(np.abs(got - ref)) / s
    assert err <= EMU_BAR, (what, N, d["i"], err)
    return max(worst, err)


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_emulated_level2_sensitivities_at_the_edge_horizons(oracle, step_emu, N):
    """sens_out level 2: du0, dU, dX within 1e-10 of max(1, |value|max) of sens_ref at the step's final set; dX_0 = I, du0 = dU_0 and
    pinned rows exactly 0."""
    worst = 0.0
    for d in (d for d in _case(oracle, step_emu, N) if d["set_finish"]):
        du0, dU, dX = d["s"][6:]
        r0, rU, rX = sens_ref(d["qp"], d["A"])
        worst = _held(du0, r0, scale(rU), "du0", N, d, worst)
        worst = _held(dU, rU, scale(rU), "dU", N, d, worst)
        worst = _held(dX, rX, scale(rX), "dX", N, d, worst)
        assert np.array_equal(dX[0], np.eye(10)) and np.array_equal(du0, dU[0]) and not dU[d["A"] != 0].any()
    print(f"N={N}: level-2 sensitivities, worst distance {worst:.3e}")


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_emulated_parameter_sensitivities_at_the_edge_horizons(oracle, step_emu, N):
    """psens_out: du0/dxr, du0/dur, du0/df within 1e-10 of max(1, |J|max) of psens_ref; stage 0's reference rows, f_N and pinned stage-0
    rows exactly 0."""
    worst = 0.0
    for d in (d for d in _case(oracle, step_emu, N) if d["set_finish"]):
        got = d["p"][7:]
        for x, r, what in zip(got, psens_apply(d["sys"]), ("dxr", "dur", "df")):
            worst = _held(x, r, scale(r), what, N, d, worst)
        dxr, dur, df = got
        assert not dxr[:, 0].any() and not df[:, N].any()
        p0 = d["A"][0] != 0
        assert not dxr[p0].any() and not dur[p0].any() and not df[p0].any()
    print(f"N={N}: parameter sensitivities, worst distance {worst:.3e}")


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_emulated_adjoint_and_model_gradient_at_the_edge_horizons(oracle, step_emu, N):
    """vjp_out<true>: gx0, gxr, gur, gf within 1e-10 of max(1, |g|max) of vjp_ref and gmodel of model_grad_ref (its two step sizes in
    1 / m agree to 1e-9); stage 0's reference row, f_N and pinned rows exactly 0; gmodel[6] and gmodel[15] exactly 0."""
    worst = worst_m = 0.0
    for d in (d for d in _case(oracle, step_emu, N) if d["set_finish"]):
        got, gm = d["a"][6:10], d["a"][10]
        ref = vjp_apply(d["sys"], *d["g"])
        s = max(scale(r) for r in ref)
        for x, r, what in zip(got, ref, ("gx0", "gxr", "gur", "gf")):
            worst = _held(x, r, s, what, N, d, worst)
        assert not got[1][0].any() and not got[3][N].any() and not got[2][d["A"] != 0].any()
        rm, rm2 = d["gm"]
        assert abs(rm[14] - rm2) <= 1e-9 * scale(rm)
        worst_m = _held(gm, rm, scale(rm), "gmodel", N, d, worst_m)
        assert gm[6] == 0.0 and gm[15] == 0.0
    print(f"N={N}: adjoint, worst distance {worst:.3e}; model gradient {worst_m:.3e}")


def test_the_model_gradient_leaves_the_adjoint_outputs_bit_equal(step_emu):
    """vjp_out<true> against vjp_out at N = 17 (the inputs' second chunk) and N = 21 (the force's): the same four outputs, bit for bit."""
    from tests.emu import emu
    for N in (17, 21):
        b = synth.make_batch(1, N=N, seed=synth.SEED0 + 40, **MIXED)
        cfg = emu.default_cfg(N=N, use_fd=True)
        rng = np.random.default_rng(600 + N)
        X, U, act = _tape(b, 0, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32)
        g = (rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4)))
        a = _vjp(step_emu, cfg, b["x0"][0], b["xr"][0], b["ur"][0], f, X, U, act, *g, model=True)
        p = _vjp(step_emu, cfg, b["x0"][0], b["xr"][0], b["ur"][0], f, X, U, act, *g)
        assert a[3] == 0 and all(np.array_equal(x, y) for x, y in zip(a[:10], p))


def _duality(d, worst=0.0):
    """<gz, JVP(t)> against <VJP(gz), t> per direction, of the larger side's magnitude (the largest |term|, at least 1)."""
    gu0, gX, gU = d["g"]
    for k in range(T):
        du0, dX, dU = (v[k] for v in d["j"][6:])
        lhs = [gu0 * du0, gX * dX, gU * dU]
        rhs = [g * t[k] for g, t in zip(d["a"][6:10], d["tan"])]
        mag = max(1.0, max(np.abs(x).max() for x in lhs + rhs))
        worst = max(worst, abs(sum(x.sum() for x in lhs) - sum(x.sum() for x in rhs)) / mag)
    return worst


@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_emulated_forward_mode_and_duality_at_the_edge_horizons(oracle, step_emu, N):
    """jvp_out with T = 2 directions in all four tangents: du0, dX, dU within 1e-10 of max(1, |z'|max) of jvp_apply (its two step sizes
    in the attitude reference agree to 1e-9); dX_0 = tx0 and du0 = dU_0 exactly, pinned rows of dU exactly 0; and on every instance
    <gz, JVP(t)> = <VJP(gz), t> against the adjoint of the same tape within 1e-11."""
    worst = gap = 0.0
    for d in _case(oracle, step_emu, N):
        gap = _duality(d, gap)
        if not d["set_finish"]:
            continue
        du0, dX, dU = d["j"][6:]
        for k in range(T):
            r0, rX, rU, dz2 = jvp_apply(d["sys"], *(t[k] for t in d["tan"]))
            s = max(scale(rX), scale(rU))
            assert np.max(np.abs(np.concatenate([rX.ravel(), rU.ravel()]) - dz2)) <= 1e-9 * s
            for x, r, what in zip((du0[k], dX[k], dU[k]), (r0, rX, rU), ("du0", "dX", "dU")):
                worst = _held(x, r, s, what, N, d, worst)
            assert np.array_equal(dX[k, 0], d["tan"][0][k]) and np.array_equal(du0[k], dU[k, 0]) and not dU[k][d["A"] != 0].any()
    print(f"N={N}: forward mode, worst distance {worst:.3e}; duality gap {gap:.3e}")
    assert gap <= DUALITY_BAR, (N, gap)


@pytest.mark.parametrize("N", [3, 4])
def test_interior_point_finishes_either_side_of_the_sweep_switch(oracle, step_emu, N):
    """qp_mode 1 with the velocity box shrunk to +-3 at N = 3 (the plain sweep after the interior point: 14 N + 10 = 52) and N = 4 (the LDL
    sweep: 66): every instance finishes in the interior-point loop with status 0, the adjoint's and forward mode's outputs are finite,
    duality holds within 1e-11 (both solve one system, the last Newton system's), pinned rows of dU are exactly 0.  The distance from
    the dense reference with the active bounds pinned is the barrier smoothing (1e-3 at worst): printed, not held."""
    from tests.emu import emu
    from tests.fixed_set_ref import NU, NX
    assert ldl_after_interior_point(N) == (N == 4)
    n = 4
    b = synth.make_batch(n, N=N, seed=synth.SEED0 + 70 + N, **MIXED)
    cfg = emu.default_cfg(N=N, use_fd=True, qp_mode=1)
    ocfg = oracle.default_cfg(N=N, use_fd=True)
    for c in (cfg, ocfg):
        for j in range(3):
            c.lbv[j], c.ubv[j] = -3.0, 3.0
    rng = np.random.default_rng(700 + N)
    gap = dist = 0.0
    for i in range(n):
        X, U, act = _tape(b, i, rng, N)
        f = rng.normal(0.0, 0.3, (N + 1, 3)).astype(np.float32)
        tan = (rng.normal(size=(T, 10)), rng.normal(size=(T, N + 1, 10)), rng.normal(size=(T, N, 4)), rng.normal(size=(T, N + 1, 3)))
        g = (rng.normal(size=4), rng.normal(size=(N + 1, 10)), rng.normal(size=(N, 4)))
        args = (cfg, b["x0"][i], b["xr"][i], b["ur"][i], f, X, U, act)
        a = _vjp(step_emu, *args, *g, model=True)
        j = _jvp(step_emu, *args, *tan)
        assert all(np.array_equal(x, y) for x, y in zip(a[:6], j[:6]))
        assert j[3] == 0 and (j[4] & 0xffff) > 0, (i, j[3], j[4])
        assert all(np.isfinite(v).all() for v in a[6:] + j[6:])
        A = j[5].reshape(N, 4)
        assert not j[8][:, A != 0].any() and not a[8][A != 0].any()
        assert np.array_equal(j[7][:, 0], tan[0]) and np.array_equal(j[6], j[8][:, 0])
        gap = _duality(dict(g=g, tan=tan, a=a, j=j), gap)
        # the barrier smoothing, for the record: the bounds active at the solution (within 1e-6) pinned in the reference
        Xn, Un = j[1].reshape(N + 1, NX), j[2].reshape(N, NU)
        f64 = f.astype(np.float64)
        qp = oracle.linearize(ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64, X, U)
        pins = []
        for lo, hi, val, n0, off, tag in ((cfg.lbu, cfg.ubu, Un, 0, (N + 1) * NX, "u"), (cfg.lbv, cfg.ubv, Xn[:, 3:6], 1, 3, "v")):
            for k in range(n0, val.shape[0]):
                for c in range(val.shape[1]):
                    up, dn = abs(val[k, c] - hi[c]) < 1e-6, abs(val[k, c] - lo[c]) < 1e-6
                    if up or dn:
                        v = off + NU * k + c if tag == "u" else k * NX + off + c
                        pins.append((v, float(qp[("u" if up else "l") + tag][k, c])))
        _, rX, rU, _ = jvp_apply(jvp_system(oracle, ocfg, b["x0"][i], b["xr"][i], b["ur"][i], f64, X, U, None, pin_v=pins),
                                 *(t[0] for t in tan))
        dist = max(dist, max(np.max(np.abs(j[7][0] - rX)), np.max(np.abs(j[8][0] - rU))) / max(scale(rX), scale(rU)))
    print(f"N={N}: interior-point finishes, duality gap {gap:.3e}; distance from the pinned dense reference {dist:.3e} (not held)")
    assert gap <= DUALITY_BAR, (N, gap)


# ---------------------------------------------------------------- what the device module rests on
@pytest.mark.parametrize("N", DERIV_EDGE_N)
def test_the_device_seeds_give_pinned_and_free_set_finishes_by_the_twin(oracle, mlp_blob, N):
    """SEEDS[N] of the device module, by the reference alone: the oracle's twin of the warm-up and the recorded step finishes at least 6
    of the 37 instances in the active set, at least MIN_PINNED[N] of them with an input on a bound -- with the supplied force, and (fusable
    horizons: the parameter sensitivities' fused engine) with the oracle's downwash network's, there with one instance to spare on each
    count: the device's network differs from the oracle's by 1e-5, which may move an instance that sits on the edge of a bound."""
    fused = K.geometry(N)[1]
    b, f = device_case(N, G.SEEDS[N], fused)
    ok, pinned = twin_finishes(oracle, N, b, f)
    assert ok.sum() >= 6 and pinned.sum() >= G.MIN_PINNED[N], (N, int(ok.sum()), int(pinned.sum()))
    if fused:
        fo = oracle.downwash_batch(mlp_blob, b["other"], b["xr"], b["ego_xy"])
        ok, pinned = twin_finishes(oracle, N, b, fo)
        assert ok.sum() >= 7 and pinned.sum() >= 3, (N, int(ok.sum()), int(pinned.sum()))
    assert set(G.SEEDS) == set(G.MIN_PINNED) == set(DERIV_EDGE_N)
    assert all(v == 2 for v in G.MIN_PINNED.values())


@pytest.mark.parametrize("what,N", [("LOWERED", k[0]) for k in G.LOWERED] + [("POINTERS", N) for N in G.POINTERS])
def test_the_small_device_batches_are_all_set_finishes_by_the_twin(oracle, what, N):
    """The lowered-waves cases (B = 5) and the optional-pointer cases (B = 8) of the device module, by the reference alone: the oracle's
    twin finishes every instance with status 0 in the active set (so bit equality there compares numbers and linearity is held to one
    bar on all of them), at least one of them with an input on a bound."""
    seed, B = (next(v for k, v in G.LOWERED.items() if k[0] == N), G.LOWERED_B) if what == "LOWERED" else (G.POINTERS[N], G.POINTERS_B)
    b, f = small_case(N, seed, B)
    assert b["x0"].shape[0] == B and f.shape[0] == B
    ok, pinned = twin_finishes(oracle, N, b, f)
    assert ok.all() and pinned.any(), (what, N, ok, pinned)


def _params(test):
    """The argument values of a test's parametrize marks, by argument names."""
    return {m.args[0]: list(m.args[1]) for m in getattr(test, "pytestmark", []) if m.name == "parametrize"}


def test_every_recompute_kernel_has_a_device_case_at_every_wave_count_it_reaches():
    """RECOMPUTE_CASES of the device module: the eight recompute kernels (rti_vjp_kernel, rti_wvjp_kernel, rti_jvp_kernel, rti_mjvp_kernel,
    each for N = 20 and for the run-time horizon) at every instances-per-workgroup count ndp_create gives their horizons -- N = 20: 4, and
    2 under NDP_DEV_WAVES; the run-time horizons: 4 (N <= 19), 2 (N = 21..27), and 1 under NDP_DEV_WAVES -- each with a test that exists,
    in the device module or (rti_mjvp_kernel's reference rows) in tests/test_step_model_jvp_edges_gpu.py."""
    import importlib
    M = importlib.import_module(G.MJVP_MODULE)
    recompute = ("rti_vjp_kernel", "rti_wvjp_kernel", "rti_jvp_kernel", "rti_mjvp_kernel")
    kernels = [f"{k}<{nc}>" for k in recompute for nc in (20, 0)]
    want = {(k, w) for k in kernels for w in ((4, 2) if k.endswith("<20>") else (4, 2, 1))}
    assert set(G.RECOMPUTE_CASES) == want, (want - set(G.RECOMPUTE_CASES), set(G.RECOMPUTE_CASES) - want)
    assert len(kernels) == 8 and len(want) == 20
    where = {name: (M if k.startswith("rti_mjvp_kernel<0>") and w > 1 else G) for (k, w), name in G.RECOMPUTE_CASES.items()}
    assert sum(mod is M for mod in where.values()) == 1                   # (the two reference rows of rti_mjvp_kernel<0>: one test)
    missing = {name for name, mod in where.items() if not (name.startswith("test_") and callable(getattr(mod, name, None)))}
    assert not missing, missing
    assert K.geometry(20)[0] == 4 and {K.geometry(N)[0] for N in DERIV_EDGE_N if N < 20} == {4}
    assert {K.geometry(N)[0] for N in DERIV_EDGE_N if N > 20} == {2}
    # the horizons the rows rest on: the reference tests run the whole list (<0> at 4 and at 2), the lowered-waves test <20> at 2 against 4
    # and <0> at 1 against 4 and against 2, and the older modules hold <20> at its default 4 to the dense references
    for name in set(G.RECOMPUTE_CASES.values()) - {"test_lowered_waves_equal_the_default_launch_bit_for_bit"}:
        assert tuple(_params(getattr(where[name], name))["N"]) == DERIV_EDGE_N, name
    assert M.pytestmark.name == "gpu" and M.SEEDS is G.SEEDS
    assert _params(G.test_lowered_waves_equal_the_default_launch_bit_for_bit)["N,waves"] == [(20, 2), (13, 1), (27, 1)] == list(G.LOWERED)
    assert (G.LOWERED_B, G.POINTERS_B, list(G.POINTERS)) == (5, 8, [20, 17])
    from tests import test_model_grad_gpu, test_step_jvp_gpu, test_step_model_jvp_gpu, test_step_vjp_gpu
    for test in (test_step_vjp_gpu.test_full_trajectory_upstream_matches_the_dense_reference,
                 test_model_grad_gpu.test_device_model_gradient_matches_the_dense_reference,
                 test_step_jvp_gpu.test_three_directions_match_the_dense_reference,
                 test_step_model_jvp_gpu.test_three_directions_match_the_dense_reference):
        assert 20 in _params(test)["N"], test.__name__
    from ndp_nmpc_qd_amd import _lib, build, isa_inspect
    build.build()
    names = [n for n in isa_inspect.CodeObject(_lib.LIB_PATH).kernels() if any(k in n for k in recompute)]
    assert len(names) == 8, names
