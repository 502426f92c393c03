"""BASELINE configs[4] as worded -- "fp32 vs bf16 MFMA on the CONDENSED QP" -- the study modes qp_precision 5 / 6 (csrc/cond_qp.hpp):
every QP's first solve in condensed form on v_mfma_f32_16x16x4_f32 / v_mfma_f32_16x16x16_bf16 with an fp32 Cholesky in LDS, kept when
it passes the fp64 inside-the-box and stationarity tests, the fp64 Riccati path otherwise.  (VERDICT r5, row +: the study that had not been run.)
The reference does not condense (qp_solver_cond_N = N, nmpc_body_rate_ctl.py:79); the oracle here is the fp64 restatement at a tight
tolerance, and the fp64 product engine on the same inputs."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ndp():
    import ndp_nmpc_qd_amd
    return ndp_nmpc_qd_amd


def _err(u, uo):
    return np.max(np.abs(u - uo) / np.maximum(1.0, np.abs(uo)), axis=1)


@pytest.mark.parametrize("N,n_rti,B", [(20, 1, 96), (40, 2, 48)])
def test_condensed_modes_against_the_fp64_path(ndp, oracle, N, n_rti, B):
    """Nominal starts (no bound in play).  fp32: every instance keeps its condensed result, status 0, and the result is an fp32-condensed
    answer -- 1e-7 .. 5e-3 from the fp64 one (the condensed Hessian's conditioning, not the instruction, costs the digits: the same
    instruction on the UNcondensed sweeps holds 2e-7, qp_precision 3).  bf16: further off, or rejected and solved in fp64 -- never a bad
    status, and an instance that did not keep a condensed result has the fp64 engine's answer."""
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 5)
    cfgo = oracle.default_cfg(N=N, n_rti=n_rti)
    cfgo.tol = 1e-11
    Xo, Uo = b["xr"].copy(), b["ur"].copy()
    uo, sto, _ = oracle.step_batch(cfgo, b["x0"], b["xr"], b["ur"], None, Xo, Uo)
    assert not sto.any()
    ref = ndp.BatchedNMPC(B, N=N, n_rti=n_rti)
    ref.reset(b["xr"], b["ur"])
    u64 = ref.update(b["x0"], b["xr"], b["ur"])
    assert _err(u64, uo).max() < 1e-9
    res = {}
    for prec in (5, 6):
        eng = ndp.BatchedNMPC(B, N=N, n_rti=n_rti, qp_precision=prec)
        eng.reset(b["xr"], b["ur"])
        u0 = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)
        st, it = eng.status()
        kept = eng.condensed_kept()
        assert not st.any() and not it.any(), (prec, np.bincount(st))
        res[prec] = (_err(u0, uo), kept, u0)
        eng.close()
    e5, k5, _ = res[5]
    assert (k5 == n_rti).all()
    assert 1e-7 < np.median(e5) < 1e-3 and e5.max() < 5e-3, (np.median(e5), e5.max())
    e6, k6, u6 = res[6]
    if n_rti == 1:
        none = k6 == 0
        if none.any():
            np.testing.assert_allclose(u6[none], u64[none], rtol=0, atol=1e-9)      # rejected: the fp64 path's answer
    both = k6 == n_rti
    if both.any():
        assert np.median(e6[both]) > np.median(e5)                                   # bf16 operands: worse than fp32 -- where the bf16
    assert np.isfinite(u6).all()                                                     # Hessian is positive definite at all (N = 40: never;
    if N == 40:                                                                      # N = 20: a sixth of the instances, errors up to O(1)
        assert not k6.any() and e6.max() < 1e-9                                      # -- those are not kept: their fp64 stationarity
    assert e6.max() < 0.05, e6.max()                                                 # residual fails, rti_wave.hpp: cond_stationarity)


def test_bounds_in_play_fall_back_to_the_fp64_path(ndp, oracle):
    """Perturbed starts (a fifth of the instances end on an input bound): a condensed result outside the box is never the step -- the
    active set / interior-point course runs in fp64 as in the product engine: same status, and (where no QP kept a condensed result)
    the same answer to 1e-9; where one was kept, the fp32-condensed accuracy."""
    B, N = 128, 20
    b = synth.make_batch(B, N=N, seed=synth.SEED0 + 40, pos_sigma=0.5, vel_sigma=1.0, quat_sigma=0.15)
    ref = ndp.BatchedNMPC(B, N=N)
    ref.reset(b["xr"], b["ur"])
    u64 = ref.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)
    st64, _ = ref.status()
    sw64, act64 = ref.active_set()
    eng = ndp.BatchedNMPC(B, N=N, qp_precision=5)
    eng.reset(b["xr"], b["ur"])
    u0 = eng.update(b["x0"], b["xr"], b["ur"], raise_on_status=False)
    st, _ = eng.status()
    kept = eng.condensed_kept()
    sw, act = eng.active_set()
    assert np.array_equal(st, st64) and not st.any()
    con = act64.any(axis=(1, 2))
    assert con.mean() > 0.1 and not kept[con].any()                # constrained instances: solved in fp64 with the pins
    assert np.array_equal(act[con], act64[con])
    np.testing.assert_allclose(u0[kept == 0], u64[kept == 0], rtol=0, atol=1e-9)
    free = kept == 1
    assert free.mean() > 0.5 and _err(u0[free], u64[free]).max() < 5e-3


def test_shapes_the_study_does_not_tile_are_refused(ndp):
    for kw in (dict(N=18, qp_precision=5), dict(N=44, qp_precision=6)):
        with pytest.raises(ndp.NdpError, match="multiple of 4"):
            ndp.BatchedNMPC(4, **kw)
