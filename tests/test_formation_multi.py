"""Downwash from several neighbours without a GPU: the CPU reference loop on stacked triples (tests/formation_multi_ref.py) shows what
hearing every neighbour buys over hearing one, the loop's own sensitivity to network error is measured (the device tests' position bar
rests on it), and the binding's prototypes of the new entry points agree with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib
from tests import formation_multi_ref as M
from tests import formation_ref as F


@pytest.mark.parametrize("dz", [0.5, 0.75])
def test_cpu_loop_hearing_every_neighbour_holds_its_height(oracle, dz):
    """2 triples, 200 ticks, z-RMSE over ticks 50 onward, the lowest vehicle of every triple: hearing all slots it is at most a third of
    hearing slot 0 only and at most a fifth of the blind one; every status is 0; no slot comes near its gate's rim."""
    r = M.reference(dz)
    rmse = {m: F.z_rmse(r[m][0], r["xr"])[0::3] for m in M.MODES}
    peak = np.abs(r["blind"][2][:, 0::3, 2]).max()
    dist = {m: M.max_slot_distance(r[m][0], r["tr"]["other_index"]) for m in M.MODES}
    print(f"dz {dz}: lowest vehicle z-RMSE blind {rmse['blind']}, slot 0 only {rmse['slot0']}, all slots {rmse['all']}; "
          f"peak |f_z| on it {peak:.2f} N; largest slot distance {dist}")
    for m in M.MODES:
        assert not r[m][3].any(), m
    assert np.all(rmse["all"] <= rmse["slot0"] / 3.0), (rmse["all"], rmse["slot0"])
    assert np.all(rmse["all"] <= rmse["blind"] / 5.0), (rmse["all"], rmse["blind"])
    assert peak > 1.0                                                         # newtons, not noise
    for m in M.MODES:
        assert dist[m] <= 0.9 * F.DP.r_horiz, (m, dist[m])


@pytest.mark.parametrize("dz", [0.5, 0.75])
def test_cpu_loop_sensitivity_to_network_error(oracle, dz):
    """Every per-slot network output perturbed inside the project's network bar, three draws: the closed loop moves by micrometres to
    tens of micrometres -- measurably more with compensation than blind, which is why the device rollout's position bar is taken per
    (mode, dz) from this probe and not from the single-neighbour rollout's figure."""
    s = M.sensitivity(dz)
    print(f"dz {dz}: worst position difference under +-{M.NET_BAR} * max(1, |f|) noise: {s}")
    for m in M.MODES:
        assert 0.0 < s[m] < 1e-3, (m, s[m])                                   # the noise does act, and the loop does not amplify it to millimetres
    assert s == M.sensitivity(dz)                                             # seeded: the bar is the same in every session


def test_summed_force_and_prediction_are_slot_ordered_sums(oracle, mlp_blob):
    """K = 1 reduces to formation_ref's single-neighbour pieces; an empty slot adds exactly nothing; a duplicate counts twice."""
    r = M.reference(0.5)
    tr, xr = r["tr"], r["xr"][3]
    x = r["all"][0][10]
    idx = tr["other_index"]
    f0, f1 = (F.true_force(mlp_blob, x, idx[:, k]) for k in (0, 1))
    assert np.array_equal(M.true_force_multi(mlp_blob, x, idx[:, :1]), f0)
    assert np.array_equal(M.true_force_multi(mlp_blob, x, idx), f0 + f1)
    hole = np.stack([idx[:, 0], np.full(len(idx), -1, np.int32), idx[:, 1]], axis=1)
    assert np.array_equal(M.true_force_multi(mlp_blob, x, hole), f0 + f1)
    assert np.array_equal(M.true_force_multi(mlp_blob, x, idx[:, [0, 0]]), f0 + f0)
    xy = x[:, 0:2].copy()
    p0, p1 = (M.oracle_prediction(mlp_blob, xr, idx[:, k], xy) for k in (0, 1))
    assert np.array_equal(M.prediction_multi(mlp_blob, xr, idx[:, :1], xy), p0)
    assert np.array_equal(M.prediction_multi(mlp_blob, xr, idx, xy), p0 + p1) and (p0 + p1).dtype == np.float32
    assert np.array_equal(M.prediction_multi(mlp_blob, xr, hole, xy), p0 + p1)


def test_binding_prototypes_match_the_header():
    hdr = open(os.path.join(M.ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    scalars = {"int": C.c_int, "double": C.c_double}
    for name in ("ndp_downwash_multi", "ndp_downwash_multi_device", "ndp_plant_force_multi", "ndp_plant_force_multi_device",
                 "ndp_rollout_formation_multi_device"):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        want = [C.c_void_p if "*" in p else scalars[p.split()[0]] for p in params]
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == want, (name, params)
    assert _lib.MAX_NEIGH == int(re.search(r"#define NDP_MAX_NEIGH\s+(\d+)", hdr).group(1)) == 8
    from ndp_nmpc_qd_amd.batched import BatchedNMPC
    for name in ("downwash_multi", "downwash_multi_device", "plant_force_multi", "plant_force_multi_device", "rollout_formation_multi_device"):
        assert callable(getattr(BatchedNMPC, name))


def test_new_kernels_have_no_scratch_and_the_prediction_parks_its_weights():
    """The shipped binary: both multi-neighbour kernels without scratch or spill; mlp_multi_kernel runs the network's matrix instructions
    once in its code (the slots are a rolled loop around the tile, not K copies of it) -- as many as mlp_kernel has."""
    from ndp_nmpc_qd_amd import build, isa_inspect
    build.build()
    co = isa_inspect.CodeObject(_lib.LIB_PATH)
    ks = co.kernels()
    names = {k: [n for n in ks if f"ndp{len(k)}{k}" in n] for k in ("mlp_multi_kernel", "plant_force_multi_kernel", "mlp_kernel", "plant_force_kernel")}
    for k, v in names.items():
        assert len(v) == 1, (k, v)
    mfma = {}
    for k, (n,) in names.items():
        m = ks[n]
        mfma[k] = sum(s.startswith("v_mfma") for s in co.disassemble(n))
        print(f"{k}: {m['vgpr']} VGPR, {m['agpr']} AGPR, {m['sgpr']} SGPR, scratch {m['scratch']}, spill {m['spill']}, "
              f"{mfma[k]} matrix instructions")
        assert m["scratch"] == 0 and m["spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
    assert mfma["mlp_multi_kernel"] == mfma["mlp_kernel"] == 12 + 3 * 32
    assert mfma["plant_force_multi_kernel"] == mfma["plant_force_kernel"] == 12 + 3 * 32
