"""The formation rollout without a GPU: the CPU reference loop (tests/formation_ref.py) reproduces the paper's effect -- a controller that
predicts the downwash holds its height under a neighbour, the blind one does not -- and the binding's prototypes of the three new entry
points agree with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ndp_nmpc_qd_amd import _lib
from tests import formation_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dz", [0.5, 1.0])
def test_cpu_reference_loop_reproduces_the_downwash_effect(oracle, dz):
    """4 pairs, 200 ticks, z-RMSE over ticks 50 onward: the lower vehicle's NDP error is at most a fifth of its NMPC error (these pairs:
    0.33 m against 0.005-0.022 m at dz = 0.5, 0.43 m against 0.004-0.008 m at dz = 1.0 -- 15x at the least), every status is 0, and the
    force it flies through is newtons, not noise."""
    r = F.reference(dz)
    nmpc, ndp = F.z_rmse(r["nmpc"][0], r["xr"]), F.z_rmse(r["ndp"][0], r["xr"])
    print(f"dz {dz}: lower NMPC {nmpc[0::2]}, lower NDP {ndp[0::2]}, upper NMPC {nmpc[1::2]}, upper NDP {ndp[1::2]}, "
          f"peak |f| {np.abs(r['nmpc'][2]).max():.2f} N")
    assert not r["nmpc"][3].any() and not r["ndp"][3].any()
    assert np.all(ndp[0::2] <= nmpc[0::2] / 5.0), (ndp[0::2], nmpc[0::2])
    assert np.abs(r["nmpc"][2][:, 0::2, 2]).max() > 1.0
    # stacked pairs: every gate stays open with half of r_horiz to spare, in either run (the blind vehicle drifts ~0.3 m sideways in the
    # wash: the force has horizontal components), so no comparison against this loop can meet a gate flip
    for run in (r["nmpc"], r["ndp"]):
        d = run[0][:, 0::2, 0:2] - run[0][:, 1::2, 0:2]
        assert np.sqrt((d * d).sum(-1)).max() < 0.5 * F.DP.r_horiz


def test_binding_prototypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "ndp_nmpc.h")).read()
    lib = _lib.load()
    scalars = {"int": C.c_int, "double": C.c_double}
    for name in ("ndp_plant_force", "ndp_plant_force_device", "ndp_rollout_formation_device"):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        want = [C.c_void_p if "*" in p else scalars[p.split()[0]] for p in params]
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == want, (name, params)
    assert (_lib.FORM_GATE, _lib.FORM_COMPENSATE) == tuple(int(re.search(r"#define NDP_FORM_" + n + r"\s+(\d+)", hdr).group(1))
                                                           for n in ("GATE", "COMPENSATE"))
    assert _lib.ABI_VERSION == int(re.search(r"#define NDP_ABI_VERSION (\d+)", hdr).group(1)) == 9
