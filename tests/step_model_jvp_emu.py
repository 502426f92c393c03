"""Forward mode of the control step along directions of the cost weights and the mass on the host wave emulator
(tests/step_model_jvp_emu.cpp): the shim, compiled once per pytest session into a temporary directory, and its wrapper, in the pattern of
tests/step_deriv_emu.py (whose _step marshals the call)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.step_deriv_emu import _step

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


@pytest.fixture(scope="session")
def model_jvp_emu(tmp_path_factory):
    global _lib                         # (a module that imports the fixture gets a definition of its own: compile for the first only)
    if _lib is None:
        so = str(tmp_path_factory.mktemp("step_model_jvp_emu") / "libstep_model_jvp_emu.so")
        subprocess.check_call(["g++", "-O2", "-fPIC", "-std=c++17", "-shared", "-o", so, os.path.join(HERE, "step_model_jvp_emu.cpp")])
        _lib = C.CDLL(so)
        _lib.mjvp_emu_step.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 18
    return _lib


def _mjvp(lib, cfg, x0, xr, ur, f, X, U, act, tmodel, tx0=None, txr=None, tur=None, tf=None):
    """T directions: tmodel [T,16] and the data tangents ([T, ...] each, None = 0).  Returns (u0, X, U, status, iteration word, act) after the
    step, then (du0 [T,4], dX [T,N+1,10], dU [T,N,4]), which start filled with -7.0."""
    N = cfg.N
    tmodel = np.ascontiguousarray(tmodel, dtype=np.float64)
    T = tmodel.shape[0]
    assert tmodel.shape == (T, 16)
    tans = tuple(None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (tx0, txr, tur, tf))
    assert all(a is None or a.shape[0] == T for a in tans)
    out = np.full((T, 4), -7.0), np.full((T, N + 1, 10), -7.0), np.full((T, N, 4), -7.0)
    return _step(lib.mjvp_emu_step, cfg, (T,), x0, xr, ur, f, X, U, act, tans + (tmodel,) + out) + out
