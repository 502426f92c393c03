"""The control step's forward-mode derivative on the host wave emulator (tests/step_jvp_emu.cpp): the shim, compiled once per pytest session
into a temporary directory, and its Python wrapper, in tests/step_deriv_emu.py's conventions (a tape in, copied; outputs start at -7.0)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.step_deriv_emu import HERE, _step

_lib = None


@pytest.fixture(scope="session")
def jvp_emu(tmp_path_factory):
    global _lib
    if _lib is None:
        so = str(tmp_path_factory.mktemp("step_jvp_emu") / "libstep_jvp_emu.so")
        subprocess.check_call(["g++", "-O2", "-fPIC", "-std=c++17", "-shared", "-o", so, os.path.join(HERE, "step_jvp_emu.cpp")])
        _lib = C.CDLL(so)
        _lib.jvp_emu_step.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 17
        _lib.vjp_emu_step.argtypes = [C.c_void_p] * 18
    return _lib


def _jvp(lib, cfg, x0, xr, ur, f, X, U, act, tx0=None, txr=None, tur=None, tf=None):
    """The tangents' T directions ([T, ...] each, None = 0): (u0, X, U, status, iteration word, act) + (du0 [T,4], dX [T,N+1,10], dU [T,N,4])."""
    N = cfg.N
    tans = tuple(None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (tx0, txr, tur, tf))
    T = next(a.shape[0] for a in tans if a is not None)
    assert all(a is None or a.shape[0] == T for a in tans)
    out = np.full((T, 4), -7.0), np.full((T, N + 1, 10), -7.0), np.full((T, N, 4), -7.0)
    return _step(lib.jvp_emu_step, cfg, (T,), x0, xr, ur, f, X, U, act, tans + out) + out
