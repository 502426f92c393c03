"""The control step's derivative code on the host wave emulator (tests/step_deriv_emu.cpp): the shim, compiled once per pytest session into a
temporary directory, and one Python wrapper per entry.  Every wrapper runs one instance's step from a tape (X, U, act: the iterate and
kept set before the step; copied, not touched) and returns (u0, X, U, status, iteration word, act) after the step, then its derivative
outputs, which start filled with -7.0 (what the step leaves alone stays -7.0)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MIXED = dict(pos_sigma=0.5, vel_sigma=1.0, quat_sigma=0.15)
_lib = None


@pytest.fixture(scope="session")
def step_emu(tmp_path_factory):
    global _lib                         # (a module that imports the fixture gets a definition of its own: compile for the first only)
    if _lib is None:
        so = str(tmp_path_factory.mktemp("step_deriv_emu") / "libstep_deriv_emu.so")
        subprocess.check_call(["g++", "-O2", "-fPIC", "-std=c++17", "-shared", "-o", so, os.path.join(HERE, "step_deriv_emu.cpp")])
        _lib = C.CDLL(so)
        _lib.sens_emu_step.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 13
        _lib.psens_emu_step.argtypes = [C.c_void_p] * 15
        _lib.vjp_emu_step.argtypes = [C.c_void_p] * 18
        _lib.wvjp_emu_step.argtypes = [C.c_void_p] * 19
        _lib.jvp_emu_step.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 17
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _tape(b, i, rng, N):
    """A pre-step iterate near the reference (so the linearisation point is not the reference itself) and an empty kept set."""
    return (b["xr"][i] + 0.01 * rng.normal(size=b["xr"][i].shape), b["ur"][i] + 0.01 * rng.normal(size=b["ur"][i].shape),
            np.zeros(4 * N, dtype=np.int8))


def _step(entry, cfg, lead, x0, xr, ur, f, X, U, act, tail):
    """entry(cfg, *lead, x0, xr, ur, f, X, U, u0, status, iters, act, *tail) on a copy of the tape; returns (u0, X, U, st, it, act)."""
    X, U, act = X.copy(), U.copy(), act.copy()
    u0 = np.zeros(4)
    st, it = C.c_int(-1), C.c_int(-1)
    f32 = None if f is None else np.ascontiguousarray(f, dtype=np.float32)
    rc = entry(C.byref(cfg), *lead, _p(x0), _p(xr), _p(ur), _p(f32), _p(X), _p(U), _p(u0), C.byref(st), C.byref(it), _p(act),
               *(_p(a) for a in tail))
    assert rc == 0
    return u0, X, U, st.value, it.value, act


def _emu_step(lib, cfg, level, x0, xr, ur, X, U, act, f=None):
    """Initial-state sensitivities at `level` (f: the step's fp32 force, with use_fd): ... + (du0, dU, dX)."""
    N = cfg.N
    out = np.full((4, 10), -7.0), np.full((N, 4, 10), -7.0), np.full((N + 1, 10, 10), -7.0)
    return _step(lib.sens_emu_step, cfg, (level,), x0, xr, ur, f, X, U, act, out) + out


def _psens(lib, cfg, x0, xr, ur, f, X, U, act):
    """Parameter sensitivities: ... + (du0, dxr, dur, df)."""
    N = cfg.N
    out = np.full((4, 10), -7.0), np.full((4, N + 1, 10), -7.0), np.full((4, N, 4), -7.0), np.full((4, N + 1, 3), -7.0)
    return _step(lib.psens_emu_step, cfg, (), x0, xr, ur, f, X, U, act, out) + out


def _vjp(lib, cfg, x0, xr, ur, f, X, U, act, gu0=None, gX=None, gU=None, model=False):
    """The adjoint for the upstream (gu0, gX, gU): ... + (gx0, gxr, gur, gf), and gmodel [16] behind them with model."""
    N = cfg.N
    up = tuple(None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (gu0, gX, gU))
    out = np.full(10, -7.0), np.full((N + 1, 10), -7.0), np.full((N, 4), -7.0), np.full((N + 1, 3), -7.0)
    if model:
        out += (np.full(16, -7.0),)
    return _step(lib.wvjp_emu_step if model else lib.vjp_emu_step, cfg, (), x0, xr, ur, f, X, U, act, up + out) + out


def _jvp(lib, cfg, x0, xr, ur, f, X, U, act, tx0=None, txr=None, tur=None, tf=None):
    """The tangents' T directions ([T, ...] each, None = 0): ... + (du0 [T,4], dX [T,N+1,10], dU [T,N,4])."""
    N = cfg.N
    tans = tuple(None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (tx0, txr, tur, tf))
    T = next(a.shape[0] for a in tans if a is not None)
    assert all(a is None or a.shape[0] == T for a in tans)
    out = np.full((T, 4), -7.0), np.full((T, N + 1, 10), -7.0), np.full((T, N, 4), -7.0)
    return _step(lib.jvp_emu_step, cfg, (T,), x0, xr, ur, f, X, U, act, tans + out) + out
