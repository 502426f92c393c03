"""The models at which the control step and its derivatives are held to references: one table, and one function per consumer that turns a
case into BatchedNMPC keyword overrides (engine_kw), an oracle.OrcCfg (oracle_cfg) or an emulator NdpCfg (emu_cfg) -- all three through
the same `_fields`, so they cannot drift apart.  A case is a dict of the entries it changes: Qd [10], Rd [4], mass, g, lbu [4], ubu [4], dt
-- and ts_nmpc beside a dt that is no whole multiple of the default 0.02 s: ndp_create wants dt = k ts_nmpc (the reference list keeps one
point per ts_nmpc and a window node is every k-th entry).  ts_nmpc is a field of ndp_cfg alone; the oracle has no list.  r_horiz, the
gate's radius, likewise: the oracle takes it as an argument of downwash_batch (radius_of hands it out).

The defaults are restated here as literals (the reference's constants: nmpc_body_rate_ctl.py / params/nmpc_params.py);
tests/test_model_envelope.py checks them against what the library, the oracle and the emulator hand out."""
import numpy as np

QD0 = (300.0, 300.0, 400.0, 10.0, 10.0, 10.0, 0.0, 10.0, 10.0, 100.0)
RD0 = (10.0, 10.0, 10.0, 5.0)
MASS0, G0, DT0 = 1.4844, 9.81, 0.1
R_HORIZ0 = 1.0
ENGINE_ONLY = ("ts_nmpc", "r_horiz")                            # fields of ndp_cfg that OrcCfg does not have
LBU0, UBU0 = (-6.0, -6.0, -6.0, 0.0), (6.0, 6.0, 6.0, 9.81 / 0.36)

_rng = np.random.default_rng(20231213 + 7000)                   # `tuned`: one seeded draw, made at import, never again
_TUNED_Q, _TUNED_R = _rng.uniform(0.5, 2.0, 10), _rng.uniform(0.5, 2.0, 4)
_ASYM = dict(lbu=[-2.0, -6.0, -0.75, 3.0], ubu=[5.0, 1.5, 4.0, 14.0])
_DISTINCT = dict(Qd=[120.0, 310.0, 540.0, 4.0, 11.0, 23.0, 7.0, 3.0, 17.0, 61.0], Rd=[3.0, 8.0, 21.0, 13.0], mass=0.9)

CASES = {
    "default": {},
    "tuned": dict(Qd=list(np.array(QD0) * _TUNED_Q), Rd=list(np.array(RD0) * _TUNED_R), mass=MASS0 * 1.1),
    "distinct": dict(_DISTINCT),                                # no two weights equal, Qd[6] != 0
    "asym_box": dict(_ASYM),
    "zero_w": dict(Qd=list(QD0[:3]) + [0.0] * 7),               # velocity and attitude unweighted: a singular stage Q
    "qd6": dict(Qd=[123.0 if i == 6 else q for i, q in enumerate(QD0)]),
    "light_lowg": dict(mass=0.6, g=7.0),
    "dt005": dict(dt=0.05, ts_nmpc=0.01),
    "dt02": dict(dt=0.2),
    "stiff": dict(Qd=list(np.array(QD0) * [100, 100, 100, 1, 1, 1, 1, 50, 50, 50]), Rd=list(np.array(RD0) * 0.05)),
}
# the derivative cases' first model: distinct weights and mass with the asymmetric box, dt 0.05 and g 7.0 together
DERIV_CASES = {"distinct": dict(_DISTINCT, **_ASYM, dt=0.05, ts_nmpc=0.01, g=7.0), "zero_w": CASES["zero_w"]}
# the plant side and the closed loop (tests/plant_side_cases.py): the models whose mass and g reach the plant's derivatives, and the
# closed loop's -- distinct weights and mass with the asymmetric box and g 7.0 at the default dt (the one call's windows are 0.1 s apart)
PLANT_CASES = {"light_lowg": CASES["light_lowg"], "m09": dict(mass=0.9)}
LOOP_CASE = dict(_DISTINCT, **_ASYM, g=7.0)
# gate radii whose squares, 0.5625 and 2.25, are exact in binary: d^2 == r^2 can be met exactly, as at r = 1
RADII = (0.75, 1.5)


def _fields(case, gravity_name):
    """The case's entries under the names of a cfg struct that calls gravity `gravity_name`."""
    unknown = set(case) - {"Qd", "Rd", "mass", "g", "lbu", "ubu", "dt", "ts_nmpc", "r_horiz"}
    assert not unknown, unknown
    ndp = gravity_name == "gravity"                             # (ndp_cfg's names; the oracle's OrcCfg says g and has no ts_nmpc or r_horiz)
    return {(gravity_name if k == "g" else k): v for k, v in case.items() if ndp or k not in ENGINE_ONLY}


def _apply(cfg, case, gravity_name):
    for k, v in _fields(case, gravity_name).items():
        if isinstance(v, (list, tuple)):
            arr = getattr(cfg, k)
            assert len(arr) == len(v), k
            for i, x in enumerate(v):
                arr[i] = float(x)
        else:
            setattr(cfg, k, float(v))
    return cfg


def engine_kw(case):
    """BatchedNMPC(batch, N=..., **engine_kw(case))."""
    return {k: (list(v) if isinstance(v, (list, tuple)) else float(v)) for k, v in _fields(case, "gravity").items()}


def oracle_cfg(oracle, case, N=20, n_rti=1, use_fd=False):
    """oracle.default_cfg(N, n_rti, use_fd) at the case's model."""
    return _apply(oracle.default_cfg(N=N, n_rti=n_rti, use_fd=use_fd), case, "g")


def emu_cfg(case, N=20, **kw):
    """tests.emu.emu.default_cfg(N, **kw) at the case's model."""
    from tests.emu import emu
    return _apply(emu.default_cfg(N=N, **kw), case, "gravity")


def radius_of(case):
    """The case's gate radius (downwash_batch's r_horiz argument; the default where the case has none)."""
    return float(case.get("r_horiz", R_HORIZ0))


def model_of(case):
    """(Qd [10], Rd [4], mass, g, lbu [4], ubu [4], dt) of a case as numpy arrays / floats, defaults filled in."""
    g = lambda k, d: np.array(case.get(k, d), dtype=np.float64)  # noqa: E731
    return g("Qd", QD0), g("Rd", RD0), float(case.get("mass", MASS0)), float(case.get("g", G0)), g("lbu", LBU0), g("ubu", UBU0), \
        float(case.get("dt", DT0))
