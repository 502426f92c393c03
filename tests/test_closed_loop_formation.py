"""The float64 reference of the formation's closed loop (tests/closed_loop_formation_ref.py) without a GPU: the conditions its inputs
must meet, on the oracle's flight; its reverse sweep against central differences of the float64-network flight restarted from the record;
the duality of the scatter; and the reverse lists of ndp_closed_loop_formation_config's rule on a hand-made index.  The device side:
tests/test_closed_loop_formation_gpu.py."""
import numpy as np
import pytest

from tests import closed_loop_chain_ref as R
from tests import closed_loop_formation_ref as C
from tests import mlp_vjp_ref as MV
from tests import plant_force_deriv_ref as PF

FD_BAR = 1e-6            # tests/test_closed_loop_chain.py's
H64, H32 = 1e-6, 2.0 ** -14
CASES = [(2, 20), (22, 20), (2, 7)]          # (triples, N): B = 6, B = 66, and the run-time-horizon run


def referenced(triples):
    """Every vehicle of two triples; of 22: triple 0 and triple 21 (vehicles 63..65, across the 64-lane workgroup boundary)."""
    return list(range(6)) if triples == 2 else [0, 1, 2, 63, 64, 65]


@pytest.mark.parametrize("triples,N", CASES)
def test_the_inputs_meet_their_conditions_on_the_oracle(oracle, triples, N):
    """At every state where the force is evaluated on the oracle's flight: every open slot of a referenced vehicle has margin >=
    mlp_vjp_ref.MARGIN, no slot fails (plant_force_deriv_ref.failing), at least one slot per referenced triple is open, and every
    referenced vehicle is a status-0 set finish.  No row is left out of any comparison: the cap on skipped rows is zero."""
    a = C.inputs(triples, N)
    rec = C.nominal_cpu(oracle, a)
    which = referenced(triples)
    assert sorted(sum((c for c in C.components(a["index"]) if set(c) & set(which)), [])) == which
    c = C.conditions(rec, which)
    print(f"triples {triples}, N {N}: smallest open margin {c['margin']:.2e}, open slots per tick and triple {c['open_per'].tolist()}")
    assert c["margin"] >= MV.MARGIN and c["failing"] == 0
    assert (c["open_per"] >= 1).all() and c["set_finish"].all()
    assert np.abs(rec["fp"][:, which]).max() > 1.0         # (newtons: the coupling is not a rounding matter)


def test_reverse_sweep_matches_central_differences_of_the_restarted_flight(oracle):
    """B = 6, N = 20, L summed over the six vehicles (the index and the weights couple them) with an upstream on the logged force too:
    central differences over the float64-network flight in two entries of x_0 and of every tick's xr, ur and f and in eight weights (one
    per parameter group), every tick of every perturbed run restarted from the nominal record's iterate and kept set, within FD_BAR of
    max(1, |g|); every vehicle keeps its sets and iteration words in every run."""
    a = C.inputs(2, 20)
    blob = np.asarray(a["blob"], dtype=np.float64)
    rec = C.nominal_cpu(oracle, a, net64=True, blob=blob)
    B, N = a["x0"].shape[0], 20
    which = list(range(B))
    assert R.set_finish(rec).all() and C.conditions(rec, which)["failing"] == 0
    G, H, A = R.upstreams(C.K, B, N, seed=5)
    Fu = np.random.default_rng(6).normal(size=(C.K, B, 3))
    g = C.reverse(R.systems(oracle, rec, which), rec, G, H, A, Fu)
    rng = np.random.default_rng(9)
    entries = [("x0", None, (int(rng.integers(0, 6)),)), ("x0", None, (int(rng.integers(6, 10)),))]
    for k in range(C.K):
        for name in ("xr", "ur", "f"):
            shape = a[name][k].shape[1:]
            for _ in range(2):
                at = tuple(int(rng.integers(0, s)) for s in shape)
                if name == "xr" and at[0] == 0:
                    at = (1,) + at[1:]
                entries.append((name, k, at))
    from ndp_nmpc_qd_amd import mlp_frag
    entries += [("w", None, (o + int(rng.integers(0, int(np.prod(s)))),)) for o, s in mlp_frag.offsets().values()]
    stable = np.ones(B, dtype=bool)
    worst = 0.0
    for name, k, at in entries:
        h = H32 if name in ("f", "w") else H64
        L = []
        for sgn in (1.0, -1.0):
            p = dict(a, x0=a["x0"].copy(), xr=a["xr"].copy(), ur=a["ur"].copy(), f=a["f"].astype(np.float64))
            w = blob.copy()
            if name == "w":
                w[at] += sgn * h
            else:
                (p[name] if k is None else p[name][k])[(slice(None),) + at] += sgn * h
            r = C.nominal_cpu(oracle, p, net64=True, restart=rec, blob=w)
            stable &= R.set_finish(r) & (r["act"] == rec["act"]).all(axis=(0, 2, 3))
            L.append(C.loss(r, G, H, A, Fu).sum())
        fd = (L[0] - L[1]) / (2 * h)
        got = g[name] if k is None else g[name][k]
        ref = got[at] if name == "w" else got[(slice(None),) + at].sum()
        err = abs(fd - ref) / max(1.0, abs(ref))
        worst = max(worst, err)
        assert err <= FD_BAR, (name, k, at, fd, ref, err)
    assert stable.all()
    # the coupling is in the gradient: without the scatter x_0's gradient is another (the triples' vehicles do reach each other's loss)
    assert np.abs(g["gz"]).max() > 1e-3 and np.abs(g["w"]).max() > 1e-3
    print(f"{len(entries)} entries, worst |fd - g| / max(1, |g|) = {worst:.2e}")


def test_the_scatter_is_dual_to_the_gather():
    """<scatter(g_z), t_x> = <g_z, t_x[o] - t_x[v]> over the slots with a neighbour, for the reference's scatter and for the ordered
    restatement of the device's (self slots left out: their two shares cancel), on the hand-made index; the two agree to rounding."""
    rng = np.random.default_rng(3)
    for B, Kn in ((65, 3), (9, 3)):
        idx = C.hand_index(B, Kn)
        gz, tx = rng.normal(size=(B, Kn, 6)), rng.normal(size=(B, 10))
        has = (idx >= 0) & (idx < B)
        o = np.where(has, idx, np.arange(B)[:, None])
        rhs = float((gz * (tx[o][..., :6] - tx[:, None, :6]) * has[:, :, None]).sum())
        for gx in (PF.scatter(gz, idx, B), C.scatter_ordered(gz, idx)):
            assert not gx[:, 6:].any()
            assert abs(float((gx * tx).sum()) - rhs) <= 1e-12 * max(1.0, abs(rhs))
        assert np.abs(PF.scatter(gz, idx, B) - C.scatter_ordered(gz, idx)).max() <= 1e-13


def test_the_reverse_lists_of_a_hand_made_index():
    """A hub heard by all, a vehicle heard by none, self slots, -1 and >= B entries, the same index twice in one row: every list is
    ascending, holds exactly the slots that name its vehicle from another one, and the lists partition those slots."""
    B, Kn = 9, 3
    idx = C.hand_index(B, Kn)
    offset, edge = C.reverse_lists(idx)
    assert offset[0] == 0 and (np.diff(offset) >= 0).all() and offset[-1] == len(edge)
    lists = [edge[offset[v]:offset[v + 1]].tolist() for v in range(B)]
    assert lists[0] == [3, 8, 12, 15, 18, 21, 24]                 # the hub: every row but its own self slots and row 3, ascending
    assert lists[1] == []                                         # heard by none
    assert lists[5] == [2 * Kn, 2 * Kn + 1]                       # the same index twice in one row: both slots, in slot order
    assert lists[3] == [] and 3 * Kn not in edge and 3 * Kn + 1 not in edge       # vehicle 3 is named by its own self slots alone
    assert lists[2] == [1, 22, 25] and 0 not in edge and 2 not in edge            # (the hub's own slots 0 and 2 name itself)
    flat = idx.reshape(-1)
    valid = [e for e in range(B * Kn) if 0 <= flat[e] < B and flat[e] != e // Kn]
    assert sorted(edge.tolist()) == valid
    for v, lst in enumerate(lists):
        assert lst == sorted(lst) and all(flat[e] == v for e in lst)
    one = np.array([[-1]], dtype=np.int32)
    assert C.reverse_lists(one)[0].tolist() == [0, 0] and C.reverse_lists(one)[1].size == 0


# ---------------------------------------------------------------- the interface and the code objects
def test_the_exports_are_declared_and_bound():
    """Header and binding agree on every new entry's argument count; the interface version is what it was (entries were added, none
    changed)."""
    import os
    import re
    from ndp_nmpc_qd_amd import _lib
    lib = _lib.load()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndp_nmpc.h")) as fh:
        hdr = fh.read()
    for name, count in (("ndp_closed_loop_formation_config", 3), ("ndp_plant_force_scatter_device", 4),
                        ("ndp_closed_loop_formation_device", 17), ("ndp_closed_loop_formation_vjp_device", 26)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m and name in _lib.EXPORTS
        assert m.group(1).count(",") + 1 == len(getattr(lib, name).argtypes) == count, name
    assert len(lib.ndp_closed_loop_device.argtypes) == 15 and len(lib.ndp_closed_loop_vjp_device.argtypes) == 23
    assert _lib.ABI_VERSION == 9 and lib.ndp_abi_version() == 9


def test_the_new_kernels_keep_their_state_in_registers():
    """closed_loop_formation_rev_link_kernel and closed_loop_scatter_kernel: one kernel each, no scratch, no spill, no LDS, at most 256
    registers, in the code object of closed_loop_rev_link_kernel -- which has the registers it had before they existed (190)."""
    from ndp_nmpc_qd_amd import build, isa_inspect as I
    co = I.CodeObject(build.build())
    k = co.kernels()
    old = [n for n in k if "closed_loop_rev_link_kernel" in n]
    assert len(old) == 1 and k[old[0]]["vgpr"] == 190 and k[old[0]]["spill"] == 0
    for part in ("closed_loop_formation_rev_link_kernel", "closed_loop_scatter_kernel"):
        found = [n for n in k if part in n]
        assert len(found) == 1, (part, found)
        v = k[found[0]]
        assert v["scratch"] == 0 and v["spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0, (part, v)
        assert v["vgpr"] + v["agpr"] <= 256, (part, v)
        assert co.code_object_of(found[0]) == co.code_object_of(old[0]), part
