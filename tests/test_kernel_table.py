"""The control-step kernel table on the CPU: every row of enum RtiId (csrc/rti_table.hpp) / k_rti (csrc/rti_kernels.hip) has a device case in
tests/test_kernel_table_gpu.py, or is listed there as unreachable for a reason this file checks by arithmetic; and the launch geometry
that module expects per horizon follows from ndp_create's rules applied to the LDS image of the wave program's host build."""
import os
import re

import pytest

from ndp_nmpc_qd_amd import _lib
from tests import test_kernel_table_gpu as G

CSRC = os.path.join(os.path.dirname(_lib.__file__), "csrc")
SRC = os.path.join(CSRC, "rti_kernels.hip")          # the table k_rti
FRAG_SRC = os.path.join(CSRC, "mlp_tile.hpp")        # the fragment blob's layout
LDS_BYTES = 160 * 1024


def _source(path=SRC):
    with open(path) as fh:
        return re.sub(r"//[^\n]*", "", fh.read())


def _fr_total():
    """FR_TOTAL (floats of the downwash network's fragment blob): the enum that defines it, evaluated with C's integer division."""
    m = re.search(r"enum \{ (FR_L1 = .*?)\};", _source(FRAG_SRC), re.S)
    vals = {}
    for item in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        name, expr = (t.strip() for t in item.split("="))
        vals[name] = eval(expr.replace("/", "//"), {}, dict(vals))
    return vals["FR_TOTAL"]


@pytest.fixture(scope="module")
def emu():
    from tests.emu import emu
    return emu


def slots_for(N):
    return (7 * N - 3 + 63) // 64


def _per_wave_bytes(emu, N):
    """ndp_create: lds_per_wave = lds_doubles(N) rounded up to an even count (emu_lds_doubles adds the debug dump's DBG_EXTRA)."""
    dbl = emu.lib().emu_lds_doubles(N) - _dbg_extra()
    return ((dbl + 1) & ~1) * 8


def _dbg_extra():
    with open(os.path.join(CSRC, "rti_wave.hpp")) as fh:
        return int(re.search(r"enum \{ DBG_EXTRA = (\d+) \}", fh.read()).group(1))


def _waves(emu, N):
    w = 4
    while w > 1 and _per_wave_bytes(emu, N) * w > LDS_BYTES:
        w >>= 1
    return w


def _fusable(emu, N, w):
    return N + 1 <= 32 and slots_for(N) <= 3 and _per_wave_bytes(emu, N) * w >= _fr_total() * 4


def test_enum_and_initialiser_have_the_same_rows():
    src = _source()
    names = _lib.rti_kernel_names()
    body = re.search(r"static const RtiKern k_rti\[\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = re.findall(r"\{\(const void \*\)", body)
    assert len(names) == len(rows) == len(set(names)) == 48, (len(names), len(rows))
    assert len(names) <= 64                            # (one bit each in ndp_debug_rti_launched's mask)


def test_every_row_has_a_device_case_or_a_checked_reason():
    names = set(_lib.rti_kernel_names())
    assert not set(G.CASES) & set(G.UNREACHABLE)
    assert set(G.CASES) | set(G.UNREACHABLE) == names, (names - set(G.CASES) - set(G.UNREACHABLE), set(G.CASES) - names)
    tests = {n for n in dir(G) if n.startswith("test_")}
    assert set(G.CASES.values()) <= tests, set(G.CASES.values()) - tests


def test_fragment_blob_size():
    assert _fr_total() == 18432                        # 73.7 KB


def test_k3f_1_is_unreachable(emu):
    """One wave per workgroup never holds the network: for every N with at most 3 slots, one wave's slice is smaller than FR_TOTAL
    floats, so can_fuse is false wherever the one-wave three-slot kernels run."""
    assert "K3F_1" in G.UNREACHABLE
    for N in range(2, 47):
        if slots_for(N) <= 3:
            assert _per_wave_bytes(emu, N) < _fr_total() * 4, N


def test_k5_4_is_unreachable(emu):
    """The five-slot kernels at four waves: every N with more than 3 slots needs more than 160 KB for four instances, so ndp_create
    halves the waves (NDP_DEV_WAVES only lowers them)."""
    assert "K5_4" in G.UNREACHABLE
    for N in range(2, 47):
        if slots_for(N) > 3:
            assert 4 * _per_wave_bytes(emu, N) > LDS_BYTES, N


def test_geometry_table_follows_the_rules(emu):
    """The GPU module's expected (waves, fusable, row) per horizon = ndp_create's and rti_pick's rules on the emulator's LDS image."""
    for N in range(2, 47):
        w = _waves(emu, N)
        fu = _fusable(emu, N, w)
        wi = {4: "4", 2: "2", 1: "1"}[w]
        plain = "K20" if (N == 20 and w == 4) else f"K{3 if slots_for(N) <= 3 else 5}_{wi}"
        fused = ("K20F" if (N == 20 and w == 4) else f"K3F_{wi}") if fu else plain
        assert G.geometry(N) == (w, fu, plain, fused), (N, G.geometry(N), (w, fu, plain, fused))
    assert slots_for(46) == 5 and 7 * 46 - 3 == 5 * 64 - 1          # N = 46: all lanes of the five slots but one
