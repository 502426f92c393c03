"""The T axis of the forward-mode entry points, from shapes alone (batched._t_axis_shapes): no device, no library.

Every forward-mode method of BatchedNMPC takes tangents and outputs that carry a T axis -- behind the batch axis, or in front for the
weights' direction -- and accepts each of them without it (T = 1 as the tensor lies).  One pure function resolves T and the shape
demanded of every tensor for all five callers.  The expected shapes below are written out by hand from those methods' docstrings:
  step_jvp_device            tx0 [B,T,10], txr [B,T,N+1,10], tur [B,T,N,4], tf [B,T,N+1,3], du0 [B,T,4], dX [B,T,N+1,10], dU [B,T,N,4]
  downwash_jvp_device        tz [B,T,N+1,6], tw [T,17859], df [B,T,N+1,3]
  downwash_multi_jvp_device  tz [B,T,K,N+1,6], tw [T,17859], df [B,T,N+1,3]
  plant_force_jvp_device and plant_force_multi_jvp_device   tx [B,T,10], tw [T,17859], df [B,T,3]
at B = 3, N = 2.  The second half calls the five methods themselves on an engine without a handle, with CPU tensors and a recording
_dptr, so that each caller's own table is held to the same shapes.
"""
import pytest
import torch

from ndp_nmpc_qd_amd.batched import BatchedNMPC, _t_axis_shapes

B, N = 3, 2
F64, F32 = torch.float64, torch.float32


def _full(T, table):
    """The hand-written shapes of a table at T directions: T is None for the shapes without the axis."""
    t = () if T is None else (T,)
    return {
        "step": [(3, *t, 10), (3, *t, 3, 10), (3, *t, 2, 4), (3, *t, 3, 3), (3, *t, 4), (3, *t, 3, 10), (3, *t, 2, 4)],
        "downwash": [(3, *t, 3, 6), (*t, 17859), (3, *t, 3, 3)],
        "multi1": [(3, *t, 1, 3, 6), (*t, 17859), (3, *t, 3, 3)],
        "multi3": [(3, *t, 3, 3, 6), (*t, 17859), (3, *t, 3, 3)],
        "plant": [(3, *t, 10), (*t, 17859), (3, *t, 3)],
        "plant_multi": [(3, *t, 10), (*t, 17859), (3, *t, 3)],
    }[table]


# (tail behind the T axis, batch dimensions in front of it) per tensor, in the callers' argument order; which one is the weights' direction
TABLES = {
    "step": ([((10,), 1), ((3, 10), 1), ((2, 4), 1), ((3, 3), 1), ((4,), 1), ((3, 10), 1), ((2, 4), 1)], None),
    "downwash": ([((3, 6), 1), ((17859,), 0), ((3, 3), 1)], 1),
    "multi1": ([((1, 3, 6), 1), ((17859,), 0), ((3, 3), 1)], 1),
    "multi3": ([((3, 3, 6), 1), ((17859,), 0), ((3, 3), 1)], 1),
    "plant": ([((10,), 1), ((17859,), 0), ((3,), 1)], 1),
    "plant_multi": ([((10,), 1), ((17859,), 0), ((3,), 1)], 1),
}
HAS_N_TAN = {"step": False, "downwash": True, "multi1": True, "multi3": True, "plant": True, "plant_multi": True}


def _rows(name, shapes):
    return [(s, tail, lead) for s, (tail, lead) in zip(shapes, TABLES[name][0])]


@pytest.mark.parametrize("name", list(TABLES))
def test_every_tensor_with_the_t_axis(name):
    for T in (1, 2, 8):
        want = _full(T, name)
        assert _t_axis_shapes(name, B, _rows(name, want)) == (T, want)
        if HAS_N_TAN[name]:
            assert _t_axis_shapes(name, B, _rows(name, want), n_tan=T) == (T, want)


@pytest.mark.parametrize("name", list(TABLES))
def test_no_tensor_with_the_t_axis(name):
    want = _full(None, name)
    assert _t_axis_shapes(name, B, _rows(name, want)) == (1, want)
    assert _t_axis_shapes(name, B, _rows(name, want), n_tan=1) == (1, want)       # n_tan = 1 with tensors lacking the axis: accepted
    # mixed at T = 1: each tensor is demanded as it came
    mixed = [a if i % 2 else b for i, (a, b) in enumerate(zip(_full(1, name), want))]
    assert _t_axis_shapes(name, B, _rows(name, mixed)) == (1, mixed)
    assert _t_axis_shapes(name, B, _rows(name, mixed), n_tan=1) == (1, mixed)


@pytest.mark.parametrize("name", list(TABLES))
def test_n_tan_2_with_a_tensor_lacking_the_axis(name):
    for k in range(len(TABLES[name][0])):
        shapes = _full(2, name)
        shapes[k] = _full(None, name)[k]
        with pytest.raises(ValueError, match=name + ": .*without the T axis"):
            _t_axis_shapes(name, B, _rows(name, shapes), n_tan=2)
        only = [s if i == k else None for i, s in enumerate(shapes)]
        with pytest.raises(ValueError, match="without the T axis"):
            _t_axis_shapes(name, B, _rows(name, only), n_tan=2)


@pytest.mark.parametrize("name", list(TABLES))
def test_two_tensors_that_disagree(name):
    n = len(TABLES[name][0])
    for i in range(n):
        for j in range(n):
            if i != j:
                shapes = [None] * n
                shapes[i], shapes[j] = _full(2, name)[i], _full(3, name)[j]
                with pytest.raises(ValueError, match=name + ": .*disagree on the number of directions"):
                    _t_axis_shapes(name, B, _rows(name, shapes))
    # one with T = 2, one without the axis (T = 1 as it lies): they disagree as well
    shapes = [None] * n
    shapes[0], shapes[-1] = _full(2, name)[0], _full(None, name)[-1]
    with pytest.raises(ValueError, match="disagree"):
        _t_axis_shapes(name, B, _rows(name, shapes))


@pytest.mark.parametrize("name", list(TABLES))
def test_all_tensors_none(name):
    n = len(TABLES[name][0])
    assert _t_axis_shapes(name, B, _rows(name, [None] * n)) == (1, [None] * n)
    for T in (1, 2, 8):
        assert _t_axis_shapes(name, B, _rows(name, [None] * n), n_tan=T) == (T, [None] * n)
    # a tensor that is not given demands nothing and says nothing about T
    for T in (2, 8):
        shapes = [s if i == 0 else None for i, s in enumerate(_full(T, name))]
        assert _t_axis_shapes(name, B, _rows(name, shapes)) == (T, shapes)


@pytest.mark.parametrize("name", list(TABLES))
def test_where_the_t_axis_sits(name):
    """Position 0 for the weights' direction, 1 for every other tensor: T is read there, and a 5 anywhere else is not taken for it."""
    table, w = TABLES[name]
    for k in range(len(table)):
        shapes = [None] * len(table)
        shapes[k] = _full(5, name)[k]
        T, want = _t_axis_shapes(name, B, _rows(name, shapes))
        assert T == 5 and want == shapes
        assert shapes[k][0 if k == w else 1] == 5 and (k == w or shapes[k][0] == B)
        assert want[k].index(5) == (0 if k == w else 1)


# ------------------------------------------------------------------ the callers' own tables
class _Lib:
    def __getattr__(self, name):
        return lambda *a: 0


def _engine(seen):
    e = object.__new__(BatchedNMPC)
    e.B, e.N, e._h, e._lib = B, N, None, _Lib()
    e._torch_default_wait = lambda stream: None

    def dptr(t, dtype, shape):
        if t is not None:
            assert t.dtype == dtype and tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape), dtype)
            seen[id(t)] = (dtype, tuple(shape))
        return None
    e._dptr = dptr
    e._other_ptr = lambda other, other_index: (None, 10)
    return e


def _call(name, e, ts, n_tan):
    z = lambda *s, dt=F64: torch.zeros(s, dtype=dt)  # noqa: E731
    if name == "step":
        assert n_tan is None
        tape = (z(B, N + 1, 10), z(B, N, 4), z(B, N, 4, dt=torch.int8))
        return e.step_jvp_device(z(B, 10), z(B, N + 1, 10), z(B, N, 4), tape, *ts[:4], du0=ts[4], dX=ts[5], dU=ts[6])
    if name == "downwash":
        return e.downwash_jvp_device(z(B, N + 1, 10), z(B, N + 1, 10), tz=ts[0], tw=ts[1], n_tan=n_tan, df=ts[2])
    if name in ("multi1", "multi3"):
        idx = torch.zeros((B, int(name[-1])), dtype=torch.int32)
        return e.downwash_multi_jvp_device(z(B, N + 1, 10), idx, z(B, N + 1, 10), tz=ts[0], tw=ts[1], n_tan=n_tan, df=ts[2])
    if name == "plant":
        return e.plant_force_jvp_device(z(B, 10), torch.zeros(B, dtype=torch.int32), tx=ts[0], tw=ts[1], n_tan=n_tan, df=ts[2])
    return e.plant_force_multi_jvp_device(z(B, 10), torch.zeros((B, 2), dtype=torch.int32), tx=ts[0], tw=ts[1], n_tan=n_tan, df=ts[2])


@pytest.mark.parametrize("name", list(TABLES))
def test_the_callers_demand_these_shapes(name):
    w = TABLES[name][1]
    for T in (None, 1, 2, 8):
        shapes = _full(T, name)
        dts = [F32 if k == w else F64 for k in range(len(shapes))]
        ts = [torch.zeros(s, dtype=dt) for s, dt in zip(shapes, dts)]
        for n_tan in {None, T or 1} if HAS_N_TAN[name] else {None}:
            seen = {}
            _call(name, _engine(seen), ts, n_tan)
            assert [seen.get(id(t)) for t in ts] == list(zip(dts, shapes))
    ts = [torch.zeros(s, dtype=F32 if k == w else F64) for k, s in enumerate(_full(2, name))]
    ts[0] = ts[0][:, 0].contiguous()
    if HAS_N_TAN[name]:
        with pytest.raises(ValueError, match=r"_jvp_device: .*without the T axis"):
            _call(name, _engine({}), ts, 2)
    with pytest.raises(ValueError, match=r"_jvp_device: .*disagree on the number of directions"):
        _call(name, _engine({}), ts, None)
