"""The downwash network's blob (ndp_set_mlp_weights: W1[128][6] b1 W2[64][128] b2 W3[128][64] b3 W4[3][128] b4, float32) and the index
map of its transposed device image, restated in numpy for the tests (csrc/mlp_vjp.hip: fragt_source)."""
import numpy as np

SHAPES = (("W1", (128, 6)), ("b1", (128,)), ("W2", (64, 128)), ("b2", (64,)), ("W3", (128, 64)), ("b3", (128,)), ("W4", (3, 128)),
          ("b4", (3,)))
NPARAM = 17859
FR_TOTAL = 18432          # floats of the forward's fragment blob (csrc/mlp_tile.hpp: FR_TOTAL)
FRT_TOTAL = 2 * 128 * 64  # floats of the transposed image (csrc/host.hpp: FRT_TOTAL)


def offsets():
    """{name: (first index in the blob, shape)} of the eight parameter groups."""
    out, o = {}, 0
    for name, shp in SHAPES:
        out[name] = (o, shp)
        o += int(np.prod(shp))
    assert o == NPARAM
    return out


def split(blob):
    """{name: array view} of a blob (numpy array or torch tensor of 17859 values)."""
    return {name: blob[o:o + int(np.prod(shp))].reshape(shp) for name, (o, shp) in offsets().items()}


def f0(r):
    return (r & 3) + 8 * (r >> 2)


def fragt_source():
    """int array [FRT_TOTAL]: index into the blob of the weight each float of the transposed image holds.  One 64-lane record per
    v_mfma_f32_32x32x2_f32 of the backward data path: lane l of record (it, st, r) is W[st*32 + f0(r) + 4 (l>>5)][it*32 + (l&31)] --
    layer 3 (d2 tile it of 2 from d3 tile st of 4) first, layer 2 (d1 tile it of 4 from d2 tile st of 2) behind it."""
    off = offsets()
    i = np.arange(FRT_TOTAL)
    l3 = i < 128 * 64
    q = np.where(l3, i, i - 128 * 64)
    lane, r, t = q & 63, (q >> 6) & 15, q >> 10
    it = np.where(l3, t >> 2, t >> 1)
    st = np.where(l3, t & 3, t & 1)
    out = st * 32 + f0(r) + 4 * (lane >> 5)
    inn = it * 32 + (lane & 31)
    return np.where(l3, off["W3"][0] + out * 64 + inn, off["W2"][0] + out * 128 + inn)
