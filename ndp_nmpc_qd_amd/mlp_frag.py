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


FR_L1, FR_B1, FR_B2, FR_B3, FR_W4, FR_B4, FR_HF = 0, 768, 896, 960, 1088, 1600, 1604   # csrc/mlp_tile.hpp: enum FR_*, 32-bit words
LO_SCALE = 2048.0         # csrc/mlp_common.hpp: NDP_LO_SCALE
H16_MAX = 65504.0         # largest finite fp16: ndp_set_mlp_weights refuses |W2|, |W3| at or above it


def pair_split(w):
    """(hi, lo) float16 arrays of a float32 array: hi = fp16(w), lo = fp16((w - hi) * 2^11), the residual taken in float32 (where it is
    exact) -- the split make_fragments applies to layers 2 and 3.  Round to nearest even, subnormal results kept."""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = w.astype(np.float16)
        lo = ((w - hi.astype(np.float32)) * np.float32(LO_SCALE)).astype(np.float16)
    return hi, lo


def frag_words(blob):
    """uint32 [FR_TOTAL]: the forward's fragment image of a blob as make_fragments (csrc/downwash.hip) defines it -- fp32 words for layer 1,
    the biases and layer 4, then 32 records of fp16 pairs for layers 2 and 3 (record = (out tile, in tile, k-step); lane l element j holds
    W[ot*32 + (l&31)][it*32 + 16 s + 8 (j>>2) + 4 (l>>5) + (j&3)]; per record 512 hi halves, then 512 lo halves)."""
    p = split(np.ascontiguousarray(blob, dtype=np.float32))
    fr = np.zeros(FR_TOTAL, dtype=np.float32)
    rec, l = np.meshgrid(np.arange(12), np.arange(64), indexing="ij")
    fr[FR_L1:FR_B1] = p["W1"][(rec // 3) * 32 + (l & 31), 2 * (rec % 3) + (l >> 5)].reshape(-1)
    fr[FR_B1:FR_B2], fr[FR_B2:FR_B3], fr[FR_B3:FR_W4] = p["b1"], p["b2"], p["b3"]
    fr[FR_W4:FR_B4].reshape(128, 4)[:, :3] = p["W4"].T
    fr[FR_B4:FR_B4 + 3] = p["b4"]
    out = fr.view(np.uint32)
    hf = out[FR_HF:FR_HF + 32 * 512].view(np.uint16).reshape(32, 2, 64, 8)
    q, l, j = np.meshgrid(np.arange(16), np.arange(64), np.arange(8), indexing="ij")
    for layer, W in ((0, p["W2"]), (1, p["W3"])):
        ot, it = (q // 8, (q // 2) % 4) if layer == 0 else (q // 4, (q // 2) % 2)
        kin = it * 32 + 16 * (q % 2) + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)
        hi, lo = pair_split(W[ot * 32 + (l & 31), kin])
        hf[16 * layer:16 * layer + 16, 0], hf[16 * layer:16 * layer + 16, 1] = hi.view(np.uint16), lo.view(np.uint16)
    return out
