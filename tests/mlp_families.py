"""Weight blobs other than the shipped one for the downwash network's tests (CPU only), and numpy restatements of its arithmetic.

family(name, seed) returns a float32 [17859] blob in mlp_frag.SHAPES order:
  shipped  weights/downwash_sn4.bin (spectrally normalised: 2 % of W2 and 5 % of W3 below 2^-14, the smallest normal fp16)
  tiny2    W2, b2 x 2^-10, W3 x 2^10          ReLU is positively homogeneous: the same function; 52 % of W2's fp16 hi parts subnormal
  tiny3    W3, b3 x 2^-10, W4 x 2^10          the same function; 42 % of W3 subnormal
  big2     W2, b2 x 2^8,   W3 x 2^-8          the same function; 11 % of W3 subnormal, layer-2 activations x 256
  sparse   half of W2 and W3 exactly 0, half of those -0.0 (a pruned network: zero and signed-zero operands)
  pert     every parameter x (1 + 0.3 N(0, 1))
  init     torch's default Linear initialisation, U(+-1/sqrt(fan_in)); forward tests only (its share of rows within 1e-4 of a ReLU kink
           reaches 0.091, above mlp_vjp_ref.MAX_DROPPED)
  edges    W2 and W3 filled cyclically from EDGE_TABLE (fp32 -> fp16 conversion edge cases), the other groups shipped; the fragment
           builders' test only (values of 65504 and above: the device form of ndp_set_mlp_weights only, the host form refuses them)
The power-of-two rescalings are exact in fp32 (no shipped weight leaves the normal fp32 range), so in float64 the three rescaled families
give the shipped network's force and g_z bit for bit (tests/test_downwash_weights.py checks it) while half of a layer's weights sit in the
fp16-subnormal range -- where a matrix instruction, a packed conversion or a host routine that flushes fp16 subnormals is 1e-3 off.

forward32 / forward_pair / forward64_capped: the network in plain numpy fp32, in the device's fp16 pair split (flush=True: every fp16
subnormal operand replaced by zero -- the fault the families are there to find), and in float64 with the device's activation cap."""
import numpy as np
import torch

from ndp_nmpc_qd_amd import _lib, mlp_frag
from tests import mlp_vjp_ref as R

RESCALED = ("tiny2", "tiny3", "big2")
BACKWARD = ("shipped",) + RESCALED + ("sparse", "pert")
FORWARD = BACKWARD + ("init",)
ALL = FORWARD + ("edges",)
CAP = 65000.0             # csrc/mlp_common.hpp: NDP_H16_CAP, on the two hidden layers that feed an fp16 split
FORWARD_BAR = 1e-5        # the project's bar for this network
FLOOR_FACTOR = 2.5        # ... or this many times the plain-fp32 evaluation's own error (test_downwash_mlp_error_against_the_fp32_noise_floor)


def _blob(p):
    return np.concatenate([np.asarray(p[n], dtype=np.float32).reshape(-1) for n, _ in mlp_frag.SHAPES])


def edge_table(seed=0):
    """float32 values at which an fp32 -> fp16 conversion (round to nearest even, subnormal results) can go wrong, both signs; odd length so
    that a cyclic fill puts every value on every element of the 8-half operand records."""
    f = np.float32
    mags = [0.0, 2.0 ** -25, np.nextafter(f(2.0 ** -25), f(1.0)), 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
            1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.996,
            2.0 ** -149, 2.0 ** -127, np.nextafter(f(2.0 ** -126), f(0.0)), 3 * 2.0 ** -140]      # (the last four: fp32 subnormals)
    fixed = np.array([s * m for m in mags for s in (1.0, -1.0)], dtype=np.float32)
    rng = np.random.default_rng(1000 + seed)
    n = 300
    bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | ((rng.integers(-30, 16, n) + 127).astype(np.uint32) << 23) \
        | rng.integers(0, 1 << 23, n).astype(np.uint32)
    t = np.concatenate([fixed, bits.view(np.float32)])
    return t if t.size % 2 else np.concatenate([t, t[-1:]])


def family(name, seed=0):
    p = {k: np.array(v, dtype=np.float64) for k, v in mlp_frag.split(_lib.load_weights()).items()}
    rng = np.random.default_rng(7000 + seed)
    if name == "shipped":
        pass
    elif name in RESCALED:
        l, s = {"tiny2": (2, 2.0 ** -10), "tiny3": (3, 2.0 ** -10), "big2": (2, 2.0 ** 8)}[name]
        p[f"W{l}"] *= s
        p[f"b{l}"] *= s
        p[f"W{l + 1}"] /= s
    elif name == "sparse":
        for l in (2, 3):
            u = rng.random(p[f"W{l}"].shape)
            p[f"W{l}"][u < 0.5] = 0.0
            p[f"W{l}"][u < 0.25] = -0.0
    elif name == "pert":
        for k in p:
            p[k] = p[k] * (1.0 + 0.3 * rng.standard_normal(p[k].shape))
    elif name == "init":
        for l, fan_in in ((1, 6), (2, 128), (3, 64), (4, 128)):
            b = 1.0 / np.sqrt(fan_in)
            p[f"W{l}"] = rng.uniform(-b, b, p[f"W{l}"].shape)
            p[f"b{l}"] = rng.uniform(-b, b, p[f"b{l}"].shape)
    elif name == "edges":
        t = edge_table(seed)
        n2 = p["W2"].size
        p["W2"] = np.resize(t, n2).reshape(p["W2"].shape)
        p["W3"] = np.resize(np.roll(t, -(n2 % t.size)), p["W3"].size).reshape(p["W3"].shape)
    else:
        raise KeyError(name)
    return _blob(p)


def in_host_range(blob):
    """`blob` with the W2 / W3 entries the host form of ndp_set_mlp_weights refuses (|w| >= 65504) pulled to the largest fp32 below."""
    out = np.array(blob, dtype=np.float32)
    top = np.nextafter(np.float32(mlp_frag.H16_MAX), np.float32(0.0))
    for k in ("W2", "W3"):
        o, shp = mlp_frag.offsets()[k]
        v = out[o:o + int(np.prod(shp))]
        big = np.abs(v) >= mlp_frag.H16_MAX
        v[big] = np.copysign(top, v[big])
    return out


def subnormal_share(blob, layer):
    """Share of the layer's nonzero weights whose fp16 hi part is subnormal (or zero)."""
    w = mlp_frag.split(np.asarray(blob))[f"W{layer}"]
    w = w[w != 0]
    return float((np.abs(w.astype(np.float16).astype(np.float64)) < 2.0 ** -14).mean())


def rel_err(f, truth):
    """max |f - truth| / max(1, |truth|)."""
    return float((np.abs(f - truth) / np.maximum(1.0, np.abs(truth))).max())


def forward64(blob, z, cap=False):
    """The float64 network on rows z [R,6]; cap=True: the hidden layers that feed an fp16 split (1 and 2) capped at CAP as relu_cap does."""
    if not cap:
        return R.forward64(R.params64(blob), torch.tensor(np.asarray(z, dtype=np.float64)))[0].numpy()
    p = {k: np.asarray(v, dtype=np.float64) for k, v in mlp_frag.split(np.asarray(blob)).items()}
    h = np.asarray(z, dtype=np.float64)
    for l in (1, 2, 3):
        h = np.maximum(h @ p[f"W{l}"].T + p[f"b{l}"], 0.0)
        if l < 3:
            h = np.minimum(h, CAP)
    return h @ p["W4"].T + p["b4"]


def forward32(blob, z, cap=False):
    """Plain numpy float32 evaluation (what fp32 arithmetic itself delivers: the floor the device is held against)."""
    p = mlp_frag.split(np.asarray(blob, dtype=np.float32))
    h = np.asarray(z, dtype=np.float32)
    for l in (1, 2, 3):
        h = np.maximum(h @ p[f"W{l}"].T + p[f"b{l}"], np.float32(0.0))
        if cap and l < 3:
            h = np.minimum(h, np.float32(CAP))
    return (h @ p["W4"].T + p["b4"]).astype(np.float64)


def _f16(x, flush):
    y = np.asarray(x, dtype=np.float32).astype(np.float16)
    if flush:
        y = np.where(np.abs(y) < np.float16(2.0 ** -14), np.float16(0.0), y)
    return y.astype(np.float64)


def _split(x, flush):
    x = np.asarray(x, dtype=np.float32)
    hi = _f16(x, flush)
    return hi, _f16((x - hi.astype(np.float32)) * np.float32(mlp_frag.LO_SCALE), flush)


def forward_pair(blob, z, flush=False):
    """mlp_tile's arithmetic restated: layer 1 fp32; layers 2 and 3 W x = W_hi x_hi + (W_hi x_lo + W_lo x_hi) / 2^11 on fp16 pairs of the
    weights and of the capped activations (products and sums exact here, rounded to fp32 per layer); layer 4 fp32 weights on fp32
    activations.  flush: every fp16 operand below 2^-14 in magnitude is zero."""
    p = mlp_frag.split(np.asarray(blob, dtype=np.float32))
    h = np.minimum(np.maximum(np.asarray(z, dtype=np.float32) @ p["W1"].T + p["b1"], np.float32(0.0)), np.float32(CAP))
    for l in (2, 3):
        wh, wl = _split(p[f"W{l}"], flush)
        xh, xl = _split(h, flush)
        v = xh @ wh.T + (xl @ wh.T + xh @ wl.T) / mlp_frag.LO_SCALE + p[f"b{l}"].astype(np.float64)
        h = np.maximum(v, 0.0).astype(np.float32)
        if l == 2:
            h = np.minimum(h, np.float32(CAP))
    return h.astype(np.float64) @ p["W4"].astype(np.float64).T + p["b4"].astype(np.float64)


def forward_bar(e_f32):
    return max(FORWARD_BAR, FLOOR_FACTOR * e_f32)


def drop_rows(name, blob, z):
    """bool [R]: rows of z [R,6] the margin rule gives a zero upstream (a hidden pre-activation within mlp_vjp_ref.MARGIN of its ReLU's
    kink in float64).  The absolute margin does not transfer to a rescaled layer (on tiny2 it would drop every row): for the three
    rescaled families the rule is taken on the shipped blob, whose pre-activations differ by the power of two alone -- the same ReLU
    pattern, the same rows."""
    ref = family("shipped") if name in RESCALED else blob
    margin = R.forward64(R.params64(ref), torch.tensor(np.asarray(z, dtype=np.float64).reshape(-1, 6)))[1].numpy()
    return (margin < R.MARGIN).reshape(np.shape(z)[:-1])


def recovered(words):
    """(W2, W3) float64 as hi + lo / 2^11 read back out of a fragment image (mlp_frag.frag_words' layout, walked the other way: by weight,
    not by record)."""
    hf = np.ascontiguousarray(words[mlp_frag.FR_HF:mlp_frag.FR_HF + 32 * 512]).view(np.float16).astype(np.float64)
    out = []
    for base, n_out, n_in in ((0, 64, 128), (16, 128, 64)):
        o, i = np.meshgrid(np.arange(n_out), np.arange(n_in), indexing="ij")
        ot, it, k = o // 32, i // 32, i % 32
        s, k = k // 16, k % 16
        j, h = 4 * (k // 8) + (k & 3), (k >> 2) & 1
        rec = base + (ot * (n_in // 32) + it) * 2 + s
        e = rec * 1024 + (32 * h + (o & 31)) * 8 + j
        out.append(hf[e] + hf[e + 512] / mlp_frag.LO_SCALE)
    return out


# ---- the cases the device tests run (tests/test_downwash_weights_gpu.py), stated here so that the CPU tests can check them
N = 20
FORWARD_B = 49            # 1 029 rows: 32 full 32-row tiles and a last one of 5 rows
BACKWARD_B = (256, 5)     # 5 376 rows; 105 rows (a partial tile, padding rows)
BACKWARD_FORMS = ("part", "index")
CAP_SCALE = 1000.0        # the cap test's inputs: this many times the envelope draw_rows draws


def backward_seed(form, B):
    """Seed of test_downwash_vjp_gpu._case for one backward case.  At B = 5 the `index` form has 21 distinct rows (all five instances read
    one neighbour row), so the share of rows under the margin moves in steps of 1/21 = 0.048: the base is one at which every backward
    family stays within MAX_DROPPED at all four cases, which tests/test_downwash_weights.py checks (a property of the inputs alone)."""
    return 800 + B + len(form)


def forward_inputs(seed=11, B=FORWARD_B, scale=1.0):
    """(other, xr [B,N+1,10] float64, z [B*(N+1),6] float64): z as the device sees it, (other - xr)[..., :6] rounded to float32."""
    rng = np.random.default_rng(seed)
    xr = rng.normal(0.0, 1.0, (B, N + 1, 10))
    other = rng.normal(0.0, 1.0, (B, N + 1, 10))
    other[:, :, :6] = xr[:, :, :6] + scale * R.draw_rows(rng, (B, N + 1))
    z = (other[:, :, :6] - xr[:, :, :6]).astype(np.float32).astype(np.float64)
    return other, xr, z.reshape(-1, 6)
