"""The downwash network at weights other than the shipped blob, CPU side (tests/mlp_families.py; device side:
tests/test_downwash_weights_gpu.py).  What is shown here, without a GPU: that the float64 reference and the bars the device tests use can
be met at every family (plain fp32 arithmetic meets them), that the device's fp16 pair split as designed meets them, that the same split
with fp16 subnormal operands flushed to zero misses them by more than 10x on the three rescaled families -- so the inputs can fail --, that
the rescaled families are the shipped function bit for bit, that the margin rule leaves enough rows at the device tests' cases, and that
mlp_frag.frag_words (the fragment image the device builders are compared with word for word) holds every weight to the pair's precision."""
import numpy as np
import pytest

from ndp_nmpc_qd_amd import mlp_frag
from tests import mlp_families as F
from tests import mlp_vjp_ref as R


@pytest.fixture(scope="module")
def rows():
    """5 376 rows as mlp_vjp_ref.draw_rows draws them, rounded to float32 (what the device sees)."""
    return R.draw_rows(np.random.default_rng(1), (5376,)).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def errors(rows):
    """{family: (plain fp32, pair split, pair split with fp16 subnormals flushed)} errors against float64, max |f - truth| / max(1, |truth|)."""
    out = {}
    for name in F.FORWARD:
        blob = F.family(name)
        truth = F.forward64(blob, rows)
        out[name] = tuple(F.rel_err(f, truth) for f in (F.forward32(blob, rows), F.forward_pair(blob, rows), F.forward_pair(blob, rows, flush=True)))
        print(f"{name:8s} fp32 {out[name][0]:.2e}  pair split {out[name][1]:.2e}  flushed {out[name][2]:.2e}  subnormal hi parts: "
              f"W2 {F.subnormal_share(blob, 2):.3f} W3 {F.subnormal_share(blob, 3):.3f}")
    return out


def test_families_are_blobs_of_the_stated_kind():
    shipped = F.family("shipped")
    for name in F.ALL:
        blob = F.family(name)
        assert blob.dtype == np.float32 and blob.shape == (mlp_frag.NPARAM,), name
        assert np.array_equal(blob, F.family(name)), name                       # seeded
        assert (name == "shipped") == np.array_equal(blob, shipped), name
        if name != "edges":
            assert np.isfinite(blob).all() and np.array_equal(blob, F.in_host_range(blob)), name
    assert F.subnormal_share(shipped, 2) < 0.03 and F.subnormal_share(shipped, 3) < 0.06
    assert F.subnormal_share(F.family("tiny2"), 2) > 0.4 and F.subnormal_share(F.family("tiny3"), 3) > 0.4
    assert F.subnormal_share(F.family("big2"), 3) > 0.1
    p = mlp_frag.split(F.family("sparse"))
    for k in ("W2", "W3"):
        zero = p[k] == 0
        assert 0.45 < zero.mean() < 0.55 and 0.4 < np.signbit(p[k][zero]).mean() < 0.6, k
    assert not np.array_equal(F.family("pert", 0), F.family("pert", 1))
    e = mlp_frag.split(F.family("edges"))
    t = F.edge_table(0)
    assert t.size % 2 == 1 and t.size > 300
    for k in ("W2", "W3"):                                                       # every table entry on every element of the 8-half records
        flat = e[k].reshape(-1).view(np.uint32)
        for j in range(8):
            assert set(flat[j::8].tolist()) == set(t.view(np.uint32).tolist()), (k, j)
    host = F.in_host_range(F.family("edges"))
    assert np.abs(mlp_frag.split(host)["W2"]).max() < mlp_frag.H16_MAX and np.abs(e["W2"]).max() >= mlp_frag.H16_MAX
    assert (host != F.family("edges")).sum() == (np.abs(F.family("edges")) >= mlp_frag.H16_MAX).sum()


@pytest.mark.parametrize("name", F.FORWARD)
def test_plain_fp32_meets_the_bar_against_the_float64_reference(errors, name):
    """The reference can be met: numpy fp32 against mlp_vjp_ref.forward64 on inputs rounded to float32 first."""
    assert errors[name][0] <= F.FORWARD_BAR


@pytest.mark.parametrize("name", F.FORWARD)
def test_the_pair_split_as_designed_meets_the_forward_bar(errors, name):
    assert errors[name][1] <= F.forward_bar(errors[name][0])


@pytest.mark.parametrize("name", F.RESCALED)
def test_flushed_fp16_subnormals_miss_the_forward_bar_tenfold(errors, name):
    """The inputs can fail: with every fp16 subnormal operand zero the same arithmetic is 2e-4 ... 6e-3 off."""
    assert errors[name][2] >= 10.0 * F.forward_bar(errors[name][0])


def test_flushing_changes_nothing_measurable_at_the_shipped_weights(errors):
    """... which is why the shipped blob alone cannot tell: there the flushed form passes the same bar."""
    assert errors["shipped"][2] <= F.forward_bar(errors["shipped"][0])


@pytest.mark.parametrize("name", F.RESCALED)
def test_rescaled_families_are_the_shipped_function_bit_for_bit_in_float64(rows, name):
    gf = np.random.default_rng(2).normal(size=(rows.shape[0], 3))
    gz0, _, _, f0 = R.vjp64(F.family("shipped"), rows, gf)
    gz, _, _, f = R.vjp64(F.family(name), rows, gf)
    assert np.array_equal(f, f0) and np.array_equal(gz, gz0)


def test_the_cap_case_is_one_and_fp32_and_the_pair_split_agree_with_the_capped_float64_network():
    """big2 at 1000x the envelope: layer-2 activations pass the cap of 65 000 (so the uncapped network is another function there), plain
    fp32 with the cap and the emulated pair split both sit at the capped float64 network."""
    blob = F.family("big2")
    _, _, z = F.forward_inputs(B=F.FORWARD_B, scale=F.CAP_SCALE)
    p = mlp_frag.split(blob.astype(np.float64))
    h1 = np.maximum(z @ p["W1"].T + p["b1"], 0.0)
    h2 = np.maximum(np.minimum(h1, F.CAP) @ p["W2"].T + p["b2"], 0.0)
    assert h1.max() < F.CAP < h2.max() and (h2 > F.CAP).any(axis=1).mean() > 0.5
    truth = F.forward64(blob, z, cap=True)
    assert F.rel_err(F.forward64(blob, z), truth) > 1e-2
    e32, ep = F.rel_err(F.forward32(blob, z, cap=True), truth), F.rel_err(F.forward_pair(blob, z), truth)
    print(f"cap: fp32 {e32:.2e}  pair split {ep:.2e}  max |force| {np.abs(truth).max():.3g}")
    assert ep <= F.forward_bar(e32)


@pytest.mark.parametrize("B", F.BACKWARD_B)
@pytest.mark.parametrize("form", F.BACKWARD_FORMS)
def test_the_margin_rule_leaves_enough_rows_at_the_device_tests_cases(form, B):
    """At the batch sizes and seeds of the device tests: at most MAX_DROPPED of the rows are within the margin of a ReLU kink, for every
    backward family (the rescaled ones under the shipped blob's margin: F.drop_rows), and some instance is live."""
    from tests.test_downwash_vjp_gpu import _case
    c = _case(form, F.backward_seed(form, B), B=B)
    assert c["live"].any()
    for name in F.BACKWARD:
        share = float(F.drop_rows(name, F.family(name), c["z"]).mean())
        print(f"{form} B = {B} {name}: {share:.4f} of the rows below the margin")
        assert share <= R.MAX_DROPPED, name
    own = R.vjp64(F.family("tiny2"), c["z"].reshape(-1, 6), np.zeros((c["z"].size // 6, 3)))[2]
    assert (own < R.MARGIN).mean() > 0.99                                        # (why tiny2 cannot use its own absolute margin)


def test_init_is_not_a_backward_family_for_a_reason(rows):
    assert float(F.drop_rows("init", F.family("init"), rows).mean()) > R.MAX_DROPPED


@pytest.mark.parametrize("name", F.ALL)
def test_frag_words_holds_every_weight_to_the_pairs_precision(name):
    """mlp_frag.frag_words against a second formulation: hi + lo / 2^11 read back out of the image per weight (F.recovered walks the layout
    from the weight's indices, frag_words from the record's) is within 2^-22 |w| + 2^-35 of every finite |w| < 65504; the fp32 words are
    the blob's own bits; the padding is zero."""
    blob = F.family(name)
    words = mlp_frag.frag_words(blob)
    assert words.dtype == np.uint32 and words.shape == (mlp_frag.FR_TOTAL,)
    p = mlp_frag.split(blob)
    for w, got in zip((p["W2"], p["W3"]), F.recovered(words)):
        w = w.astype(np.float64)
        ok = np.isfinite(w) & (np.abs(w) < mlp_frag.H16_MAX)
        assert ok.mean() > 0.9
        assert (np.abs(w - got)[ok] <= 2.0 ** -22 * np.abs(w)[ok] + 2.0 ** -35).all()
        assert np.array_equal(np.signbit(got[ok & (w != 0)]), np.signbit(w[ok & (w != 0)]))
    f = words.view(np.float32)
    assert np.array_equal(f[mlp_frag.FR_B1:mlp_frag.FR_B2], p["b1"]) and np.array_equal(f[mlp_frag.FR_B2:mlp_frag.FR_B3], p["b2"])
    assert np.array_equal(f[mlp_frag.FR_B3:mlp_frag.FR_W4], p["b3"]) and np.array_equal(f[mlp_frag.FR_B4:mlp_frag.FR_B4 + 3], p["b4"])
    assert np.array_equal(f[mlp_frag.FR_W4:mlp_frag.FR_B4].reshape(128, 4)[:, :3], p["W4"].T)
    assert np.array_equal(np.sort(f[mlp_frag.FR_L1:mlp_frag.FR_B1]), np.sort(p["W1"].reshape(-1)))
    assert not words[mlp_frag.FR_HF + 32 * 512:].any() and not words[mlp_frag.FR_B4 + 3]
    assert not f[mlp_frag.FR_W4:mlp_frag.FR_B4].reshape(128, 4)[:, 3].any()


def test_host_form_refuses_what_it_documents_before_touching_the_device():
    """ndp_set_mlp_weights' argument checks need no handle state beyond the error string -- but they do need a handle, so the refusals
    themselves are tested on the device (tests/test_downwash_weights_gpu.py); here: the limit is declared where the header states it."""
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndp_nmpc.h")).read()
    assert "#define NDP_MLP_W23_LIMIT 65504.0f" in hdr and mlp_frag.H16_MAX == 65504.0
