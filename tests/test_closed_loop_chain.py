"""The composed float64 reference of the chained closed loop (tests/closed_loop_chain_ref.py) without a GPU: its reverse sweep against
central finite differences of the oracle's closed loop, its forward sweep against its reverse sweep (duality), and the shape of the graph
the torch layer builds over three ticks, on a stub engine.  The device side: tests/test_closed_loop_chain_gpu.py.

What is differentiated is a PARTIAL derivative, the one the layer promises: every tick's linearisation point (the pre-step iterate), final
active set and gate are held fixed.  The finite differences therefore restart every tick of every perturbed run from the nominal run's
recorded iterate and kept set, and count only the vehicles whose sets and iteration words stay put at every tick."""
import numpy as np
import pytest

from tests import closed_loop_chain_ref as R

K, N = 3, 20
FD_BAR = 1e-6            # test_device_finite_differences_of_a_trajectory_loss's
H64, H32 = 1e-6, 2.0 ** -14


def _case(oracle, form):
    """Inputs, the nominal record (ndp form: with the float64 network, see closed_loop_chain_ref._force), upstreams and the systems."""
    if form == "ext":
        a = R.ext_inputs(8, K, N, seed=20231516)
        kw = dict(f=a["f"])
    else:
        a = R.ndp_inputs(K, seed=1)
        kw = dict(other=a["other"], idx=a["idx"], blob=np.asarray(a["blob"], dtype=np.float64), net64=True)
    rec = R.nominal_cpu(oracle, a["x0"], a["xr"], a["ur"], a["fp"], **kw)
    B = a["x0"].shape[0]
    ok = R.set_finish(rec)
    which = list(range(B)) if form == "ndp" else [int(v) for v in np.flatnonzero(ok)[:4]]
    return a, kw, rec, ok, which, R.upstreams(K, B, N, seed=5), R.systems(oracle, rec, which)


@pytest.fixture(scope="module")
def cases(oracle):
    return {form: _case(oracle, form) for form in ("ext", "ndp")}


@pytest.mark.parametrize("form", ["ext", "ndp"])
def test_reverse_sweep_matches_central_differences_of_the_oracle_loop(oracle, cases, form):
    """Two entries of every leaf at every tick (x_0; xr_k, ur_k, fp_k; ext: f_k; ndp: other_k and eight weights, one per parameter group):
    central differences of L over the oracle's closed loop, steps 1e-6 (2^-14 on the float32 leaves f and w), every tick of every
    perturbed run restarted from the nominal iterate and kept set, within 1e-6 of max(1, |g|) on the vehicles whose set and iteration
    word stay put at every tick.  ext: per vehicle; ndp: L summed over the four vehicles (other_k and w couple them), all four must stay."""
    a, kw, rec, ok, which, (G, H, A), sys_ = cases[form]
    B = a["x0"].shape[0]
    assert ok[which].all() and len(which) >= 4
    if form == "ext":
        assert rec["act"][:, which].any()                                      # an input on a bound among them
    else:
        assert rec["open"].all() and R.margins(a["blob"], a["other"], a["xr"], a["idx"]).min() >= 1e-3       # no ReLU near its kink
    g = R.reverse(sys_, rec, G, H, A)
    row = {v: j for j, v in enumerate(which)}
    rng = np.random.default_rng(9)
    leaves = [("x0", None)] + [(n, k) for k in range(K) for n in (("xr", "ur", "fp") + (("f",) if form == "ext" else ("other",)))]
    cases_ = []
    for name, k in leaves:
        base = a[name] if k is None else a[name][k]
        for _ in range(2):
            at = tuple(int(rng.integers(0, s)) for s in base.shape[1:])
            if name == "xr" and at[0] == 0:
                at = (1,) + at[1:]                                              # (stage 0's reference row has no weight: gradient exactly 0)
            if name == "other":
                at = (at[0] % N, at[1] % 6)                                     # (the network reads columns 0..5; f_N moves nothing)
            cases_.append((name, k, at))
    if form == "ndp":
        from ndp_nmpc_qd_amd import mlp_frag
        cases_ += [("w", None, (o + int(rng.integers(0, int(np.prod(s)))),)) for o, s in mlp_frag.offsets().values()]
    stable = ok.copy()
    fds = []
    for name, k, at in cases_:
        h = H32 if name in ("f", "w") else H64
        L = []
        for sgn in (1.0, -1.0):
            p = {n: np.array(v, dtype=np.float64) for n, v in a.items() if n in ("x0", "xr", "ur", "fp", "f", "other")}
            blob = None if form == "ext" else np.asarray(a["blob"], dtype=np.float64).copy()
            if name == "w":
                blob[at] += sgn * h
            else:
                (p[name] if k is None else p[name][k])[(slice(None),) + at] += sgn * h
            kw2 = dict(f=p["f"]) if form == "ext" else dict(other=p["other"], idx=a["idx"], blob=blob, net64=True)
            r = R.nominal_cpu(oracle, p["x0"], p["xr"], p["ur"], p["fp"], restart=rec, **kw2)
            stable &= R.set_finish(r) & (r["act"] == rec["act"]).all(axis=(0, 2, 3))
            L.append(R.loss(r, G, H, A))
        fds.append((L[0] - L[1]) / (2 * h))
    assert stable[which].all() if form == "ndp" else stable[which].sum() >= 3
    worst = 0.0
    for (name, k, at), fd in zip(cases_, fds):
        got = g[name] if k is None else g[name][k]
        if form == "ndp":       # L summed over the vehicles: the perturbation moved that entry of every row of the leaf at once
            ref = got[at] if name == "w" else got[(slice(None),) + at].sum()
            err = abs(fd.sum() - ref) / max(1.0, abs(ref))
            if name == "other":
                assert abs(ref) > 1e-6                                          # (the neighbour's window does reach the loss)
        else:
            vs = [v for v in which if stable[v]]
            ref = np.array([got[(row[v],) + at] for v in vs])
            err = float((np.abs(fd[vs] - ref) / np.maximum(1.0, np.abs(ref))).max())
        worst = max(worst, err)
        assert err <= FD_BAR, (name, k, at, err)
    print(f"{form}: {len(cases_)} entries, worst |fd - g| / max(1, |g|) = {worst:.2e}")


@pytest.mark.parametrize("form", ["ext", "ndp"])
def test_forward_sweep_is_dual_to_the_reverse_sweep(cases, form):
    """<G, dx> + <H, du0> + <A, dX> along T = 2 seeded directions of every leaf = <direction, gradient>: float64 against float64 over the
    same systems, so the gap is rounding.  Found: 1.2e-14 (ext) and 8.5e-15 (ndp) of the largest term; the bar, 1e-12, leaves room for
    another LAPACK's solve of the ~530-row systems."""
    a, kw, rec, ok, which, (G, H, A), sys_ = cases[form]
    B, T = a["x0"].shape[0], 2
    t = R.tangents(K, B, N, T, seed=6, rows=None if form == "ext" else a["other"].shape[1])
    if form == "ext":
        t.pop("t_other", None)
    else:
        t.pop("t_f")
    g = R.reverse(sys_, rec, G, H, A)
    dx, du0, dX = R.forward(sys_, rec, **t)
    lhs = (np.einsum("kvtc,kvc->t", dx, G[:, which]) + np.einsum("kvtc,kvc->t", du0, H[:, which])
           + np.einsum("kvtnc,kvnc->t", dX, A[:, which]))
    terms = [np.einsum("vtc,vc->t", t["t_x0"][which], g["x0"]), np.einsum("kvtnc,kvnc->t", t["t_xr"][:, which], g["xr"]),
             np.einsum("kvtnc,kvnc->t", t["t_ur"][:, which], g["ur"]), np.einsum("kvtc,kvc->t", t["t_fp"][:, which], g["fp"])]
    if form == "ext":
        terms.append(np.einsum("kvtnc,kvnc->t", t["t_f"][:, which], g["f"]))
    else:
        terms += [np.einsum("krtnc,krnc->t", t["t_other"], g["other"]), t["t_w"].astype(np.float64) @ g["w"]]
    rhs = np.sum(terms, axis=0)
    gap = np.abs(lhs - rhs) / max(np.abs(np.array(terms)).max(), np.abs(lhs).max())
    print(f"{form}: duality gap {gap.max():.2e} of the largest term")
    assert gap.max() <= 1e-12


# ---------------------------------------------------------------- the graph's shape, on a stub engine
class _StubLoop:
    """An engine on CPU tensors whose step is u0 = 2 x0[:, :4], X = 3 xr and whose plant is x' = 5 x + pad(u): linear, so every upstream is
    known in closed form.  It numbers its steps, hands the number out as the tape, and logs every derivative call."""

    def __init__(self, B, N):
        self.B, self.N, self.steps, self.log = B, N, 0, []

    def record_tape(self, stream=None):
        import torch
        return (torch.full((1,), float(self.steps), dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int8))

    def update_device(self, x0, xr, ur, u0, f=None, other=None, ego_xy=None, stream=None, other_index=None):
        self.steps += 1
        self._X, self._U = 3.0 * xr, ur.clone()
        u0.copy_(2.0 * x0[:, :4])

    def device_iterate(self):
        return self._X, self._U

    def step_vjp_device(self, x0, xr, ur, tape, gu0=None, gX=None, gU=None, f=None, gx0=None, gxr=None, gur=None, gf=None, stream=None):
        gx0.zero_()
        gx0[:, :4] = 2.0 * gu0
        for out in (gxr, gur, gf):
            if out is not None:
                out.zero_()
        self.log.append(("step", int(tape[0][0]), x0.clone(), gu0.clone(), None if gX is None else gX.clone(), gx0.clone()))

    def plant_rollout_device(self, x0, u, xs, f=None, dt=None, substeps=None, stream=None):
        xs[0] = 5.0 * x0
        xs[0][:, :4] += u[0]

    def plant_rollout_vjp_device(self, x0, u, xs, gxs, f=None, gx0=None, gu=None, gf=None, dt=None, substeps=None, stream=None):
        if gx0 is not None:
            gx0.copy_(5.0 * gxs[0])
        if gu is not None:
            gu[0] = gxs[0][:, :4]
        if gf is not None:
            gf.zero_()
        self.log.append(("plant", x0.clone(), gxs[0].clone(), 5.0 * gxs[0]))

    def synchronize(self):
        pass


def test_three_ticks_on_a_stub_engine_build_the_promised_graph():
    """K = 3 ticks of control_step_trajectory -> plant_step: the backward calls step_vjp_device once per tick, last tick first, each
    with its own tick's tape, x0 and upstreams (g_u0 = H_k + the plant's gu, g_X = A_k), and tick k's step g_x0 plus its plant g_x arrive,
    with G_{k-1}, as tick k-1's plant upstream."""
    import torch
    from ndp_nmpc_qd_amd.torch_layer import control_step_trajectory, plant_step
    B = 3
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    eng = _StubLoop(B, N)
    x = r(B, 10).requires_grad_(True)
    x_first = x
    G, H, A = r(K, B, 10), r(K, B, 4), r(K, B, N + 1, 10)
    xs, L = [], 0.0
    for k in range(K):
        xr, ur = r(B, N + 1, 10).requires_grad_(True), r(B, N, 4)
        u0, X, U = control_step_trajectory(eng, x, xr, ur)
        xs.append(x.detach().clone())
        x = plant_step(eng, x, u0)
        L = L + (G[k] * x).sum() + (H[k] * u0).sum() + (A[k] * X).sum()
    assert eng.steps == K and not eng.log
    L.backward()
    kinds = [e[0] for e in eng.log]
    assert kinds == ["plant", "step"] * K
    steps = [e for e in eng.log if e[0] == "step"]
    plants = [e for e in eng.log if e[0] == "plant"]
    assert [e[1] for e in steps] == [2, 1, 0]                                   # once per tick, in reverse order, each with its own tape
    for j, k in enumerate((2, 1, 0)):
        assert torch.equal(steps[j][2], xs[k]) and torch.equal(plants[j][1], xs[k])
        up = G[k] if k == K - 1 else G[k] + steps[j - 1][5] + plants[j - 1][3]  # tick k + 1's g_x0 (step and plant) arrives here
        assert torch.allclose(plants[j][2], up, rtol=0, atol=1e-13)
        assert torch.allclose(steps[j][3], H[k] + plants[j][2][:, :4], rtol=0, atol=1e-13) and torch.equal(steps[j][4], A[k])
    assert torch.allclose(x_first.grad, steps[-1][5] + plants[-1][3], rtol=0, atol=1e-12)
