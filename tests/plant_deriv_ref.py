"""float64 numpy reference of the plant over an input sequence and of its derivatives, independent of the device code
(tests/test_plant_rollout.py holds it to the oracle's plant step and to finite differences; tests/test_plant_rollout_gpu.py holds
ndp_plant_rollout*_device to it).

The forward is a transcription of plant_f / plant_kernel: acc = f / mass - g held over the tick, RK4 substeps with u and acc held, the
quaternion renormalised once per tick.  The derivative is the full Jacobian of the flattened log with respect to (x0, u, f) per
vehicle by the complex-step method: the function is a polynomial plus one square root and one division per tick, all analytic, so
Im f(z + i eps) / eps with eps = 1e-30 is the derivative to rounding (no subtraction, no step-size error).  |q| is formed as
sqrt(sum q^2) WITHOUT conjugation, which is what keeps it analytic."""
import numpy as np

from ndp_nmpc_qd_amd.params import nmpc_params as CP

EPS = 1e-30


def plant_f(x, u, acc):
    """x [..., 10], u [..., 4], acc [..., 3] -> dx/dt [..., 10] (real or complex)."""
    qw, qx, qy, qz = x[..., 6], x[..., 7], x[..., 8], x[..., 9]
    d = np.empty_like(x)
    d[..., 0:3] = x[..., 3:6]
    d[..., 3] = 2.0 * (qx * qz + qw * qy) * u[..., 3] + acc[..., 0]
    d[..., 4] = 2.0 * (qy * qz - qw * qx) * u[..., 3] + acc[..., 1]
    d[..., 5] = (1.0 - 2.0 * qx * qx - 2.0 * qy * qy) * u[..., 3] + acc[..., 2]
    d[..., 6] = (-u[..., 0] * qx - u[..., 1] * qy - u[..., 2] * qz) * 0.5
    d[..., 7] = (u[..., 0] * qw + u[..., 2] * qy - u[..., 1] * qz) * 0.5
    d[..., 8] = (u[..., 1] * qw - u[..., 2] * qx + u[..., 0] * qz) * 0.5
    d[..., 9] = (u[..., 2] * qw + u[..., 1] * qx - u[..., 0] * qy) * 0.5
    return d


def tick(x, u, f, dt, substeps, mass, gravity):
    """One tick: x [..., 10] -> the state after dt (`substeps` RK4 steps, then q / |q|)."""
    acc = f / mass
    acc[..., 2] = acc[..., 2] - gravity
    h = dt / substeps
    for _ in range(substeps):
        k1 = plant_f(x, u, acc)
        k2 = plant_f(x + 0.5 * h * k1, u, acc)
        k3 = plant_f(x + 0.5 * h * k2, u, acc)
        k4 = plant_f(x + h * k3, u, acc)
        x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    x = x.copy()
    q = x[..., 6:10]
    x[..., 6:10] = q / np.sqrt((q * q).sum(axis=-1))[..., None]
    return x


def rollout(x0, u, f=None, dt=CP.ts_nmpc, substeps=4, mass=CP.mass, gravity=CP.gravity):
    """x0 [B,10], u [ticks,B,4], f [ticks,B,3] or None -> xs [ticks,B,10] (the dtype of the inputs: real or complex)."""
    ticks = u.shape[0]
    if f is None:
        f = np.zeros(u.shape[:-1] + (3,))
    dtype = np.result_type(x0, u, f)
    x, xs = x0.astype(dtype), []
    for k in range(ticks):
        x = tick(x, u[k].astype(dtype), f[k].astype(dtype), dt, substeps, mass, gravity)
        xs.append(x)
    return np.stack(xs)


def n_in(ticks):
    return 10 + 7 * ticks


def jacobian(x0, u, f=None, dt=CP.ts_nmpc, substeps=4, mass=CP.mass, gravity=CP.gravity):
    """J [B, ticks*10, 10 + ticks*4 + ticks*3]: d xs[:, v].ravel() / d (x0[v], u[:, v].ravel(), f[:, v].ravel()) per vehicle v, by complex
    step.  (With f None the derivative with respect to f is taken at f = 0.)"""
    ticks, B = u.shape[0], u.shape[1]
    if f is None:
        f = np.zeros((ticks, B, 3))
    n = n_in(ticks)
    # one complex rollout of B * n vehicles: copy c of vehicle v has input column c perturbed
    X0 = np.repeat(x0[:, None, :], n, axis=1).astype(complex)                 # [B, n, 10]
    U = np.repeat(u[:, :, None, :], n, axis=2).astype(complex)                # [ticks, B, n, 4]
    F = np.repeat(f[:, :, None, :], n, axis=2).astype(complex)
    for c in range(10):
        X0[:, c, c] += 1j * EPS
    for k in range(ticks):
        for c in range(4):
            U[k, :, 10 + 4 * k + c, c] += 1j * EPS
        for c in range(3):
            F[k, :, 10 + 4 * ticks + 3 * k + c, c] += 1j * EPS
    xs = rollout(X0.reshape(B * n, 10), U.reshape(ticks, B * n, 4), F.reshape(ticks, B * n, 3), dt, substeps, mass, gravity)
    d = xs.imag.reshape(ticks, B, n, 10) / EPS                                # [k, v, column, component]
    return np.ascontiguousarray(d.transpose(1, 0, 3, 2).reshape(B, ticks * 10, n))


def vjp(J, gxs):
    """gxs [ticks,B,10] -> (gx0 [B,10], gu [ticks,B,4], gf [ticks,B,3]) = J' g per vehicle."""
    ticks, B = gxs.shape[0], gxs.shape[1]
    g = np.einsum("bo,boi->bi", gxs.transpose(1, 0, 2).reshape(B, ticks * 10), J)
    gu = g[:, 10:10 + 4 * ticks].reshape(B, ticks, 4).transpose(1, 0, 2)
    gf = g[:, 10 + 4 * ticks:].reshape(B, ticks, 3).transpose(1, 0, 2)
    return g[:, :10].copy(), np.ascontiguousarray(gu), np.ascontiguousarray(gf)


def jvp(J, tx0=None, tu=None, tf=None):
    """tx0 [B,T,10], tu [ticks,B,T,4], tf [ticks,B,T,3] (each None = 0) -> dxs [ticks,B,T,10] = J t per vehicle and direction."""
    B, ticks = J.shape[0], J.shape[1] // 10
    T = next(t.shape[-2] for t in (tx0, tu, tf) if t is not None)
    t = np.zeros((B, T, n_in(ticks)))
    if tx0 is not None:
        t[:, :, :10] = tx0
    if tu is not None:
        t[:, :, 10:10 + 4 * ticks] = tu.transpose(1, 2, 0, 3).reshape(B, T, ticks * 4)
    if tf is not None:
        t[:, :, 10 + 4 * ticks:] = tf.transpose(1, 2, 0, 3).reshape(B, T, ticks * 3)
    d = np.einsum("boi,bti->bto", J, t).reshape(B, T, ticks, 10)
    return np.ascontiguousarray(d.transpose(2, 0, 1, 3))


def inputs(B, ticks, seed, force=True):
    """Inputs from the project's envelope: unit quaternions, body rates in +-6 rad/s, thrust in 0..c_max, forces ~ N(0, 4 N)
    (force False: None).  -> x0 [B,10], u [ticks,B,4], f [ticks,B,3] or None."""
    rng = np.random.default_rng(seed)
    x0 = np.concatenate([rng.normal(0, 2, (B, 3)), rng.normal(0, 2, (B, 3)), rng.normal(0, 1, (B, 4))], axis=1)
    x0[:, 6:] /= np.linalg.norm(x0[:, 6:], axis=1, keepdims=True)
    u = np.concatenate([rng.uniform(CP.w_min, CP.w_max, (ticks, B, 3)), rng.uniform(CP.c_min, CP.c_max, (ticks, B, 1))], axis=2)
    f = rng.normal(0, 4, (ticks, B, 3)) if force else None
    return x0, u, f


def within_bar(dev, ref, bar=1e-13):
    """The project's plant bar, per row (the last axis): |dev - ref| <= bar * max(1, max |ref| of that row).  -> (ok, the worst ratio)."""
    scale = np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
    r = float((np.abs(dev - ref) / scale).max()) if ref.size else 0.0
    return r <= bar, r
