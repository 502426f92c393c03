// rows.hip -- the rows either side of the control step, kernels and entry points: f1 the reference window and the reference's sliding
// list (ref_window_kernel, ref_list_*_kernel), f2 the follower relay, f3 the hover-throttle estimator and the actuator command, f4 the
// plant and the closed-loop rollouts (rollout_head: what all three start with; rollout_formation: both formation rollouts; their force on the
// plant: downwash.hip).  (A reference point itself, the list store and the estimator's update: ref_point.hpp.)
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "host.hpp"
#include "mlp_common.hpp"
#include "plant_dyn.hpp"
#include "ref_point.hpp"

namespace ndp {

// ------------------------------------------------------------------------------------------ f3 kernels
// Hover-throttle estimator (2-state Kalman filter on [f_collect, k_throttle] + Tustin differentiator), one thread
// per vehicle.  Elementwise and HBM-bound: state is SoA ([8][B] doubles) so every access is a coalesced 512-B wave
// load/store; 152 algorithmic bytes per vehicle and tick.  Operation order follows the reference's numpy
// expressions (hover_throttle_estimator.py:38-51) so results agree to rounding.

// Streaming (non-temporal) accesses of the rows' kernels: outputs nobody reads again in the same launch, inputs read once.  With plain
// stores ref_window_kernel ran at 0.45 of the HBM roof although its loads + arithmetic alone take 75 us and its arithmetic + stores
// alone 111 us of the 187 (knock-out builds, round 5): the 616 MB of window rows went through L2 as ordinary dirty lines and every
// wave's dependent load rounds queued behind them.  `nt`: 137 us (0.62).
typedef double nt_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_stream(double2 *p, const double2 &v)
{
    const nt_d2 t = {v.x, v.y};
    __builtin_nontemporal_store(t, reinterpret_cast<nt_d2 *>(p));
}
__device__ __forceinline__ void st_stream(double *p, double v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ double2 ld_stream(const double2 *p)
{
    const nt_d2 t = __builtin_nontemporal_load(reinterpret_cast<const nt_d2 *>(p));
    return make_double2(t.x, t.y);
}

__global__ __launch_bounds__(256) void throttle_kernel(ThrCfg c, double *__restrict__ st, const double *__restrict__ vz,
                                                       const double *__restrict__ throttle, double *__restrict__ k_out, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    k_out[v] = throttle_update_one(c, st, (size_t)B, v, vz[v], throttle[v]);
}

__global__ __launch_bounds__(256) void throttle_reset_kernel(double *st, double k_init, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    const size_t S = (size_t)B;
    st[0 * S + v] = 0.0; st[1 * S + v] = k_init;
    st[2 * S + v] = 1.0; st[3 * S + v] = 0.0; st[4 * S + v] = 0.0; st[5 * S + v] = 1.0;
    st[6 * S + v] = 0.0; st[7 * S + v] = 0.0;
}

// nmpc_u_2_att_tgt (nmpc_node.py:273-283): body rates pass through, thrust = c * mass / k_throttle (0 if k == 0)
__device__ __forceinline__ double thrust_cmd(double c, double mass, double k) { return k != 0.0 ? nc_mul(c, mass) / k : 0.0; }
__global__ __launch_bounds__(256) void actuator_kernel(const double *__restrict__ u0, const double *__restrict__ k,
                                                       double *__restrict__ cmd, double mass, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    const double2 a = reinterpret_cast<const double2 *>(u0)[2 * v], b = reinterpret_cast<const double2 *>(u0)[2 * v + 1];
    const double kk = k[v];
    double2 o0 = a, o1 = b;
    o1.y = thrust_cmd(b.y, mass, kk);
    reinterpret_cast<double2 *>(cmd)[2 * v] = o0;
    reinterpret_cast<double2 *>(cmd)[2 * v + 1] = o1;
}

// ------------------------------------------------------------------------------------------ f2 kernels
// AlphaFilter per instance and axis (alpha_filter.py:19; individually rounded like the Python expression)
__global__ __launch_bounds__(256) void relay_formation_kernel(double alpha, double *__restrict__ st, const double *__restrict__ form, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    const bool init = st[v * 4 + 3] != 0.0;
    const double oma = 1.0 - alpha;
    for (int a = 0; a < 3; ++a) {
        const double u = form[v * 3 + a];
        const double y = init ? st[v * 4 + a] : u;
        st[v * 4 + a] = nc_add(nc_mul(alpha, y), nc_mul(oma, u));
    }
    st[v * 4 + 3] = 1.0;
}

// follower reference = leader window with the filtered offset added to the positions.  HBM-bound: 3360 B per instance at N = 20.
// A dense copy in 16-byte pieces (piece p: row p / 5, doubles 2 (p % 5) and + 1 of it), the offset added to pieces 0 (x, y) and 1 (z):
// every instruction of a wave covers 1 KB of contiguous memory on both sides, the output streams (st_stream).  As one thread per ROW
// -- five pieces at an 80-byte lane stride -- each instruction touched 40 lines a fifth each: 195 us for 262 144 windows (0.58 of the
// roof); that form with streaming loads / stores: 685 us, every partial line fetched again by each of its five instructions.
enum { RELAY_UNROLL = 4 };
__global__ __launch_bounds__(256) void relay_reference_kernel(const double *__restrict__ st, const double *__restrict__ xr_lead,
                                                              double *__restrict__ xr_out, int rows, int np1)
{
    const size_t total = (size_t)rows * 5;
    const size_t p0 = (size_t)blockIdx.x * (256 * RELAY_UNROLL) + threadIdx.x;
    const double2 *src = reinterpret_cast<const double2 *>(xr_lead);
    double2 *dst = reinterpret_cast<double2 *>(xr_out);
    double2 v[RELAY_UNROLL], o[RELAY_UNROLL];
#pragma unroll
    for (int j = 0; j < RELAY_UNROLL; ++j) {
        const size_t p = p0 + (size_t)j * 256, pc = p < total ? p : total - 1;
        const int r = (int)(pc / 5), c = (int)(pc - (size_t)r * 5), inst = r / np1;
        v[j] = src[pc];
        o[j] = make_double2(0.0, 0.0);
        if (c == 0) o[j] = *reinterpret_cast<const double2 *>(st + (size_t)inst * 4);        // (ox, oy)
        else if (c == 1) o[j].x = st[(size_t)inst * 4 + 2];                                   // (oz, -)
    }
#pragma unroll
    for (int j = 0; j < RELAY_UNROLL; ++j) {
        const size_t p = p0 + (size_t)j * 256;
        const int c = (int)(p % 5);
        double2 w = v[j];
        if (c == 0) { w.x += o[j].x; w.y += o[j].y; }
        else if (c == 1) w.x += o[j].x;
        if (p < total) st_stream(dst + p, w);
    }
}

// ------------------------------------------------------------------------------------------ f4 kernel
// plant: the OCP's own dynamics, RK4 substeps, quaternion renormalised -- the tick's arithmetic is plant_tick (plant_dyn.hpp), shared
// with the rollout over an input sequence (plant_deriv.hip), whose log rows are these results bit for bit
__global__ __launch_bounds__(256) void plant_kernel(double *__restrict__ x, const double *__restrict__ u, const double *__restrict__ f,
                                                    double h, int sub, double inv_mass, double g, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    double xv[10], uv[4];
    plant_ld_row<5>(x + (size_t)v * 10, xv);
    plant_ld_row<2>(u + (size_t)v * 4, uv);
    plant_tick(xv, uv, f, (size_t)v * 3, h, sub, inv_mass, g);
    plant_st_row<5>(x + (size_t)v * 10, xv);
}

// the formation rollout's worst status per vehicle: the first tick writes it, the later ones keep the larger value
__global__ __launch_bounds__(256) void status_max_kernel(const int *__restrict__ status, int *__restrict__ worst, int first, int B)
{
    const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (v >= B) return;
    const int st = status[v];
    worst[v] = first || st > worst[v] ? st : worst[v];
}

#define REF_ROWS 64     // rows (vehicle, node) per workgroup = one wave: small batches spread over all CUs
// What binds it (round 5, knock-out builds at 262 144 windows, 187 us as it stood): loads + arithmetic alone 75 us, arithmetic + stores
// alone 111 us (5.5 TB/s of writes: the device's fill ceiling), loads + stores WITHOUT the arithmetic 168 us -- the two memory phases
// did not overlap across waves: the 616 MB of output went through L2 as ordinary dirty lines and the dependent load rounds of the
// other waves (time -> segment -> coefficients) queued behind them.  Streaming stores (st_stream): 127-137 us, 0.62-0.68 of the roof.
// Not what binds it, each measured: the number of load instructions (coefficients as 14 16-byte loads: +2.6 %; from the scalar
// cache instead, a timing experiment: nothing), the number of dependent rounds (a branch-free scan that merges two of the three rounds
// but requests six more time_cum entries: 13 % SLOWER), occupancy (64 registers for 8 waves spills and is slower).  ONE 5 KB staging
// buffer used twice (x rows, then u rows): 7 KB per wave had capped a CU at 22 workgroups.
__global__ __launch_bounds__(REF_ROWS)
void ref_window_kernel(RefCfg cf, const double *__restrict__ coeff, const double *__restrict__ tcum,
                       const double *__restrict__ tseg, const double *__restrict__ fpt,
                       const double *__restrict__ tq, double *__restrict__ xr, double *__restrict__ ur)
{
    // Each lane produces 80 + 32 contiguous bytes; written directly that is a 16-byte store at an 80-byte lane stride
    // (one fifth of every cache line per instruction).  The wave's rows are contiguous in xr (and, minus the node-N
    // rows, in ur), so the outputs are transposed through LDS and leave as dense 1024-byte wave stores.
    __shared__ __attribute__((aligned(16))) double sx[REF_ROWS * 10];
    const int lane = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * REF_ROWS;
    const int np1 = cf.N + 1, nrows = cf.B * np1;
    const int row = row0 + lane < nrows ? row0 + lane : nrows - 1;      // tail lanes recompute the last row, never store
    const int b = row / np1, k = row - b * np1;
    const double t = (tq ? tq[b] : 0.0) + cf.toff + k * cf.dt;
    double xv[10], uv[4];
    ref_point(cf, coeff, tcum, tseg, fpt, b, t, xv, uv);
#pragma unroll
    for (int i = 0; i < 5; ++i) reinterpret_cast<double2 *>(sx)[lane * 5 + i] = make_double2(xv[2 * i], xv[2 * i + 1]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int rows_here = nrows - row0 < REF_ROWS ? nrows - row0 : REF_ROWS;
    // 16 bytes per lane and store (rows are 80 / 32 bytes: both arrays stay 16-byte aligned at every row)
    double2 *xg = reinterpret_cast<double2 *>(xr + (size_t)row0 * 10);
    const double2 *s2 = reinterpret_cast<const double2 *>(sx);
    for (int i = lane; i < rows_here * 5; i += REF_ROWS) st_stream(xg + i, s2[i]);
    // ur has no node-N rows: the number of u rows before row (b, k) is b N + k = row - b
    const int ufirst = row0 - row0 / np1;
    const int uslot = (row - b) - ufirst;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();                                        // every lane has read its x pieces: the buffer is free
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (k < cf.N && row0 + lane < nrows) {
        reinterpret_cast<double2 *>(sx)[uslot * 2] = make_double2(uv[0], uv[1]);
        reinterpret_cast<double2 *>(sx)[uslot * 2 + 1] = make_double2(uv[2], uv[3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int rend = row0 + rows_here;
    const int nu = (rend - rend / np1) - ufirst;                                 // u rows among [row0, rend)
    double2 *ug = reinterpret_cast<double2 *>(ur + (size_t)ufirst * 4);
    for (int i = lane; i < nu * 2; i += REF_ROWS) st_stream(ug + i, s2[i]);
}

// ---- f1, the reference's own bookkeeping: NMPCRefPublisher keeps a list of `ring` = step N + 1 reference points per vehicle,
// ts_nmpc apart (pt_publisher.py:36-38, params/nmpc_params.py:40-43; step = 5); every control tick drops the oldest and appends
// the point at ros_t + T_horizon (:78-97); the controller's window is every step-th entry (:99-103).
// Device layout (round 5): the window of tick n is the list entries with ABSOLUTE index n, n + step, .., n + step N (entry j =
// the j-th point ever put into the list) -- all of one residue class mod step.  So the list is kept PHASE-MAJOR, a short ring of
// N + 1 positions per phase, every entry stored twice, N + 1 positions apart:
//     x ring [B][step][2 (N+1)][10]      u ring [B][step][2 (N+1)][4]
//     entry j -> phase j % step, positions (j / step) % (N+1) and + (N+1)
// and every window is N + 1 CONTIGUOUS x rows (N u rows) starting at position (n / step) % (N+1) of phase n % step: the control
// step reads its reference window -- and a neighbour's -- straight out of the list (instance pitch = RingGeom::px / pu doubles),
// there is no window copy on the control tick's path, and the stand-alone window call is a dense copy.  `n` lives on the host
// (ndp_handle::list_n) and is baked into each launch's arguments.

// Fills list entries: point i of vehicle b at trajectory time (tq ? tq[b] : 0) + toff + i * tstep becomes entry j0 + i;
// dup0 also makes point 0 entry j0 - 1 (_gen_long_list_w_traj's duplicate, :73-74).
__global__ __launch_bounds__(256) void ref_list_fill_kernel(RefCfg cf, const double *__restrict__ coeff, const double *__restrict__ tcum,
                                                            const double *__restrict__ tseg, const double *__restrict__ fpt,
                                                            const double *__restrict__ tq, double tstep, int npts, unsigned long long j0,
                                                            RingGeom rg, int dup0, double *__restrict__ rx, double *__restrict__ ru)
{
    const int id = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (id >= cf.B * npts) return;
    const int b = id / npts, i = id - b * npts;
    double xv[10], uv[4];
    // one point per vehicle = the per-tick advance: the segment hint applies (it lives behind final_pt, see ndp_ref_set_trajectory)
    int *hint = npts == 1 ? reinterpret_cast<int *>(const_cast<double *>(fpt + (size_t)cf.B * 3 + (size_t)cf.B * SEGC_PER)) : nullptr;
    ref_point(cf, coeff, tcum, tseg, fpt, b, (tq ? tq[b] : 0.0) + cf.toff + i * tstep, xv, uv, hint);
    ring_store(rg, rx, ru, b, j0 + (unsigned long long)i, xv, uv);
    if (dup0 && i == 0) ring_store(rg, rx, ru, b, j0 - 1, xv, uv);
}

// gen_fix_pt_ref (pt_publisher.py:40-55): every entry = the odometry state, u = [0, 0, 0, c_hover]; one thread per stored row
__global__ __launch_bounds__(256) void ref_list_fix_kernel(const double *__restrict__ x_odom, double c_hover, int B, RingGeom rg,
                                                           double *__restrict__ rx, double *__restrict__ ru)
{
    const int per = rg.step * 2 * rg.np1;
    const int id = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (id >= B * per) return;
    const int b = id / per;
    const double2 *s = reinterpret_cast<const double2 *>(x_odom) + (size_t)b * 5;
    double2 *dx = reinterpret_cast<double2 *>(rx) + (size_t)id * 5, *du = reinterpret_cast<double2 *>(ru) + (size_t)id * 2;
#pragma unroll
    for (int c = 0; c < 5; ++c) dx[c] = s[c];
    du[0] = make_double2(0.0, 0.0);
    du[1] = make_double2(0.0, c_hover);
}

// get_nmpc_ref_from_long_list (:99-103) as a stand-alone call: the window of tick n -> xr[B][N+1][10], ur[B][N][4].  Both sides
// are contiguous per vehicle (see RingGeom): a dense copy, 16 bytes per lane -- 5 (N+1) + 2 N pieces per vehicle.
enum { WIN_UNROLL = 4 };      // 16-byte pieces per thread, a block apart: four loads in flight per lane before the first store
__global__ __launch_bounds__(256) void ref_list_window_kernel(const double *__restrict__ rx, const double *__restrict__ ru, RingGeom rg,
                                                              unsigned long long n, int B, double *__restrict__ xr, double *__restrict__ ur)
{
    const int N = rg.np1 - 1, nxp = 5 * rg.np1, per = nxp + 2 * N;
    const size_t total = (size_t)B * per, s = rg.slot(n);
    const size_t id0 = (size_t)blockIdx.x * (256 * WIN_UNROLL) + threadIdx.x;
    double2 v[WIN_UNROLL];
    double2 *dst[WIN_UNROLL];
#pragma unroll
    for (int j = 0; j < WIN_UNROLL; ++j) {
        const size_t id = id0 + (size_t)j * 256;
        const size_t idc = id < total ? id : total - 1;
        const int b = (int)(idc / per), e = (int)(idc - (size_t)b * per);
        const double2 *src = e < nxp ? reinterpret_cast<const double2 *>(rx + (size_t)b * rg.px() + s * 10) + e
                                     : reinterpret_cast<const double2 *>(ru + (size_t)b * rg.pu() + s * 4) + (e - nxp);
        dst[j] = id < total ? (e < nxp ? reinterpret_cast<double2 *>(xr) + (size_t)b * nxp + e
                                       : reinterpret_cast<double2 *>(ur) + (size_t)b * 2 * N + (e - nxp)) : nullptr;
        v[j] = *src;
    }
#pragma unroll
    for (int j = 0; j < WIN_UNROLL; ++j)
        if (dst[j]) st_stream(dst[j], v[j]);
}

}  // namespace ndp

using namespace ndp;

extern "C" {

// ---- f3: hover-throttle estimator + actuator command (reference constants: params/estimator_params.py:13-18)
ThrCfg thr_cfg(const ndp_handle *h)
{
    const double ts = 0.02, tau = 0.05;
    ThrCfg c;
    c.a1 = (2.0 * tau - ts) / (2.0 * tau + ts);
    c.a2 = 2.0 / (2.0 * tau + ts);
    c.hm = 1.0 / h->cfg.mass;
    c.g = h->cfg.gravity;
    c.R = 1.225; c.Q0 = 0.1; c.Q1 = 0.1;
    c.mass = h->cfg.mass;
    return c;
}

// the estimator's initial state on the handle's stream (ndp_create, ndp_throttle_reset)
void launch_throttle_reset(const ndp_handle *h)
{
    hipLaunchKernelGGL(throttle_reset_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, h->stream, h->dThr, 50.0, h->cfg.batch);
}

int ndp_throttle_reset(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    launch_throttle_reset(h);
    NDP_HIP(h, hipGetLastError());
    return g.synced(0);
}

// The host-pointer forms below hold the handle's lock from the first staging copy to the read-back: they share the
// staging area sThr (and sx0 / sxr / sur / su0 of the step), which a concurrent call must not overwrite in between.
static int launch_throttle(ndp_handle *h, const double *d_vz, const double *d_throttle, double *d_k, hipStream_t s)
{
    hipLaunchKernelGGL(throttle_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, s, thr_cfg(h), h->dThr, d_vz, d_throttle, d_k, h->cfg.batch);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_throttle_update_device(ndp_handle *h, const void *d_vz, const void *d_throttle, void *d_k, void *stream)
{
    Entry g(h, d_vz && d_throttle && d_k, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_throttle(h, (const double *)d_vz, (const double *)d_throttle, (double *)d_k, g.s));
}

int ndp_throttle_update(ndp_handle *h, const double *vz, const double *throttle, double *k)
{
    Entry g(h, vz && throttle && k);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, vz, B * 8, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->sThr + B, throttle, B * 8, hipMemcpyHostToDevice, h->stream));
    int rc = launch_throttle(h, h->sThr, h->sThr + B, h->sThr + 2 * B, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(k, h->sThr + 2 * B, B * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

static int launch_actuator(ndp_handle *h, const double *d_u0, const double *d_k, double *d_cmd, hipStream_t s)
{
    hipLaunchKernelGGL(actuator_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, s, d_u0, d_k, d_cmd, h->cfg.mass, h->cfg.batch);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_actuator_cmd_device(ndp_handle *h, const void *d_u0, const void *d_k, void *d_cmd, void *stream)
{
    Entry g(h, d_u0 && d_k && d_cmd, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_actuator(h, (const double *)d_u0, (const double *)d_k, (double *)d_cmd, g.s));
}

int ndp_actuator_cmd(ndp_handle *h, const double *u0, const double *k, double *cmd)
{
    Entry g(h, u0 && k && cmd);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sThr + 2 * B, k, B * 8, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->sThr + 3 * B, u0, B * 32, hipMemcpyHostToDevice, h->stream));
    int rc = launch_actuator(h, h->sThr + 3 * B, h->sThr + 2 * B, h->sThr + 7 * B, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(cmd, h->sThr + 7 * B, B * 32, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

int ndp_throttle_get_state(ndp_handle *h, double *state)
{
    Entry g(h, state);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    int rc = wait_all(h);
    if (rc) return rc;
    std::vector<double> soa(B * 8);
    NDP_HIP(h, hipMemcpy(soa.data(), h->dThr, B * 64, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < B; ++v)
        for (int i = 0; i < 8; ++i) state[v * 8 + i] = soa[(size_t)i * B + v];
    return 0;
}

// ---- f2: follower reference relay
int ndp_relay_reset(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemsetAsync(h->dRelay, 0, (size_t)h->cfg.batch * 32, h->stream));
    return g.synced(0);
}

int ndp_relay_formation(ndp_handle *h, const double *form, double *offset_out)
{
    Entry g(h, form);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, form, B * 24, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(relay_formation_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, 0.8, h->dRelay, (const double *)h->sThr, (int)B);
    NDP_HIP(h, hipGetLastError());
    std::vector<double> st(offset_out ? B * 4 : 0);
    if (offset_out) NDP_HIP(h, hipMemcpyAsync(st.data(), h->dRelay, B * 32, hipMemcpyDeviceToHost, h->stream));
    int rc = g.synced(0);
    if (rc) return rc;
    for (size_t v = 0; offset_out && v < B; ++v)
        for (int a = 0; a < 3; ++a) offset_out[v * 3 + a] = st[v * 4 + a];
    return 0;
}

static int launch_relay_reference(ndp_handle *h, const double *d_xr_lead, double *d_xr_out, hipStream_t s)
{
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const size_t pieces = (size_t)rows * 5, per_block = 256 * RELAY_UNROLL;
    hipLaunchKernelGGL(relay_reference_kernel, dim3((unsigned)((pieces + per_block - 1) / per_block)), dim3(256), 0, s, (const double *)h->dRelay, d_xr_lead, d_xr_out, rows, np1);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_relay_reference_device(ndp_handle *h, const void *d_xr_lead, void *d_xr_out, void *stream)
{
    Entry g(h, d_xr_lead && d_xr_out, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_relay_reference(h, (const double *)d_xr_lead, (double *)d_xr_out, g.s));
}

int ndp_relay_reference(ndp_handle *h, const double *xr_lead, double *xr_out)
{
    Entry g(h, xr_lead && xr_out);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemcpyAsync(h->sother, xr_lead, nxs(h) * 8, hipMemcpyHostToDevice, h->stream));
    int rc = launch_relay_reference(h, h->sother, h->sxr, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(xr_out, h->sxr, nxs(h) * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- f1: reference window generation
int ndp_ref_set_trajectory(ndp_handle *h, int n_seg, const double *coeff_x, const double *coeff_y, const double *coeff_z,
                           const double *coeff_yaw, const double *time_cum, const double *time_seg, const double *final_pt)
{
    Entry g(h, n_seg >= 1 && coeff_x && coeff_y && coeff_z && coeff_yaw && time_cum && time_seg && final_pt);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch, S = (size_t)n_seg;
    std::vector<double> host(traj_view(nullptr, B, S).doubles);     // (the hints start at 0)
    const TrajView v = traj_view(host.data(), B, S);
    for (size_t b = 0; b < B; ++b)
        for (size_t s = 0; s < S; ++s) {
            double *d = v.coeff + (b * S + s) * 28;          // interleave the four message arrays per segment
            for (int i = 0; i < 8; ++i) {
                d[i] = coeff_x[(b * S + s) * 8 + i];
                d[8 + i] = coeff_y[(b * S + s) * 8 + i];
                d[16 + i] = coeff_z[(b * S + s) * 8 + i];
            }
            for (int i = 0; i < 4; ++i) d[24 + i] = coeff_yaw[(b * S + s) * 4 + i];
        }
    memcpy(v.tcum, time_cum, B * (S + 1) * 8);
    memcpy(v.tseg, time_seg, B * S * 8);
    memcpy(v.fpt, final_pt, B * 3 * 8);
    for (double *c : v.segc) memset(c, 0xFF, B * SEGC_PER * 8);
    int rc = wait_all(h);
    if (rc) return rc;
    NDP_HIP(h, h->dTraj.alloc(v.doubles * 8));
    NDP_HIP(h, hipMemcpy(h->dTraj, host.data(), v.doubles * 8, hipMemcpyHostToDevice));
    h->segc_par = 0;
    h->traj_seg = n_seg;
    return 0;
}

RefCfg ref_cfg(const ndp_handle *h, double toff)
{
    return RefCfg{h->cfg.batch, h->cfg.N, h->traj_seg, h->cfg.dt, h->cfg.mass, h->cfg.gravity, toff};
}

// enqueue helper (no locking): windows at node-0 times d_t[b] (or 0 when null) + toff
static int launch_ref_window(ndp_handle *h, const double *d_t, double toff, double *d_xr, double *d_ur, hipStream_t s)
{
    if (!h->dTraj) { h->err = "ndp_ref_window: ndp_ref_set_trajectory was never called"; return -11; }
    const TrajView tv = traj_view(h);
    const int rows = h->cfg.batch * (h->cfg.N + 1);
    hipLaunchKernelGGL(ref_window_kernel, dim3((rows + REF_ROWS - 1) / REF_ROWS), dim3(REF_ROWS), 0, s, ref_cfg(h, toff), tv.coeff, tv.tcum, tv.tseg,
                       tv.fpt, d_t, d_xr, d_ur);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_ref_window_device(ndp_handle *h, const void *d_t, void *d_xr, void *d_ur, void *stream)
{
    Entry g(h, d_t && d_xr && d_ur, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_ref_window(h, (const double *)d_t, 0.0, (double *)d_xr, (double *)d_ur, g.s));
}

int ndp_ref_window(ndp_handle *h, const double *t, double *xr, double *ur)
{
    Entry g(h, t && xr && ur);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, t, (size_t)h->cfg.batch * 8, hipMemcpyHostToDevice, h->stream));
    int rc = launch_ref_window(h, h->sThr, 0.0, h->sxr, h->sur, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(xr, h->sxr, nxs(h) * 8, hipMemcpyDeviceToHost, h->stream));
    NDP_HIP(h, hipMemcpyAsync(ur, h->sur, nus(h) * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- f1, the reference's sliding list (ref_list_* kernels; layout: RingGeom)
static int list_ring(const ndp_handle *h) { return ring_geom(h).ring(); }

static int list_alloc(ndp_handle *h)
{
    if (h->dRingX) return 0;
    const RingGeom rg = ring_geom(h);
    NDP_HIP(h, h->dRingX.alloc((size_t)h->cfg.batch * (rg.px() + rg.pu()) * 8));
    h->dRingU = h->dRingX + (size_t)h->cfg.batch * rg.px();
    return 0;
}

// points at (d_t ? d_t[b] : 0) + toff + i * ts_nmpc, i = 0 .. npts-1, become list entries j0 + i (dup0: point 0 also entry j0 - 1)
static int launch_list_fill(ndp_handle *h, const double *d_t, double toff, int npts, unsigned long long j0, int dup0, hipStream_t s)
{
    if (!h->dTraj) { h->err = "ndp_ref_list: ndp_ref_set_trajectory was never called"; return -11; }
    const TrajView tv = traj_view(h);
    const int n = h->cfg.batch * npts;
    const int bs = npts == 1 ? 64 : 256;        // one point per vehicle (the per-tick advance): small blocks spread over the CUs
    hipLaunchKernelGGL(ref_list_fill_kernel, dim3((n + bs - 1) / bs), dim3(bs), 0, s, ref_cfg(h, toff), tv.coeff, tv.tcum, tv.tseg, tv.fpt, d_t,
                       h->cfg.ts_nmpc, npts, j0, ring_geom(h), dup0, h->dRingX, h->dRingU);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_ref_list_reset(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = list_alloc(h);
    if (rc) return rc;
    if ((rc = wait_all(h))) return rc;
    h->list_n = 0;
    // entries 1 .. ring-1 = the points at i * ts_nmpc, i = 0 .. ring-2; the first one duplicated as entry 0 (:62-76)
    return g.synced(launch_list_fill(h, nullptr, 0.0, list_ring(h) - 1, 1, 1, h->stream));
}

int ndp_ref_list_fix_pt(ndp_handle *h, const double *x_odom, int quirk_b1)
{
    Entry g(h, x_odom);
    if (g.rc) return g.rc;
    int rc = list_alloc(h);
    if (rc) return rc;
    if ((rc = wait_all(h))) return rc;
    h->list_n = 0;
    NDP_HIP(h, hipMemcpyAsync(h->sThr, x_odom, (size_t)h->cfg.batch * 80, hipMemcpyHostToDevice, h->stream));
    const RingGeom rg = ring_geom(h);
    const size_t n = (size_t)h->cfg.batch * rg.step * 2 * rg.np1;
    hipLaunchKernelGGL(ref_list_fix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->sThr,
                       quirk_b1 ? h->cfg.mass * h->cfg.gravity : h->cfg.gravity, h->cfg.batch, rg, h->dRingX, h->dRingU);
    NDP_HIP(h, hipGetLastError());
    return g.synced(0);
}

// pop the oldest entry, append the point at trajectory time t + T_horizon (get_nmpc_pts, :79-93)
static int list_advance(ndp_handle *h, const double *d_t, hipStream_t s)
{
    if (!h->dRingX) { h->err = "ndp_ref_list_advance: no list (ndp_ref_list_reset / ndp_ref_list_fix_pt first)"; return -11; }
    const int rc = launch_list_fill(h, d_t, h->cfg.N * h->cfg.dt, 1, h->list_n + (unsigned long long)list_ring(h), 0, s);
    if (rc) return rc;                                             // nothing was launched (e.g. no trajectory): the list stays as it is
    ++h->list_n;
    return 0;
}

int ndp_ref_list_advance_device(ndp_handle *h, const void *d_t, void *stream)
{
    Entry g(h, d_t, stream);
    if (g.rc) return g.rc;
    return g.noted(list_advance(h, (const double *)d_t, g.s));
}

int launch_list_window(ndp_handle *h, double *d_xr, double *d_ur, hipStream_t s)
{
    if (!h->dRingX) { h->err = "ndp_ref_list_window: no list (ndp_ref_list_reset / ndp_ref_list_fix_pt first)"; return -11; }
    const size_t n = (size_t)h->cfg.batch * (5 * (h->cfg.N + 1) + 2 * h->cfg.N), per_block = 256 * WIN_UNROLL;
    hipLaunchKernelGGL(ref_list_window_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, s, (const double *)h->dRingX,
                       (const double *)h->dRingU, ring_geom(h), h->list_n, h->cfg.batch, d_xr, d_ur);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_ref_list_window_device(ndp_handle *h, void *d_xr, void *d_ur, void *stream)
{
    Entry g(h, d_xr && d_ur, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_list_window(h, (double *)d_xr, (double *)d_ur, g.s));
}

// t == NULL: only read the current window (get_nmpc_ref_from_long_list); else advance first (get_nmpc_pts)
int ndp_ref_list_window(ndp_handle *h, const double *t, double *xr, double *ur)
{
    Entry g(h, xr && ur);
    if (g.rc) return g.rc;
    int rc = 0;
    if (t) {
        NDP_HIP(h, hipMemcpyAsync(h->sThr, t, (size_t)h->cfg.batch * 8, hipMemcpyHostToDevice, h->stream));
        if ((rc = list_advance(h, h->sThr, h->stream))) return rc;
    }
    if ((rc = launch_list_window(h, h->sxr, h->sur, h->stream))) return rc;
    NDP_HIP(h, hipMemcpyAsync(xr, h->sxr, nxs(h) * 8, hipMemcpyDeviceToHost, h->stream));
    NDP_HIP(h, hipMemcpyAsync(ur, h->sur, nus(h) * 8, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- f4: plant step
static int launch_plant(ndp_handle *h, double *d_x, const double *d_u, const double *d_f, double dt, int substeps, hipStream_t s)
{
    const PlantNum p = plant_num(h, dt, substeps);
    hipLaunchKernelGGL(plant_kernel, dim3((h->cfg.batch + 255) / 256), dim3(256), 0, s, d_x, d_u, d_f, p.h, substeps, p.inv_mass, p.g, h->cfg.batch);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_plant_step_device(ndp_handle *h, void *d_x, const void *d_u, const void *d_f, double dt, int substeps, void *stream)
{
    Entry g(h, d_x && d_u && substeps >= 1, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_plant(h, (double *)d_x, (const double *)d_u, (const double *)d_f, dt, substeps, g.s));
}

int ndp_plant_step(ndp_handle *h, double *x, const double *u, const double *f, double dt, int substeps)
{
    Entry g(h, x && u && substeps >= 1);
    if (g.rc) return g.rc;
    const size_t B = h->cfg.batch;
    NDP_HIP(h, hipMemcpyAsync(h->sx0, x, B * 80, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->su0, u, B * 32, hipMemcpyHostToDevice, h->stream));
    if (f) NDP_HIP(h, hipMemcpyAsync(h->sThr, f, B * 24, hipMemcpyHostToDevice, h->stream));
    int rc = launch_plant(h, h->sx0, h->su0, f ? h->sThr : nullptr, dt, substeps, h->stream);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(x, h->sx0, B * 80, hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

// ---- f4: the rollouts.  Their head: the first tick's reference window and reset(xr, ur) on it; clear_act: the kept active sets emptied too
// (the formation rollouts do, ndp_rollout_device does not -- kept as it is)
static int rollout_head(ndp_handle *h, double t0, bool clear_act, hipStream_t s)
{
    int rc = launch_ref_window(h, nullptr, t0, h->sxr, h->sur, s);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(h->dX, h->sxr, nxs(h) * 8, hipMemcpyDefault, s));
    NDP_HIP(h, hipMemcpyAsync(h->dU, h->sur, nus(h) * 8, hipMemcpyDefault, s));
    if (clear_act) NDP_HIP(h, hipMemsetAsync(h->dAct, 0, act_bytes(h), s));
    return 0;
}

// ---- f4: closed-loop rollout, everything enqueued back to back on one stream, nothing returns to the host in between
int ndp_rollout_device(ndp_handle *h, int ticks, double t0, double dt_tick, int substeps, void *d_x, void *d_log, void *stream)
{
    Entry g(h, ticks >= 1 && substeps >= 1 && d_x, stream, "ndp_rollout_device");
    if (g.rc) return g.rc;
    hipStream_t s = g.s;
    if (h->cfg.use_fd) { h->err = "ndp_rollout_device: the rollout drives the NMPC model (use_fd = 0)"; return -8; }
    const size_t B = h->cfg.batch;
    double *x = (double *)d_x, *log = (double *)d_log;
    int rc = rollout_head(h, t0, false, s);
    if (rc) return rc;
    for (int k = 0; k < ticks; ++k) {
        if (k > 0 && (rc = launch_ref_window(h, nullptr, t0 + k * dt_tick, h->sxr, h->sur, s))) return rc;
        if ((rc = launch_rti(h, x, h->sxr, h->sur, nullptr, h->su0, nullptr, s))) return rc;
        if ((rc = launch_plant(h, x, h->su0, nullptr, dt_tick, substeps, s))) return rc;
        if (log) NDP_HIP(h, hipMemcpyAsync(log + (size_t)k * B * NX, x, B * NX * 8, hipMemcpyDeviceToDevice, s));
    }
    return g.noted(0);
}

// ---- f4: closed-loop FORMATION rollout: the rollout above with the downwash acting on the plant, one body for ndp_rollout_formation_device
// (multi false: other_index int32[B], K not read) and ndp_rollout_formation_multi_device (multi: K neighbours per vehicle, forces superposed,
// other_index int32[B][K]), `who` the entry's name.  Per tick: reference window -> the force the neighbours' actual states put on the actual
// vehicle, + the ego xy (launch_plant_force, from the states BEFORE the tick's plant step) -> control step -> plant step with that force,
// held over the tick.  The control step with NDP_FORM_COMPENSATE and an index:
//   single  the fused step of ndp_step_device_ex against this tick's reference windows of the whole batch
//   multi   mlp_multi_kernel on those windows into the handle's force buffer, then the step of ndp_step_device with that force as its
//           external force (no control-step kernel knows about K)
// else the plain step, blind.  u0 and the force are written straight into their log slots when those are given.  Refused (-2: K, multi only;
// then -8) before anything is enqueued.
static int rollout_formation(ndp_handle *h, const char *who, bool multi, int ticks, double t0, double dt_tick, int substeps,
                             const void *d_other_index, int K, int flags, double plant_scale, void *d_x, void *d_log, void *d_log_u,
                             void *d_log_f, void *d_worst_status, void *stream)
{
    Entry g(h, ticks >= 1 && substeps >= 1 && d_x && !(flags & ~(NDP_FORM_GATE | NDP_FORM_COMPENSATE)), stream, who);
    if (g.rc) return g.rc;
    hipStream_t s = g.s;
    const bool comp = (flags & NDP_FORM_COMPENSATE) != 0, gate = (flags & NDP_FORM_GATE) != 0;
    const int *idx = (const int *)d_other_index;
    int rc;
    if (multi && (rc = check_neigh(h, who, K))) return rc;      // (also without an index: an index array of K = 0 may well be NULL)
    const char *why = nullptr;
    if (comp && !h->cfg.use_fd) why = ": NDP_FORM_COMPENSATE needs use_fd = 1 (NDP model)";
    else if (idx && !h->have_mlp) why = ": ndp_set_mlp_weights was never called (the force on the plant is the network's)";
    else if (!h->dTraj) why = ": ndp_ref_set_trajectory was never called";
    if (why) { h->err = std::string(who) + why; return -8; }
    const size_t B = h->cfg.batch;
    double *x = (double *)d_x, *log = (double *)d_log, *log_u = (double *)d_log_u, *log_f = (double *)d_log_f;
    double *xy = h->sThr + 3 * B;                                      // sThr: f [B][3] | xy [B][2]
    Neigh nb;                                                          // (the single form's fused step)
    nb.other = h->sxr; nb.index = idx; nb.ego_xy = gate ? xy : nullptr;
    if ((rc = rollout_head(h, t0, true, s))) return rc;
    for (int k = 0; k < ticks; ++k) {
        double *f = log_f ? log_f + (size_t)k * B * 3 : h->sThr, *u = log_u ? log_u + (size_t)k * B * NU : h->su0;
        if (k > 0 && (rc = launch_ref_window(h, nullptr, t0 + k * dt_tick, h->sxr, h->sur, s))) return rc;
        if ((rc = launch_plant_force(h, x, idx, multi ? K : 0, gate, plant_scale, f, xy, s))) return rc;
        if (comp && idx && multi) {
            if ((rc = launch_mlp_multi(h, h->sxr, NX, idx, K, h->sxr, nb.ego_xy, h->dForce, s))) return rc;
            rc = enqueue_step(h, x, h->sxr, h->sur, h->dForce, Neigh{}, u, nullptr, s);
        } else if (comp && idx) rc = enqueue_step(h, x, h->sxr, h->sur, nullptr, nb, u, nullptr, s);
        else rc = launch_rti(h, x, h->sxr, h->sur, nullptr, u, nullptr, s);
        if (rc) return rc;
        if (d_worst_status) {
            hipLaunchKernelGGL(status_max_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, h->lastStatus, (int *)d_worst_status, k == 0, (int)B);
            NDP_HIP(h, hipGetLastError());
        }
        if ((rc = launch_plant(h, x, u, f, dt_tick, substeps, s))) return rc;
        if (log) NDP_HIP(h, hipMemcpyAsync(log + (size_t)k * B * NX, x, B * NX * 8, hipMemcpyDeviceToDevice, s));
    }
    return g.noted(0);
}

int ndp_rollout_formation_device(ndp_handle *h, int ticks, double t0, double dt_tick, int substeps, const void *d_other_index, int flags,
                                 double plant_scale, void *d_x, void *d_log, void *d_log_u, void *d_log_f, void *d_worst_status, void *stream)
{
    return rollout_formation(h, "ndp_rollout_formation_device", false, ticks, t0, dt_tick, substeps, d_other_index, 0, flags, plant_scale, d_x,
                             d_log, d_log_u, d_log_f, d_worst_status, stream);
}

int ndp_rollout_formation_multi_device(ndp_handle *h, int ticks, double t0, double dt_tick, int substeps, const void *d_other_index, int K,
                                       int flags, double plant_scale, void *d_x, void *d_log, void *d_log_u, void *d_log_f,
                                       void *d_worst_status, void *stream)
{
    return rollout_formation(h, "ndp_rollout_formation_multi_device", true, ticks, t0, dt_tick, substeps, d_other_index, K, flags, plant_scale,
                             d_x, d_log, d_log_u, d_log_f, d_worst_status, stream);
}

}  // extern "C"
