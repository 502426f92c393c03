// tick.hip -- the node's control tick (ndp_tick*), host side.  Host code only (build.HOST_ONLY): the one-launch form's device prologue
// runs inside the control step (tick_wave.hpp), and tick_pre_kernel with launch_tick_pre is in rti_kernels.hip (see there: it shares
// seg_locate with the one-launch ticks).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "host.hpp"

// ------------------------------------------------------------------------------------------ the node's control tick (ndp_tick)
// nmpc_node.py:211-231 for every vehicle of the handle, on the device, references resident: per tick the host hands over the
// odometry states (80 B per vehicle) and a few scalars; everything else the tick needs is already in HBM.
//   tick_pre_kernel  (one thread per vehicle): the reference list's advance -- the point at t + T_horizon becomes the list's newest
//                    entry (get_nmpc_pts, pt_publisher.py:79-97), which is also node N of this tick's window -- and the hover-
//                    throttle estimator's update (hover_throttle_callback, nmpc_node.py:251-253) from vz and the thrust command of
//                    the previous tick
//   rti_kernel       the control step: x0 = the odometry rows, xr / ur / the neighbour's window straight out of the list; its last
//                    store is nmpc_u_2_att_tgt (:273-283): [wx, wy, wz, c mass / k_throttle] where the host reads it (RtiIo::cmd),
//                    the thrust kept on the device for the next estimator update.  (A third launch for that -- tick_post_kernel,
//                    the first form -- cost 4.6 us per tick in the trace for 32 bytes per vehicle.)

using namespace ndp;

extern "C" {

// ---- the node's control tick, end to end on the device (nmpc_node.py:211-231; kernels: rti_kernel<..., TICK>, or tick_pre_kernel + rti_kernel)
int ensure_tick(ndp_handle *h)
{
    if (h->dTickThrust) return 0;
    NDP_HIP(h, h->dTickThrust.alloc((size_t)h->cfg.batch * 8));
    NDP_HIP(h, hipMemsetAsync(h->dTickThrust, 0, (size_t)h->cfg.batch * 8, h->stream));     // AttitudeTarget(): thrust 0 (nmpc_node.py:104)
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ndp_tick_config(ndp_handle *h, const int32_t *other_index, int gate_on_odometry)
{
    Entry g(h, true, nullptr, "ndp_tick_config");
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if ((rc = ensure_tick(h))) return rc;
    const size_t B = h->cfg.batch;
    bool any = false;
    if (other_index)
        for (size_t i = 0; i < B; ++i) {
            if (other_index[i] >= (int32_t)B) { h->err = "ndp_tick_config: other_index names an instance outside the handle"; return -2; }
            any = any || other_index[i] >= 0;
        }
    if (any && !h->cfg.use_fd) { h->err = "ndp_tick_config: neighbours (downwash) need use_fd = 1 (NDP model)"; return -8; }
    if (any && !h->have_mlp) { h->err = "ndp_tick_config: neighbours given but ndp_set_mlp_weights was never called"; return -6; }
    if (any) {
        NDP_HIP(h, h->dTickIndex.ensure(B * 4));
        NDP_HIP(h, hipMemcpy(h->dTickIndex, other_index, B * 4, hipMemcpyHostToDevice));
    } else h->dTickIndex.reset();
    h->tick_gate = gate_on_odometry != 0;
    h->tick_remote = nullptr;
    return 0;
}

// The control tick with neighbours on OTHER ranks (nmpc_node.py:116-133,229-230 -> ndp_nmpc_leader_node.py:40,60-76: every vehicle
// publishes its window every tick, the leader consumes its neighbour's): the neighbour rows come from the caller's exchange buffer, and
// a tick is three enqueues with the exchange between the first two and the last:
//   ndp_tick_advance_device    list advance (+ estimator): this rank's window of the tick is complete, node N included
//   ndp_tick_window_pv_device  that window's position / velocity columns [B][N+1][6] -> the exchange's send buffer   ... exchange ...
//   ndp_tick_step_device       the control step (gate + network + RTI + actuator command), neighbour rows from the gathered windows
// Same arithmetic as the one-launch tick with the neighbour in the same handle (bit-equal: tests/test_tick.py).
int ndp_tick_config_remote(ndp_handle *h, const void *d_windows, int stride, int64_t rows, const int32_t *other_index, int gate_on_odometry)
{
    Entry g(h, d_windows && other_index, nullptr, "ndp_tick_config_remote");
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if ((rc = ensure_tick(h))) return rc;
    if (stride != 6 && stride != NX) { h->err = "ndp_tick_config_remote: stride must be 6 (position / velocity columns) or 10"; return -13; }
    if (!h->cfg.use_fd) { h->err = "ndp_tick_config_remote: neighbours (downwash) need use_fd = 1 (NDP model)"; return -8; }
    if (!h->have_mlp) { h->err = "ndp_tick_config_remote: ndp_set_mlp_weights was never called"; return -6; }
    if (!can_fuse(h)) { h->err = "ndp_tick_config_remote: serves the shapes whose downwash is fused into the control step (N + 1 <= 32, fp64)"; return -12; }
    const size_t B = h->cfg.batch;
    for (size_t i = 0; i < B; ++i)
        if ((int64_t)other_index[i] >= rows) { h->err = "ndp_tick_config_remote: other_index names a row outside the window buffer"; return -2; }
    NDP_HIP(h, h->dTickIndex.ensure(B * 4));
    NDP_HIP(h, hipMemcpy(h->dTickIndex, other_index, B * 4, hipMemcpyHostToDevice));
    h->tick_gate = gate_on_odometry != 0;
    h->tick_remote = (const double *)d_windows;
    h->tick_remote_stride = stride;
    return 0;
}

// nmpc_ctl.reset(*ref_pub.get_nmpc_ref_from_long_list()) (nmpc_node.py:92,151-152): the iterate := the list's current window
int ndp_tick_reset(ndp_handle *h)
{
    Entry g(h, true, nullptr, "ndp_tick_reset");
    if (g.rc) return g.rc;
    if (h->slots_busy) { h->err = "ndp_tick_reset: ticks are still in flight (ndp_tick_end them first)"; return -14; }
    int rc = wait_all(h);
    if (rc) return rc;
    if ((rc = launch_list_window(h, h->dX, h->dU, h->stream))) return rc;
    NDP_HIP(h, hipMemsetAsync(h->dAct, 0, act_bytes(h), h->stream));      // reset(): the QPs start from an empty active set
    return g.synced(0);
}

// tick_pre_kernel's arguments.  adv: the list is advanced, its new entry the point at t[b] (device-accessible), or t_all for every vehicle
// when t is null, + T_horizon.  est: the estimator runs on vz[B] (null: column 5 of x_odom[B][10]) and throttle[B] (null: the thrust
// this handle commanded last tick).  pv: the advanced window's position / velocity columns also go there (ndp_xchg_tick_begin).
}  // extern "C"      (tick_pre: C++ linkage, it returns a TickPre)
TickPre tick_pre(const ndp_handle *h, bool adv, const double *t, double t_all, bool est, const double *x_odom, const double *vz,
                 const double *throttle, double *pv)
{
    TickPre a{};
    a.cf = ref_cfg(h, h->cfg.N * h->cfg.dt);
    if (adv) {
        const TrajView tv = traj_view(h);
        a.coeff = tv.coeff; a.tcum = tv.tcum; a.tseg = tv.tseg; a.fpt = tv.fpt; a.seg_hint = tv.hint;
    }
    a.t = t; a.t_all = t_all; a.advance = adv ? 1 : 0;
    a.rg = ring_geom(h);
    a.j_new = h->list_n + (unsigned long long)a.rg.ring();
    a.rx = h->dRingX; a.ru = h->dRingU;
    a.thr = thr_cfg(h); a.st = h->dThr;
    a.vz = vz ? vz : x_odom + 5; a.vz_pitch = vz ? 1 : NX;
    a.throttle = throttle ? throttle : h->dTickThrust;
    a.est = est ? 1 : 0;
    if (pv) { a.pv = pv; a.pv_slot = a.rg.slot(h->list_n + 1); }
    return a;
}
extern "C" {

// the same work inside the one-launch tick (TickArgs), which reads the trajectory's segment cache the last such tick wrote
static TickArgs tick_args(const ndp_handle *h, const TickPre &a)
{
    TickArgs ta{};
    if (a.advance) {
        const TrajView tv = traj_view(h);
        ta.coeff = a.coeff; ta.tcum = a.tcum; ta.tseg = a.tseg; ta.fpt = a.fpt; ta.n_seg = a.cf.n_seg;
        ta.segc = tv.segc[h->segc_par]; ta.segc_wr = tv.segc[h->segc_par ^ 1];
    }
    ta.t = a.t; ta.t_all = a.t_all; ta.advance = a.advance;
    ta.toff = a.cf.toff; ta.mass = a.cf.mass; ta.g = a.cf.g;
    ta.j_new = a.j_new; ta.new_slot = a.rg.slot(a.j_new);
    ta.rg = a.rg; ta.rx = a.rx; ta.ru = a.ru;
    ta.thr = a.thr; ta.st = a.st;
    ta.vz = a.vz; ta.vz_pitch = a.vz_pitch; ta.throttle = a.throttle;
    ta.est = a.est;
    return ta;
}

// One tick's launches on `s`.  Every pointer is device-accessible (HBM or page-locked host memory): x_odom[B][10]; t[B] or null (the
// list is not advanced: hover at a fixed point, or a vehicle between two trajectories); vz[B] or null (column 5 of x_odom);
// throttle[B] or null (the thrust this handle commanded last tick); cmd[B][4]; u0_copy[B][4] or null.
// adv: the list is advanced; its times are t[B] (device-accessible), or t_all for every vehicle when t is null.
static int tick_enqueue(ndp_handle *h, hipStream_t s, const double *x_odom, bool adv, const double *t, double t_all, const double *vz,
                        const double *throttle, int flags, double *cmd, double *u0_copy, StepOut so)
{
    int rc = ensure_tick(h);
    if (rc) return rc;
    if (!h->dRingX) { h->err = "ndp_tick: no reference list (ndp_ref_list_fix_pt, or ndp_ref_set_trajectory + ndp_ref_list_reset, first)"; return -11; }
    if (adv && !h->dTraj) { h->err = "ndp_tick: a trajectory time was given but ndp_ref_set_trajectory was never called"; return -11; }
    if (h->tick_remote) { h->err = "ndp_tick: neighbours come from an exchange buffer (ndp_tick_config_remote): a tick is ndp_tick_advance_device, the exchange, ndp_tick_step_device"; return -17; }
    const int B = h->cfg.batch;
    const RingGeom rg = ring_geom(h);
    const bool est = (flags & TICK_ESTIMATE) != 0;
    // ONE launch per tick (rti_kernel<..., TICK>: list advance and estimator inside the control step's waves) for the reference
    // configuration's compile-time kernels; any other shape: tick_pre_kernel in front of the control step.  NDP_TICK_FORM=pre forces
    // the two-launch form (A/B measurements).
    static const bool force_pre = [] { const char *e = getenv("NDP_TICK_FORM"); return e && !strcmp(e, "pre"); }();
    // (a neighbour's window node N is made INSIDE the one-launch kernel's fused downwash: without the fused form -- can_fuse -- the
    // two-launch form serves)
    const bool one_launch = !force_pre && h->cfg.N == 20 && h->cfg.n_rti == 1 && h->waves == 4 && h->cfg.qp_precision == 0 &&
                            (!h->dTickIndex || can_fuse(h));
    // the list position and the cache's copies move on only when the tick's launches have been accepted (below)
    const unsigned long long n_after = h->list_n + (adv ? 1ull : 0ull);
    TickArgs ta;
    if (adv || est) {
        const TickPre a = tick_pre(h, adv, t, t_all, est, x_odom, vz, throttle);
        if (one_launch) {
            ta = tick_args(h, a);
            so.tick = &ta;
        } else {
            launch_tick_pre(a, s);
            NDP_HIP(h, hipGetLastError());
        }
    }
    const size_t slot = rg.slot(n_after);
    Neigh nb;
    if (h->dTickIndex) {
        nb.other = h->dRingX + slot * 10; nb.stride = NX; nb.index = h->dTickIndex; nb.pitch = rg.px();
        if (h->tick_gate) { nb.ego_xy = x_odom; nb.ego_pitch = NX; }
    }
    so.xr_pitch = rg.px(); so.ur_pitch = rg.pu();
    // nmpc_u_2_att_tgt is the control step's own last store (RtiIo::cmd): no third launch.  k_throttle = row 1 of the estimator's state
    // (k_throttle_init until the estimator has run)
    so.cmd = cmd; so.kthr = h->dThr + (size_t)B; so.thrust_keep = h->dTickThrust;
    rc = enqueue_step(h, x_odom, h->dRingX + slot * 10, h->dRingU + slot * 4, nullptr, nb, u0_copy ? u0_copy : h->su0, nullptr, s, &so);
    if (rc) return rc;               // (refused: the list stays where it was -- an entry the pre-launch may have written lies beyond every window)
    h->list_n = n_after;
    if (adv && so.tick) h->segc_par ^= 1;
    return 0;
}

int ndp_tick_advance_device(ndp_handle *h, const void *d_x_odom, const void *d_t, const void *d_vz, const void *d_throttle, int flags, void *stream)
{
    Entry g(h, d_x_odom, stream, "ndp_tick_advance_device");
    if (g.rc) return g.rc;
    int rc = ensure_tick(h);
    if (rc) return rc;
    if (!h->dRingX) { h->err = "ndp_tick_advance: no reference list (ndp_ref_list_fix_pt, or ndp_ref_set_trajectory + ndp_ref_list_reset, first)"; return -11; }
    const bool adv = d_t != nullptr, est = (flags & TICK_ESTIMATE) != 0, uni = adv && (flags & TICK_T_UNIFORM);
    if (adv && !h->dTraj) { h->err = "ndp_tick_advance: a trajectory time was given but ndp_ref_set_trajectory was never called"; return -11; }
    if (adv || est) {
        const TickPre a = tick_pre(h, adv, uni ? nullptr : (const double *)d_t, uni ? *(const double *)d_t : 0.0, est, (const double *)d_x_odom,
                                   (const double *)d_vz, (const double *)d_throttle);
        launch_tick_pre(a, g.s);
        NDP_HIP(h, hipGetLastError());
        if (adv) ++h->list_n;
    }
    return g.noted(0);
}

int ndp_tick_window_pv_device(ndp_handle *h, void *d_pv, void *stream)
{
    Entry g(h, d_pv, stream, "ndp_tick_window_pv_device");
    if (g.rc) return g.rc;
    if (!h->dRingX) { h->err = "ndp_tick_window_pv: no reference list"; return -11; }
    const RingGeom rg = ring_geom(h);
    launch_pack_pv_list(h->dRingX + rg.slot(h->list_n) * 10, rg.px(), h->cfg.N + 1, (double *)d_pv, h->cfg.batch, g.s);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

// stage 3 on `s` (h->mu held): the control step of the window at list position `pos`, neighbour rows out of `windows`
int tick_step_enqueue(ndp_handle *h, hipStream_t s, const double *x_odom, double *cmd, double *u0, const double *windows, unsigned long long pos)
{
    if (!h->tick_remote) { h->err = "ndp_tick_step: ndp_tick_config_remote first (neighbours in the same handle: ndp_tick_device)"; return -17; }
    if (!h->dRingX) { h->err = "ndp_tick_step: no reference list"; return -11; }
    const RingGeom rg = ring_geom(h);
    const size_t slot = rg.slot(pos), B = h->cfg.batch;
    Neigh nb;
    nb.other = windows; nb.stride = h->tick_remote_stride; nb.index = h->dTickIndex;
    if (h->tick_gate) { nb.ego_xy = x_odom; nb.ego_pitch = NX; }
    StepOut so;
    so.xr_pitch = rg.px(); so.ur_pitch = rg.pu();
    so.cmd = cmd; so.kthr = h->dThr + B; so.thrust_keep = h->dTickThrust;
    return enqueue_step(h, x_odom, h->dRingX + slot * 10, h->dRingU + slot * 4, nullptr, nb, u0 ? u0 : h->su0, nullptr, s, &so);
}

int ndp_tick_step_device(ndp_handle *h, const void *d_x_odom, void *d_cmd, void *d_u0, void *stream)
{
    Entry g(h, d_x_odom && d_cmd, stream, "ndp_tick_step_device");
    if (g.rc) return g.rc;
    return g.noted(tick_step_enqueue(h, g.s, (const double *)d_x_odom, (double *)d_cmd, (double *)d_u0, h->tick_remote, h->list_n));
}

int ndp_tick_device(ndp_handle *h, const void *d_x_odom, const void *d_t, const void *d_vz, const void *d_throttle, int flags,
                    void *d_cmd, void *d_u0, void *stream)
{
    Entry g(h, d_x_odom && d_cmd, stream, "ndp_tick_device");
    if (g.rc) return g.rc;
    const bool uni = d_t && (flags & TICK_T_UNIFORM);       // (then d_t is HOST memory: one double, read here)
    return g.noted(tick_enqueue(h, g.s, (const double *)d_x_odom, d_t != nullptr, uni ? nullptr : (const double *)d_t, uni ? *(const double *)d_t : 0.0,
                                (const double *)d_vz, (const double *)d_throttle, flags, (double *)d_cmd, (double *)d_u0, StepOut()));
}

// host arrays: the inputs of a tick are packed into a slot's page-locked input mirror -- x_odom | t | vz | throttle, 80 + 24 bytes per
// vehicle at most -- which the tick's kernels read over PCIe themselves; cmd | status | iterations (| u0) are written into the
// slot's page-locked output mirror by the kernels (the same two slots, the same zero-copy scheme as ndp_step_begin / _end)
static int tick_begin_locked(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags)
{
    const size_t B = h->cfg.batch;
    int rc = ensure_slots(h);
    if (rc) return rc;
    if (h->slots_busy == 2) { h->err = "ndp_tick_begin: two ticks are already in flight (call ndp_tick_end first)"; return -14; }
    if (h->ev_pending && (rc = wait_all(h))) return rc;
    ndp_handle::HostSlot &sl = h->slot[h->slot_head];
    const auto tp0 = std::chrono::steady_clock::now();
    unsigned char *ib = sl.hIn;
    const size_t o_t = up256(B * NX * 8), o_vz = o_t + up256(B * 8), o_th = o_vz + up256(B * 8);    // (<= in_bytes: the mirror holds a whole step's inputs)
    memcpy(ib, x_odom, B * NX * 8);
    const bool uni = t && (flags & TICK_T_UNIFORM);         // one time for every vehicle: it travels in the kernel arguments
    if (t && !uni) memcpy(ib + o_t, t, B * 8);
    if (vz) memcpy(ib + o_vz, vz, B * 8);
    if (throttle) memcpy(ib + o_th, throttle, B * 8);
    const auto tp1 = std::chrono::steady_clock::now();
    StepOut so;
    so.status = (int *)(sl.hOut + h->off_st); so.iters = (int *)(sl.hOut + h->off_it);
    so.done = sl.evOut;
    const bool want_u0 = (flags & TICK_WANT_U0) != 0;
    rc = tick_enqueue(h, h->stream, (const double *)ib, t != nullptr, t && !uni ? (const double *)(ib + o_t) : nullptr, uni ? t[0] : 0.0,
                      vz ? (const double *)(ib + o_vz) : nullptr,
                      throttle ? (const double *)(ib + o_th) : nullptr, flags, (double *)(sl.hOut + h->off_u0),
                      want_u0 ? (double *)(sl.hOut + h->out_bytes) : nullptr, so);
    if (rc) return rc;
    sl.busy = true; sl.want_iter = false; sl.dump = nullptr;
    h->tslot[h->slot_head].busy = true; h->tslot[h->slot_head].want_u0 = want_u0;
    h->host_us[0] = std::chrono::duration<double, std::micro>(tp1 - tp0).count();
    h->host_us[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tp1).count();
    h->slot_head ^= 1;
    ++h->slots_busy;
    return 0;
}

static int tick_end_locked(ndp_handle *h, double *cmd, double *u0, int32_t *status_out, int32_t *iters_out)
{
    const size_t B = h->cfg.batch;
    if (h->slots_busy == 0 || !h->tslot[h->slot_tail].busy) { h->err = "ndp_tick_end: no tick in flight (ndp_tick_begin first)"; return -14; }
    ndp_handle::HostSlot &sl = h->slot[h->slot_tail];
    if (u0 && !h->tslot[h->slot_tail].want_u0) { h->err = "ndp_tick_end: u0 was not requested at ndp_tick_begin (flags bit 1)"; return -15; }
    const auto tw0 = std::chrono::steady_clock::now();
    hipError_t e = hipErrorNotReady;
    for (int spin = 0; spin < 4000 && e == hipErrorNotReady; ++spin) e = hipEventQuery(sl.evOut);
    if (e == hipErrorNotReady) e = hipEventSynchronize(sl.evOut);
    sl.busy = false;
    h->tslot[h->slot_tail].busy = false;
    h->slot_tail ^= 1;
    --h->slots_busy;
    NDP_HIP(h, e);
    const auto tw1 = std::chrono::steady_clock::now();
    const unsigned char *ho = sl.hOut;
    memcpy(cmd, ho + h->off_u0, B * NU * 8);
    if (u0) memcpy(u0, ho + h->out_bytes, B * NU * 8);
    const int32_t *st = (const int32_t *)(ho + h->off_st);
    if (status_out) memcpy(status_out, st, B * 4);
    if (iters_out) copy_ipm_iters(iters_out, reinterpret_cast<const int32_t *>(ho + h->off_it), B);
    int w = 0;
    for (size_t i = 0; i < B; ++i) w = st[i] > w ? st[i] : w;
    h->host_us[2] = std::chrono::duration<double, std::micro>(tw1 - tw0).count();
    h->host_us[3] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw1).count();
    return w;
}

int ndp_tick_begin(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags)
{
    Entry g(h, x_odom, nullptr, "ndp_tick_begin");
    return g.rc ? g.rc : tick_begin_locked(h, x_odom, t, vz, throttle, flags);
}

int ndp_tick_end(ndp_handle *h, double *cmd, double *u0, int32_t *status_out, int32_t *ipm_iters_out)
{
    Entry g(h, cmd, nullptr, "ndp_tick_end");
    return g.rc ? g.rc : tick_end_locked(h, cmd, u0, status_out, ipm_iters_out);
}

int ndp_tick(ndp_handle *h, const double *x_odom, const double *t, const double *vz, const double *throttle, int flags,
             double *cmd, double *u0, int32_t *status_out, int32_t *ipm_iters_out)
{
    Entry g(h, x_odom && cmd, nullptr, "ndp_tick");      // (begin and end under the one lock)
    if (g.rc) return g.rc;
    if (h->slots_busy) { h->err = "ndp_tick: steps / ticks begun earlier are still in flight (end them first)"; return -14; }
    int rc = tick_begin_locked(h, x_odom, t, vz, throttle, flags | (u0 ? TICK_WANT_U0 : 0));
    if (rc) return rc;
    return tick_end_locked(h, cmd, u0, status_out, ipm_iters_out);
}

}  // extern "C"
