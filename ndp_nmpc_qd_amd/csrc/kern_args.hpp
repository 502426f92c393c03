// kern_args.hpp -- argument blocks of the rows and the tick that more than one translation unit uses (the host fills them, the kernels
// read them).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace ndp {

struct ThrCfg { double a1, a2, hm, g, R, Q0, Q1, mass; };

// layout of the reference list in HBM (see the f1 list kernels below)
struct RingGeom {
    int step, np1;                 // list entries per node spacing; N + 1
    __host__ __device__ int ring() const { return step * (np1 - 1) + 1; }
    __host__ __device__ size_t px() const { return (size_t)step * 2 * np1 * 10; }     // doubles per vehicle, x ring
    __host__ __device__ size_t pu() const { return (size_t)step * 2 * np1 * 4; }
    __host__ __device__ size_t slot(unsigned long long j) const { return (size_t)(j % step) * 2 * np1 + (size_t)((j / step) % np1); }
};

struct RefCfg { int B, N, n_seg; double dt, mass, g, toff; };   // toff: added to every vehicle's node-0 time (rollouts)

struct TickPre {
    RefCfg cf;
    const double *coeff, *tcum, *tseg, *fpt;
    int *seg_hint;                     // [B] the segment each vehicle's last point lay in (ref_point)
    const double *t;                   // [B] trajectory time of the tick, or null: t_all for every vehicle
    double t_all;
    int advance;                       // 0: the list is not advanced
    unsigned long long j_new;          // absolute index of the entry the new point becomes
    RingGeom rg;
    double *rx, *ru;
    ThrCfg thr;
    double *st;                        // estimator state, SoA [8][B]
    const double *vz;                  // vz of vehicle b at vz[b * vz_pitch]: a [B] array (pitch 1) or column 5 of the odometry rows (pitch 10)
    size_t vz_pitch;
    const double *throttle;            // [B]: the thrust command sent last tick (caller's array, or the one the control step kept)
    int est;                           // run the estimator this tick
    // ndp_xchg_tick_begin: the advanced window's position / velocity columns -> pv[b][N+1][6] in the same launch (one launch less on a
    // path that is bound by the host's launches); the window starts at list slot pv_slot, its node N is the point made here
    double *pv = nullptr;
    size_t pv_slot = 0;
};

}  // namespace ndp
