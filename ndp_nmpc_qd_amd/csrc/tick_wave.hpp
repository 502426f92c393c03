// tick_wave.hpp -- the one-launch tick's prologue, inlined by rti_kernel<..., TICK> (rti_kernels.hip): what tick_pre_kernel (tick.hip)
// does, done by the control step's own wave (TickArgs, kern_args.hpp).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kern_args.hpp"
#include "ref_point.hpp"

namespace ndp {

// what tick_new_point works on, all of it requested at the kernel's very top (tick_early): the time, and the lane's share of the
// vehicle's two cached segment records (see tick_early)
typedef double tick_d2 __attribute__((ext_vector_type(2)));
// h0 / h1: (time_cum[i], time_cum[i + 1]), (time_seg[i], i) of slot 0 / 1; ca / cn: the lane's 8 coefficients in slot 0 / 1; tf: (end of the
// trajectory, the lane's component of final_pt)
struct TickEarly { double tv; tick_d2 h0[2], h1[2], ca[4], cn[4], tf; int v; double own, ownc; };   // own / ownc: word `lane` / constant `lane` of the EGO's record (carried over)

// Arguments a kernel needs LATE (the tick's estimator constants, the list's geometry for the new entry's store, the trajectory arrays
// of the rare slow path), fetched where they are used.  Read as ordinary members of `ka` the compiler requests every argument at the
// kernel's top and keeps it in scalar registers until its use: the tick kernels ran out of them (160 spills to / 740 reloads from
// vector-register lanes against 19 / 82 in the plain step -- with one wave per SIMD every one of those is time on the clock).  The
// pointer goes through an empty asm so that the loads cannot move up; they hit the scalar cache (the block was touched at the top).
struct KernargLate {
    const __attribute__((address_space(4))) unsigned *kp;
    __device__ __forceinline__ KernargLate()
    {
        kp = (const __attribute__((address_space(4))) unsigned *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
    }
    template <class T> __device__ __forceinline__ T get(unsigned off) const
    {
        static_assert(sizeof(T) % 4 == 0 && std::is_trivially_copyable<T>::value, "plain words only");
        unsigned w[sizeof(T) / 4];
#pragma unroll
        for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = kp[off / 4 + i];
        T t;
        __builtin_memcpy(&t, w, sizeof(T));
        return t;
    }
};
#define NDP_TA_LATE(L, f) ((L).template get<decltype(TickArgs::f)>((unsigned)(offsetof(KernArgs, ta) + offsetof(TickArgs, f))))
// (A pointer fetched this way has lost what the compiler knows of pointers in the argument block -- that they point to global memory --
// and is dereferenced with FLAT instructions, which also count as LDS operations and turn the waits behind them into full drains:
// fine on the rare paths; the common one goes through gptr.)
template <class T> using gptr = __attribute__((address_space(1))) T *;

// ---- the one-launch tick's prologue (rti_kernel<..., TICK>, see TickArgs), one wave per vehicle
// Lanes 0..13 evaluate the 14 polynomial values of the ego's new point (value c on lane c: the same traj_chain a list kernel calls),
// lanes 16..21 the position / velocity values of the neighbour's (orow >= 0); the values are collected with v_readlane and every lane
// runs the flatness map on them (uniform values: as long as one lane's work).  Lanes 0..13 then store the entry into the list (both
// copies), for the ticks to come.  x_new / u_new / nb_new are the same in every lane.
__device__ __forceinline__ double uniform_lane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// A per-vehicle cache of the trajectory's CURRENT and NEXT segment records, 2 x 32 doubles at segc + SEGC_PER v:
//     [0] time_cum[i]  [1] time_cum[i + 1]  [2] time_seg[i]  [3] i  [4 .. 31] the 28 coefficients of segment i
// and behind them [64 + 2 a], [65 + 2 a] = (time_cum[n_seg], final_pt[a]) for the axes a = 0..2 (one 16-byte load per lane)
// Found through the trajectory arrays a point costs two dependent memory round trips (segment index -> record), ~1 700 cycles
// each and nothing in the wave to hide them under; the cache's address depends on the vehicle only, so its loads are the launch's
// first and arrive under the weight transfer.  A vehicle moves on to its next segment every time_seg / 20 ms ticks (and in a batch
// of a thousand some vehicle does in every tick): that is slot 1, valid from the moment slot 0 was; the wave that crosses re-fills
// both slots -- one load per lane, requested in the prologue, stored behind the MLP phase (tick_cache_store), off everybody's
// critical path.  Anything else (the first tick after ndp_ref_set_trajectory -- the cache starts as NaNs --, a jump in time) takes
// seg_locate and the trajectory arrays, and re-fills the cache the same way.
__device__ __forceinline__ TickEarly tick_early(const TickArgs &ta, int inst, int orow, int lane)
{
    TickEarly te;
    const int c = (lane & 15) < 14 ? (lane & 15) : 13, q = (4 + chain_base(c)) >> 1;
    te.v = ((lane >> 4) & 1) && orow >= 0 ? orow : inst;
    // The load unit takes 16 cycles per instruction and wave of 64 (four lanes a cycle, whatever the width), and the four waves of a
    // compute unit share it: as 35 8-byte loads by all 64 lanes these requests alone kept it busy for 2 200 cycles.  Hence 16-byte
    // loads (13 of them) and only the 24 lanes whose values are looked at (lanes 0..13 ego, 16..21 neighbour).
    const tick_d2 *s0 = reinterpret_cast<const tick_d2 *>(ta.segc + (size_t)te.v * SEGC_PER);
    te.tv = ta.t_all;
    if (lane < 24) {
        te.h0[0] = s0[0]; te.h0[1] = s0[1]; te.h1[0] = s0[SEGC_SLOT / 2]; te.h1[1] = s0[SEGC_SLOT / 2 + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = q + (c >= 12 ? (k & 1) : k);
            te.ca[k] = s0[o]; te.cn[k] = s0[SEGC_SLOT / 2 + o];
        }
        te.tf = s0[SEGC_SLOT + (c < 3 ? c : 0)];
    }
    // the ego's whole record, word `lane` (and constant `lane` in lanes 0..5): carried over into the copy the NEXT tick reads
    te.own = ta.segc[(size_t)inst * SEGC_PER + lane];
    te.ownc = ta.segc[(size_t)inst * SEGC_PER + 2 * SEGC_SLOT + (lane < 6 ? lane : 5)];
    if (lane < 24) {
        // (written as a branch: as a select the compiler picks between two ADDRESSES -- the argument's copy parked in scratch memory
        // for it -- and loads through a flat pointer)
        if (ta.t) te.tv = ta.t[te.v];
    }
    return te;
}

// Consume everything tick_early requested, HERE.  While an LDS-DMA transfer (global_load_lds) is in flight the compiler cannot use the
// in-order load counter: the instruction counts as "may touch memory AND LDS", and from its issue to the next full drain every wait of
// the wave -- for whatever value -- is emitted as s_waitcnt vmcnt(0), i.e. a wait for the whole 72-KB weight transfer.  Left to its
// first use inside tick_new_point the cached records therefore "arrived" only when the transfer was complete (6 400 cycles after
// entry; requested at 1 000) and the polynomial work ran BEHIND the transfer instead of under it.  Waiting for them in front of the
// transfer costs the transfer a later start (the records' own latency) and takes the polynomial work off the critical path.
__device__ __forceinline__ void tick_arrived(TickEarly &te)
{
    asm volatile("" : "+v"(te.tv), "+v"(te.h0[0]), "+v"(te.h0[1]), "+v"(te.h1[0]), "+v"(te.h1[1]), "+v"(te.tf), "+v"(te.own), "+v"(te.ownc));
    asm volatile("" : "+v"(te.ca[0]), "+v"(te.ca[1]), "+v"(te.ca[2]), "+v"(te.ca[3]), "+v"(te.cn[0]), "+v"(te.cn[1]), "+v"(te.cn[2]), "+v"(te.cn[3]));
}

// returns (in every lane) the value lane l must store into the ego's cache word l behind the MLP phase, valid if refill != 0
// store: false in the idle waves of a ragged last workgroup (they shadow the last instance for the barriers' sake and must not write)
__device__ __forceinline__ double tick_new_point(const TickArgs &ta, const TickEarly &te, int inst, int lane, bool store, double xv[10],
                                                 double uv[4], double nbv[6], int &refill, double &cfill, double *stamps)
{
    // profiling hook (ndp_debug_stamps): slots 17.. = the prologue's own timeline; each stamp waits for the value it names
    auto stamp_after = [&](int idx, double dep) {
        if (NDP_RARELY(stamps != nullptr)) {
            unsigned long long tk;
            asm volatile("s_nop 0\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tk) : "v"(dep) : "memory");
            if (lane == 0) stamps[idx] = (double)tk;
        }
    };
    const int c = (lane & 15) < 14 ? (lane & 15) : 13;
    const int v = te.v;
    const int S = ta.n_seg;
    const double lo0 = te.h0[0][0], hi0 = te.h0[0][1], ts0 = te.h0[1][0], i0 = te.h0[1][1];
    const double lo1 = te.h1[0][0], hi1 = te.h1[0][1], ts1 = te.h1[1][0], i1 = te.h1[1][1];
    stamp_after(17, lo0 + te.cn[3][1] + te.tf[1]);                    // the cached records are there
    const double t = te.tv + ta.toff;
    stamp_after(18, t);                                               // the time is there
    bool past = t >= te.tf[0];                                        // base_pt_publisher.py:93-94: hover at final_pt after the end
    // (the same tests as seg_locate's: segment 0 also serves times in front of time_cum[0]; a NaN bound -- the empty cache -- fails all three)
    const bool in0 = (i0 == 0.0 || !(lo0 > t)) && hi0 > t, in1 = !in0 && !(lo1 > t) && hi1 > t;
    const bool slow = lane < 24 && !past && !in0 && !in1;            // (lanes 24..63 hold nothing: tick_early)
    int idx = (int)(in0 ? i0 : i1);
    double tcs = in0 ? lo0 : lo1, tsg = in0 ? ts0 : ts1, fp = te.tf[1];
    // (opaque to the optimiser: left visible as "a loaded value or, on the slow path, another load", it parks the cached values in
    // scratch memory to select between ADDRESSES and load through a flat pointer)
    asm volatile("" : "+v"(tcs), "+v"(tsg), "+v"(fp));
    double ca[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ca[i] = in1 ? te.cn[i >> 1][i & 1] : te.ca[i >> 1][i & 1];
    if (slow) {                                                       // (rare; per lane) through the trajectory arrays
        const KernargLate L;
        const double *tc = NDP_TA_LATE(L, tcum) + (size_t)v * (S + 1);
        const int cb = chain_base(c);
        idx = seg_locate(S, tc, t, -1);
        if (idx < 0) {                                                // (an empty cache does not know where the trajectory ends)
            past = true;
            idx = S - 1;
            fp = NDP_TA_LATE(L, fpt)[(size_t)v * 3 + (c < 3 ? c : 0)];
        } else {
            tcs = tc[idx]; tsg = NDP_TA_LATE(L, tseg)[(size_t)v * S + idx];
            const double *r = NDP_TA_LATE(L, coeff) + ((size_t)v * S + idx) * 28 + cb;
#pragma unroll
            for (int i = 0; i < 8; ++i) ca[i] = r[c >= 12 ? (i & 3) : i];
        }
    }
    double val = 0.0;
    if (past) {
        if (c < 3) val = fp;
    } else {
        const double its = rcp_n(tsg);
        double s;
        {
#pragma clang fp contract(off)
            s = (t - tcs) * its;
        }
        val = traj_chain(ca, c, s, its);
    }
    // the ego's cache: re-filled by this wave when its point did not come out of slot 0 (lane 0 belongs to the ego's group)
    refill = __builtin_amdgcn_readlane((in1 || slow) ? 1 : 0, 0);
    double fill = 0.0;
    cfill = te.ownc;
    if (refill) {
        const int ie = __builtin_amdgcn_readlane(idx, 0);
        const int sl = lane >> 5, f = lane & 31, i = ie + sl < S ? ie + sl : S - 1;
        const KernargLate L;
        const double *tce = NDP_TA_LATE(L, tcum) + (size_t)inst * (S + 1), *fpt = NDP_TA_LATE(L, fpt);
        cfill = lane < 6 ? ((lane & 1) ? fpt[(size_t)inst * 3 + (lane >> 1)] : tce[S]) : 0.0;   // (constants of the trajectory; stored by tick_cache_store)
        fill = f == 0 ? tce[i] : (f == 1 ? tce[i + 1] : (f == 2 ? NDP_TA_LATE(L, tseg)[(size_t)inst * S + i] : (f == 3 ? (double)i
                 : NDP_TA_LATE(L, coeff)[((size_t)inst * S + i) * 28 + (f - 4)])));
        if (ie + sl >= S && f == 1) fill = -1.0e300;                  // no segment behind the last one: slot 1 never matches (hi <= any t)
    }
    stamp_after(19, val);                                             // the lane's polynomial value
    double pvaj[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) pvaj[i] = uniform_lane(val, i);
    const double yaw = uniform_lane(val, 12), yawd = uniform_lane(val, 13);
#pragma unroll
    for (int i = 0; i < 6; ++i) nbv[i] = uniform_lane(val, 16 + i);
    stamp_after(20, pvaj[11] + nbv[5] + yawd);                        // collected over the lanes
    // where the entry goes (lane l: element l of x | u): the list's geometry is a late argument, requested HERE so that its fetch passes
    // under the flatness map instead of standing between the map and the barrier (-390 cycles per tick)
    gptr<double> dst;
    size_t mirror;
    {
        const KernargLate L;
        const size_t sl = NDP_TA_LATE(L, new_slot);
        const RingGeom rg = NDP_TA_LATE(L, rg);
        dst = (gptr<double>)(lane < 10 ? NDP_TA_LATE(L, rx) + (size_t)inst * rg.px() + sl * 10 + lane
                                       : NDP_TA_LATE(L, ru) + (size_t)inst * rg.pu() + sl * 4 + (lane - 10));
        mirror = (size_t)rg.np1 * (lane < 10 ? 10 : 4);
    }
    flatness_xu(ta.mass, ta.g, pvaj, yaw, yawd, xv, uv);
    stamp_after(21, xv[9] + uv[0]);                                   // flatness map done
    // the entry, for the windows of the ticks to come: element l of x | u from lane l
    // (v_writelane of the uniform values: written as a chain of selects on the lane id the compiler builds a table in scratch memory)
    int elo = 0, ehi = 0;
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        const double w = i < 10 ? xv[i] : uv[i - 10];
        const int wl = __builtin_amdgcn_readfirstlane(__double2loint(w)), wh = __builtin_amdgcn_readfirstlane(__double2hiint(w));
        asm("v_writelane_b32 %0, %1, %2" : "+v"(elo) : "s"(wl), "n"(i));
        asm("v_writelane_b32 %0, %1, %2" : "+v"(ehi) : "s"(wh), "n"(i));
    }
    const double e = __hiloint2double(ehi, elo);
    if (store && lane < 14) {
        dst[0] = e;
        dst[mirror] = e;
    }
    return fill;
}

// The cache has two copies.  A launch READS one (its own record and its neighbour's, at entry) and WRITES the other -- every vehicle's
// record, every advancing tick: re-filled when the vehicle crossed into its next segment, carried over otherwise -- and the host swaps
// them between ticks.  (With one copy written in place, the neighbour's wave -- another workgroup, possibly another XCD, possibly a later
// round of a batch larger than the device -- could read a record while its owner re-filled it in the same launch: old header, new
// coefficients.  Nothing orders two workgroups of one launch; a kernel boundary orders everything.)
__device__ __forceinline__ void tick_cache_store(const TickArgs &ta, const TickEarly &te, int inst, int lane, int refill, double fill, double cfill)
{
    ta.segc_wr[(size_t)inst * SEGC_PER + lane] = refill ? fill : te.own;
    if (lane < 6) ta.segc_wr[(size_t)inst * SEGC_PER + 2 * SEGC_SLOT + lane] = cfill;
}

// hover_throttle_callback (nmpc_node.py:251-253) of this vehicle, by lane 0; returns k_throttle to every lane
__device__ __forceinline__ double tick_estimator(const TickArgs &ta, int inst, int B, int lane)
{
    double k = 0.0;
    const KernargLate L;
    if (lane == 0) k = throttle_update_one(NDP_TA_LATE(L, thr), NDP_TA_LATE(L, st), (size_t)B, inst, NDP_TA_LATE(L, vz)[(size_t)inst * NDP_TA_LATE(L, vz_pitch)],
                                           NDP_TA_LATE(L, throttle)[inst]);
    return uniform_lane(k, 0);
}

}  // namespace ndp
