// ndp_hip.hip -- the handle's runtime and the control step's host side behind the C-ABI of include/ndp_nmpc.h: the pack threads, ndp_create /
// destroy and the getters, every step form (enqueue_step -> launch_rti -> rti_pick), the host-array step, timing, the sensitivity
// buffers, the adjoint / forward-mode entry points, ndp_set_model and the debug entry points.  The kernels live with the host code that
// launches them (host.hpp: which unit owns what); here: the work list's reset launch.
// The iterate (X, U) of a handle lives in HBM and stays there between steps; host-array steps (ndp_step / ndp_step_begin)
// read their inputs from, and mirror their outputs to, page-locked host slots over PCIe (zero-copy) -- see step_begin_locked.
// There is no CPU fallback: every entry point fails (<0) if HIP is unusable.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <sched.h>
#include <stdio.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "host.hpp"
#include "cond_qp.hpp"
#include "mlp_tile.hpp"      // FR_TOTAL

namespace ndp {

// behind the work list's consumer launch: the list is empty again for the next step's producer
__global__ void queue_reset_kernel(unsigned *count, unsigned long long *ipm_total)
{
    if (threadIdx.x == 0) {
        *ipm_total += *count;
        *count = 0u;
    }
}

}  // namespace ndp

// ------------------------------------------------------------------------------------------ C-ABI
using namespace ndp;

// ---- host pack threads.  A host-array step first moves the caller's (pageable) arrays into a page-locked mirror the kernel can
// read; at batch 1024 that is 4.2 MB per step -- 56 us for one core, 26-30 us for eight (measured), against ~100 us for the
// kernel that then pulls them over PCIe.  The mirror is filled by a few persistent threads and the caller, a chunk
// (<= PACK_CHUNK bytes) at a time.
// len bytes as they lie, or -- rows > 0 -- `rows` rows of `len` bytes each taken from rows src_stride bytes apart (the neighbour
// windows: the 6 position / velocity columns of every 10-column row, all the gate and the network read)
struct PackJob { unsigned char *dst; const unsigned char *src; size_t len; size_t rows = 0, src_stride = 0; };
enum : size_t { PACK_CHUNK = (size_t)256 << 10 };
struct PackPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<const PackJob *> jobs{nullptr};
    std::atomic<int> njobs{0}, next{0}, active{0};
    std::unique_ptr<std::atomic<int>[]> done;
    int done_cap = 0;
    uint64_t gen = 0;
    std::atomic<uint64_t> gen_pub{0};   // gen, readable without the lock (the workers' polling phase)
    bool stop = false;
    static void cpu_relax()
    {
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
        __asm__ __volatile__("pause");
#endif
    }

    explicit PackPool(int n)
    {
        for (int i = 0; i < n; ++i) th.emplace_back([this] { work(); });
    }
    ~PackPool()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
    bool take_one()
    {   // njobs is published last (release) and read first (acquire): a thread that sees a job count sees that list and its flags
        const int n = njobs.load(std::memory_order_acquire);
        if (n == 0) return false;
        const int i = next.fetch_add(1, std::memory_order_acq_rel);
        if (i >= n) return false;
        const PackJob &j = jobs.load(std::memory_order_relaxed)[i];
        if (j.rows == 0) memcpy(j.dst, j.src, j.len);
        else
            for (size_t r = 0; r < j.rows; ++r) memcpy(j.dst + r * j.len, j.src + r * j.src_stride, j.len);
        done[i].store(1, std::memory_order_release);
        return true;
    }
    void drain() { while (take_one()) {} }
    void work()
    {
        uint64_t seen = 0;
        for (;;) {
            // back-to-back steps: the next job list arrives within microseconds -- poll for it a short while (a futex wake-up
            // costs 30-60 us per thread) before going to sleep on the condition variable (a 50 Hz control loop sleeps)
            for (int spin = 0; spin < 20000 && gen_pub.load(std::memory_order_acquire) == seen; ++spin) cpu_relax();
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                active.fetch_add(1, std::memory_order_acq_rel);   // under the lock: post() cannot miss a worker that saw this generation
            }
            drain();
            active.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    // hands the job list to the workers; the caller then consumes done[i] in order (wait_job) and must call finish()
    void post(const PackJob *j, int n)
    {
        if (n > done_cap) { done.reset(new std::atomic<int>[n]); done_cap = n; }
        for (int i = 0; i < n; ++i) done[i].store(0, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(mu);
            jobs.store(j, std::memory_order_relaxed);
            next.store(0, std::memory_order_relaxed);
            njobs.store(n, std::memory_order_release);
            ++gen;
            gen_pub.store(gen, std::memory_order_release);
        }
        if (!th.empty() && n > 1) cv.notify_all();
    }
    bool is_done(int i) const { return done[i].load(std::memory_order_acquire) != 0; }
    void wait_job(int i)
    {
        // the caller packs as well while it has nothing to hand to the DMA engine (and does everything when there are no threads)
        while (!is_done(i))
            if (!take_one()) std::this_thread::yield();
    }
    void finish()
    {   // the job list lives on the caller's stack: no worker may still be looking at it when the caller returns
        njobs.store(0, std::memory_order_release);
        while (active.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    }
};

static thread_local std::string g_create_err;

// host cores this process may really use: the affinity mask, cut down to the cgroup's CPU quota (cpu.max: "<quota> <period>" or "max ...")
static int usable_cores()
{
    int n = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int a = CPU_COUNT(&set); if (a > 0 && a < n) n = a; }
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        double period = 0.0;
        if (fscanf(f, "%31s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0.0) {
            const int c = (int)(atof(q) / period);
            if (c >= 1 && c < n) n = c;
        }
        fclose(f);
    }
    return n < 1 ? 1 : n;
}

// entry points that do not run the control step through rti_sens_kernel: refused on a handle with sensitivities on
int sens_refuse(ndp_handle *h, const char *what)
{
    h->err = std::string(what) + ": not available while initial-state sensitivities are enabled (ndp_sens_enable(h, 0) first): "
             "only the in-place and work-list step forms compute them";
    return -2;
}

extern "C" {

int ndp_abi_version(void) { return NDP_ABI_VERSION; }
size_t ndp_cfg_size(void) { return sizeof(ndp_cfg); }

int ndp_default_cfg(ndp_cfg *cfg)
{
    if (!cfg) return -1;
    fill_default_cfg(cfg);
    return 0;
}

const char *ndp_last_error(const ndp_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int ndp_debug_lds_doubles(int N) { return lds_doubles(N) + DBG_EXTRA; }

int ndp_debug_lds_layout(int N, int *out8)
{
    if (!out8) return -1;
    lds_layout(N, out8);
    return 0;
}

int ndp_destroy(ndp_handle *h)
{
    if (!h) return -1;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ev_pending) (void)hipEventSynchronize(h->evLast);
    if (h->aux) (void)hipStreamSynchronize(h->aux);
    h->pool.reset();                        // the pack threads stop before the page-locked mirrors go
    if (h->hIpm) (void)hipDeviceSynchronize();      // (a copy into it may still be queued on a caller's stream)
    delete h;                               // every member releases what it owns (hip_own.hpp), the streams last
    return 0;
}

long long ndp_debug_live_resources(void) { return live_resources.load(std::memory_order_relaxed); }

// a pin is the weight as_gamma on its input: far below the input weights it holds nothing, yet as_check still writes the input onto
// its bound -- a wrong step with status 0 (NDP_AS_GAMMA_FLOOR in the header).  ndp_create's rule, and ndp_set_model's for a new Rd.
static bool as_gamma_holds(const ndp_cfg &c, const double *Rd)
{
    if (c.as_iter_max <= 0) return true;
    double rd = 0.0;
    for (int i = 0; i < 4; ++i) rd = std::max(rd, std::fabs(c.dt * Rd[i]));
    return std::isfinite(c.as_gamma) && c.as_gamma >= NDP_AS_GAMMA_FLOOR * rd;
}

int ndp_create(const ndp_cfg *cfg, ndp_handle **out)
{
    if (!cfg || !out) { g_create_err = "ndp_create: null argument"; return -1; }
    *out = nullptr;
    if (cfg->batch < 1 || cfg->N < 2 || slots_for(cfg->N) > 5 || cfg->n_rti < 1 || cfg->qp_precision < 0 || cfg->qp_precision > 6 ||
        cfg->work_queue < 0 || cfg->work_queue > 2 || !(cfg->ts_nmpc > 0.0) || cfg->dt < cfg->ts_nmpc) {
        g_create_err = "ndp_create: need batch >= 1, 2 <= N <= 46, n_rti >= 1, qp_precision in 0..6, work_queue in 0..2, 0 < ts_nmpc <= dt";
        return -2;
    }
    if (cfg->qp_precision >= 5 && (cfg->N % 4 != 0 || cfg->N > 40)) {
        g_create_err = "ndp_create: the condensed study (qp_precision 5 / 6) tiles the 4N x 4N Hessian by 16: N must be a multiple of 4, at most 40";
        return -2;
    }
    if (!as_gamma_holds(*cfg, cfg->Rd)) {
        g_create_err = "ndp_create: as_gamma must be finite and at least 1e8 * max(dt * Rd) when as_iter_max > 0 (a weaker pin does not hold "
                       "its input on the bound)";
        return -2;
    }
    if (cfg->ipm_refine > 0 && (slots_for(cfg->N) > 3 || cfg->qp_precision != 0)) {
        // (rounds 4-5 accepted the setting and ignored it -- a getter nobody called said so)
        g_create_err = "ndp_create: ipm_refine > 0 is not served for this shape: the refinement path (stiff sweeps + second solves while a STATE bound's "
                       "barrier term exceeds refine_gamma) lives in the three-slot fp64 kernels only (N <= 27, qp_precision 0); the five-slot kernels "
                       "(N >= 28) sit at the register limit without it.  Set ipm_refine = 0: strongly active state bounds at a tight tolerance then "
                       "end in status 4 (never a silent answer)";
        return -2;
    }
    {   // the reference list holds one point per control period and the window is every (dt / ts_nmpc)-th entry
        // (params/nmpc_params.py:40-43): the ratio has to be a whole number, else ring windows and direct windows disagree
        const double ratio = cfg->dt / cfg->ts_nmpc, nearest = (double)(long long)(ratio + 0.5);
        if (ratio - nearest > 1e-9 || nearest - ratio > 1e-9) {
            g_create_err = "ndp_create: dt must be a whole multiple of ts_nmpc (node spacing = every k-th entry of the reference list)";
            return -2;
        }
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= cfg->device) {
        g_create_err = std::string("ndp_create: no usable HIP device (") + hipGetErrorString(e) + ")";
        return -3;
    }
    ndp_handle *h = new (std::nothrow) ndp_handle;
    if (!h) return -4;
    h->cfg = *cfg;
    h->P = to_params(*cfg);
    h->list_step = (int)(cfg->dt / cfg->ts_nmpc + 0.5);      // params/nmpc_params.py:40-43: every 5th list entry is a node
    h->lds_per_wave = (lds_doubles(cfg->N) + 1) & ~1;   // keep 16-byte alignment per wave slice
    if (cfg->qp_precision >= 5) h->lds_per_wave += (cond_extra_doubles(cfg->N) + 1) & ~1;   // (the condensed study works behind the slice: one wave per workgroup)
    const size_t per_wave_bytes = (size_t)h->lds_per_wave * sizeof(double);
    h->waves = 4;
    while (h->waves > 1 && per_wave_bytes * h->waves > 160 * 1024) h->waves >>= 1;
    if (const char *e = getenv("NDP_DEV_WAVES")) {      // measurement switch: instances per workgroup (2: two workgroups per CU)
        const int w = atoi(e);
        if ((w == 1 || w == 2 || w == 4) && w <= h->waves) h->waves = w;
    }
    auto fail = [&](const char *what, hipError_t err) {
        g_create_err = std::string("ndp_create: ") + what + ": " + hipGetErrorString(err);
        ndp_destroy(h);
        return -5;
    };
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return fail("hipSetDevice", e);
    {
        hipDeviceProp_t prop;
        if ((e = hipGetDeviceProperties(&prop, cfg->device)) != hipSuccess) return fail("hipGetDeviceProperties", e);
        h->n_simd = 4 * prop.multiProcessorCount;
    }
    // work list: with one instance per SIMD nothing can be re-balanced; with two or more it is switched by what the steps do
    // (queue_policy) -- callers who know their workload set cfg.work_queue = 1 / 2.
    // The N = 40 / 2-iteration shape always takes the list: its producer kernel carries no interior-point code and does not
    // spill, which is worth 17 % even when nothing is listed (the in-place kernel of that shape uses 0.9 KB of scratch per lane)
    if (cfg->work_queue == 1 && !(queue_shape(h) && cfg->qp_mode == NDP_QP_AUTO)) {
        g_create_err = "ndp_create: work_queue = 1 needs qp_mode AUTO, qp_precision 0 and (N, n_rti) = (20, 1) or (40, 2)";
        delete h;
        return -2;
    }
    // reference shape, two or more instances per SIMD, cfg.work_queue = 0: in place to begin with, the list when the steps ask for it
    // (queue_policy)
    h->queue_auto = cfg->work_queue == 0 && queue_shape(h) && cfg->qp_mode == NDP_QP_AUTO && cfg->N == 20 && cfg->batch >= 2 * h->n_simd;
    h->use_queue = cfg->work_queue == 1 || (cfg->work_queue == 0 && queue_shape(h) && cfg->qp_mode == NDP_QP_AUTO && cfg->N == 40);
    if (h->queue_auto) {
        if ((e = h->hIpm.alloc(64)) != hipSuccess) return fail("hipHostMalloc (work-list counter)", e);
        h->hIpm[0] = h->hIpm[1] = 0;
    }
    if ((e = h->stream.ensure(hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = h->evLast.ensure(hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    const size_t B = cfg->batch;
    {   // input / output blocks
        size_t o = 0;
        h->off_x0 = o; o += up256(B * NX * 8);
        h->off_xr = o; o += up256(nxs(h) * 8);
        h->off_ur = o; o += up256(nus(h) * 8);
        h->off_f = o; o += up256(nfs(h) * 8);        // (fp32 forces, or fp64 ones: ndp_step_ex_f64)
        h->off_other = o; o += up256(nxs(h) * 8);
        h->off_ego = o; o += up256(B * 2 * 8);
        h->in_bytes = o;
        o = 0;
        h->off_u0 = o; o += up256(B * NU * 8);
        h->off_st = o; o += up256(B * 4);
        h->off_it = o; o += up256(B * 4);
        h->out_bytes = o;
        // the persistent iterate lives right behind the small outputs: u0 | status | iterations | X | U come back to the host
        // in ONE copy when a caller asks for the iterate as well (ndp_step_ex).  All of it is HBM; the page-locked host
        // mirrors of the host-array entry points are allocated by their first call (ensure_slots).
        h->out_all = h->out_bytes + (nxs(h) + nus(h)) * 8;
    }
    std::string what;
    auto dev = [&](auto &buf, size_t bytes, const char *name) {
        if ((e = buf.alloc(bytes)) != hipSuccess) what = std::string("hipMalloc ") + name;
        return e == hipSuccess;
    };
    if (!dev(h->dForce, nfs(h) * 4, "dForce") || !dev(h->dFrag, FR_TOTAL * 4, "dFrag") || !dev(h->dFragT, FRT_TOTAL * 4, "dFragT") ||
        !dev(h->dGwPart, (size_t)mlp_vjp_groups(h) * NDP_MLP_NPARAM * 4, "dGwPart") || !dev(h->dKC, KC_HOST * 8, "dKC") ||
        !dev(h->dThr, B * 8 * 8, "dThr") || !dev(h->sThr, B * 11 * 8, "sThr") || !dev(h->dRelay, B * 4 * 8, "dRelay") ||
        !dev(h->dQctr, 256, "dQctr") || !dev(h->dQids, B * 4, "dQids") || !dev(h->dAct, act_bytes(h), "dAct") ||
        !dev(h->dTrain, TRAIN_WS_BYTES, "dTrain") ||
        !dev(h->dFitPart, FIT_WS_BYTES, "dFitPart") ||      // (every entry a call reads is written by that call: no memset)
        !dev(h->dTables, TB_WORDS * 4, "dTables") || !dev(h->dIn, h->in_bytes, "dIn") || !dev(h->dOut, h->out_all, "dOut") ||
        !dev(h->sdbg, (size_t)(lds_doubles(cfg->N) + DBG_EXTRA) * 8, "sdbg"))
        return fail(what.c_str(), e);
    // the views into dIn / dOut
    h->dX = (double *)(h->dOut + h->out_bytes); h->dU = h->dX + nxs(h);
    h->sx0 = (double *)(h->dIn + h->off_x0); h->sxr = (double *)(h->dIn + h->off_xr); h->sur = (double *)(h->dIn + h->off_ur);
    h->sf = (float *)(h->dIn + h->off_f); h->sother = (double *)(h->dIn + h->off_other); h->sego = (double *)(h->dIn + h->off_ego);
    h->su0 = (double *)(h->dOut + h->off_u0); h->dStatus = (int *)(h->dOut + h->off_st); h->dIters = (int *)(h->dOut + h->off_it);
    h->lastStatus = h->dStatus; h->lastIters = h->dIters;
    (void)hipMemsetAsync(h->dAct, 0, act_bytes(h), h->stream);
    (void)hipMemsetAsync(h->dRelay, 0, B * 4 * 8, h->stream);
    (void)hipMemsetAsync(h->dQctr, 0, 256, h->stream);
    (void)hipMemsetAsync(h->dTrain, 0, 64, h->stream);
    {
        double kc[KC_HOST];
        fill_kc(h->P, kc);
        if ((e = hipMemcpyAsync(h->dKC, kc, sizeof(kc), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail("hipMemcpy kc", e);
        std::vector<int> tb(TB_WORDS);
        fill_tables(cfg->N, tb.data(), (cfg->qp_precision == 3 || cfg->qp_precision == 4) ? 1 : 0);   // the fp32 / bf16 sweeps keep a different column per lane
        if ((e = hipMemcpyAsync(h->dTables, tb.data(), TB_WORDS * 4, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return fail("hipMemcpy tables", e);
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail("hipStreamSynchronize", e);
    }
    (void)hipMemsetAsync(h->dX, 0, nxs(h) * 8, h->stream);
    (void)hipMemsetAsync(h->dU, 0, nus(h) * 8, h->stream);
    (void)hipMemsetAsync(h->dOut, 0, h->out_bytes, h->stream);
    (void)hipMemsetAsync(h->dForce, 0, nfs(h) * 4, h->stream);
    // allow the big dynamic-LDS launches
    const int lds_bytes = (int)(per_wave_bytes * h->waves);
    if ((e = mlp_prepare()) != hipSuccess) return fail("hipFuncSetAttribute(mlp_kernel)", e);
    if ((e = mlp_vjp_prepare()) != hipSuccess) return fail("hipFuncSetAttribute(mlp_vjp_kernel)", e);
    if ((e = mlp_fit_prepare()) != hipSuccess) return fail("hipFuncSetAttribute(mlp_fit_rows_kernel)", e);
    if ((e = mlp_multi_prepare()) != hipSuccess) return fail("hipFuncSetAttribute(mlp_multi_kernel)", e);
    if ((e = plant_force_deriv_prepare()) != hipSuccess) return fail("hipFuncSetAttribute(plant_force_vjp_kernel)", e);
    const char *attr = nullptr;
    if ((e = rti_set_lds(false, lds_bytes, &attr)) != hipSuccess) return fail(attr, e);      // (the sensitivity kernels: ndp_sens_enable)
    launch_throttle_reset(h);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail("hipStreamSynchronize", e);
    *out = h;
    return 0;
}

// ---- enqueue helpers (no locking, no sync) ----
// defer: the caller may hand the pair to the launch itself (hipExtLaunchKernel's start / stop events: the dispatch packet's own
// timestamps, no event packets around the kernel -- an event pair recorded around a launch adds ~2.5 us of dispatch gap to what it
// measures); it records ev.a itself if it cannot.
int begin_timing(ndp_handle *h, hipStream_t s, int kind, bool defer)
{
    h->timing_open = false;
    if (!h->timing || (h->launch_no[kind]++ % h->timing) != 0) return 0;
    h->timing_open = true;
    ndp_handle::Ev ev; ev.kind = kind;
    NDP_HIP(h, ev.a.ensure(hipEventDefault)); NDP_HIP(h, ev.b.ensure(hipEventDefault));
    if (!defer) NDP_HIP(h, hipEventRecord(ev.a, s));
    h->events.push_back(std::move(ev));
    return 0;
}
int end_timing(ndp_handle *h, hipStream_t s)
{
    if (!h->timing_open) return 0;
    NDP_HIP(h, hipEventRecord(h->events.back().b, s));
    return 0;
}

// A *_device call enqueued on a caller's stream: remember it so that the getters (ndp_get_status, ndp_get_iterate, ...)
// wait for that work and not only for the library's own stream.  Streams being captured into a graph are skipped (an
// event recorded there belongs to the graph and cannot be waited on from the host).
int note_stream(ndp_handle *h, hipStream_t s)
{
    if (s == h->stream) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return 0; }
    NDP_HIP(h, hipEventRecord(h->evLast, s));
    h->ev_pending = true;
    return 0;
}
int wait_all(ndp_handle *h)
{
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    if (h->ev_pending) {
        NDP_HIP(h, hipEventSynchronize(h->evLast));
        h->ev_pending = false;
    }
    if (h->track_pending) {            // tracked control steps on a caller's stream (ndp_xchg_tick_step): the last one's completion event
        if (h->stepDone[h->step_seq & 3]) NDP_HIP(h, hipEventSynchronize(h->stepDone[h->step_seq & 3]));
        h->track_pending = false;
    }
    return 0;
}

int set_device(ndp_handle *h)
{
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    return 0;
}

// The automatic work-list rule (cfg.work_queue = 0, reference shape, at least two instances per SIMD).  The list re-balances interior-
// point solves over all SIMDs (+70 % at batch 4096 when a fifth of the instances iterate) but costs a step that lists nothing two more
// launches and a slower producer kernel: 8-15 % (batch 2048: 45.4 against 39.5 us; 16 384: 332 against 309 us).  So the handle starts in
// place and looks at what the steps do: the device keeps two monotonic counts -- instances that went into the interior-point loop (counted
// by the in-place kernel, added up by the list's reset launch) and control steps executed -- and a 16-byte copy of the pair is enqueued
// behind every QP_WINDOW-th launch.  Whenever a snapshot that covers QP_WINDOW more executed steps has LANDED (the host may be many
// launches ahead of the device), the fraction over those steps switches the list on at >= 4 %, off at <= 1.5 %.  Evaluated at launch
// time: a captured graph keeps the form it was captured in.
enum { QP_WINDOW = 8 };
static void queue_policy(ndp_handle *h, hipStream_t s)
{
    if (!h->queue_auto) return;
    const unsigned long long steps_now = ((volatile unsigned long long *)h->hIpm)[1], ipm_now = ((volatile unsigned long long *)h->hIpm)[0];
    if (steps_now >= h->steps_seen + QP_WINDOW && ipm_now >= h->ipm_seen) {
        const double frac = (double)(ipm_now - h->ipm_seen) / ((double)(steps_now - h->steps_seen) * (double)h->cfg.batch);
        if (frac >= 0.04) h->use_queue = true;
        else if (frac <= 0.015) h->use_queue = false;
        h->ipm_seen = ipm_now;
        h->steps_seen = steps_now;
    }
    if (++h->queue_launches < QP_WINDOW) return;
    h->queue_launches = 0;
    if (hipMemcpyAsync(h->hIpm, reinterpret_cast<unsigned long long *>(h->dQctr + 16), 16, hipMemcpyDeviceToHost, s) != hipSuccess) (void)hipGetLastError();
}

// The kernel of one launch of a step.  phase: 0 the in-place step, 1 / 2 the work list's producer / consumer.  (The late-force and tick
// forms have no sensitivity kernel: launch_rti refuses them first.)
static RtiId rti_pick(const ndp_handle *h, bool fused, bool tick, bool prefetched, int phase)
{
    const int N = h->cfg.N, W = h->waves, pr = h->cfg.qp_precision, wi = W == 4 ? 0 : W == 2 ? 1 : 2;
    const bool ref = N == 20 && h->cfg.n_rti == 1;     // the reference configuration (params/nmpc_params.py:9, 1 RTI iteration): compile-time instantiations
    if (pr) {                                          // BASELINE config 5 (unfused; run ndp_downwash first for a force)
        if (pr >= 3 && N == 40 && h->cfg.n_rti == 2 && W == 2) return pr == 3 ? K40_F32 : K40_BF16;   // config 5's own shape: 2 instances per workgroup
        return (RtiId)(KPREC1 + pr - 1);               // any horizon: one wave per workgroup (5 / 6: the condensed study, fp32 / bf16 instruction)
    }
    if (h->sens_level > 0) {
        // (ndp_sens_enable admits three-slot shapes at qp_precision 0, one RTI iteration, 2 or 4 instances per workgroup; work list: N = 20)
        RtiId id;
        if (phase) id = phase == 2 ? S20_CONS : fused ? S20F_PROD : S20_PROD;
        else if (N == 20 && W == 4) id = fused ? S20F : S20;
        else if (W == 4) id = fused ? SF_4 : S_4;
        else id = fused ? SF_2 : S_2;
        if (!h->dPSensXr) return id;
        // ndp_sens_params_enable (launch_rti has refused the unfused run-time horizon: S_4, S_2)
        switch (id) {
        case S20F_PROD: return P20F_PROD;
        case S20_PROD: return P20_PROD;
        case S20_CONS: return P20_CONS;
        case S20F: return P20F;
        case S20: return P20;
        case SF_4: return PF_4;
        default: return PF_2;
        }
    }
    if (phase == 2) return N == 20 ? K20_CONS : K40_CONS;
    if (phase == 1) {
        if (N != 20) return K40_PROD;
        if (tick) return fused ? K20F_PROD_TICK : K20_PROD_TICK;
        return fused ? K20F_PROD : K20_PROD;
    }
    if (ref && W == 4) {
        if (tick) return fused ? K20F_TICK : K20_TICK;
        return fused ? K20F : prefetched ? K20_LATE : K20;
    }
    if (ref && W == 2) return fused ? K20F_W2 : K20_W2;     // (NDP_DEV_WAVES = 2: the same program, two instances per workgroup)
    if (N == 40 && h->cfg.n_rti == 2 && W == 2 && !fused) return K40;   // BASELINE config 5's shape, compile-time as well
    if (fused) return (RtiId)(K3F_4 + wi);
    return (RtiId)((slots_for(N) <= 3 ? K3_4 : K5_4) + wi);
}

int launch_rti(ndp_handle *h, const double *d_x0, const double *d_xr, const double *d_ur, const float *d_f,
               double *d_u0, double *d_dbg, hipStream_t s, const Neigh *nb, const StepOut *so, bool prefetched)
{
    int *d_status = so && so->status ? so->status : h->dStatus, *d_iters = so && so->iters ? so->iters : h->dIters;
    h->lastStatus = d_status; h->lastIters = d_iters;
    BatchPtrs bp{h->dKC, h->dTables, d_x0, d_xr, d_ur, d_f, h->dX, h->dU, d_u0, d_status, d_iters,
                 so ? so->Xm : nullptr, so ? so->Um : nullptr, d_dbg, h->dStamps,
                 so && so->xr_pitch ? so->xr_pitch : (size_t)(h->cfg.N + 1) * NX, so && so->ur_pitch ? so->ur_pitch : (size_t)h->cfg.N * NU, (size_t)NX,
                 so ? so->cmd : nullptr, so ? so->kthr : nullptr, so ? so->thrust_keep : nullptr, h->cfg.mass, so && so->f_f64 ? 1 : 0,
                 h->dAct};
    const bool fused = nb && nb->other;
    MlpArgs ma{fused ? h->dFrag : nullptr, fused ? nb->other : nullptr, fused ? nb->ego_xy : nullptr, h->dForce,
               h->cfg.r_horiz * h->cfg.r_horiz, fused ? nb->stride : NX, fused ? nb->index : nullptr, fused ? peer_mapped(nb->other) : 0,
               fused && nb->pitch ? nb->pitch : (size_t)(h->cfg.N + 1) * (fused ? nb->stride : NX), fused && nb->ego_pitch ? nb->ego_pitch : (size_t)2};
    QueueArgs qa{h->dQctr, h->dQids, reinterpret_cast<unsigned long long *>(h->dQctr + 16)};
    LateArgs la{prefetched ? h->dProto : nullptr, {h->dForceAB[0], h->dForceAB[1]}, h->prefetch_timeout_us,
                h->pf_groups_rti, h->pf_ntiles};
    KernArgs ka{h->P, bp, h->cfg.batch, h->lds_per_wave, ma, qa, la, so && so->tick ? *so->tick : TickArgs{}};
    SensArgs sa{h->dSensU0, h->sens_level >= 2 ? h->dSensU : nullptr, h->sens_level >= 2 ? h->dSensX : nullptr, h->sens_level};
    const bool tick1 = so && so->tick;   // (tick_enqueue hands a TickArgs over only for the shapes the TICK kernels exist for)
    const int pr = h->cfg.qp_precision;
    const bool q = h->use_queue && !d_dbg && !prefetched;      // (the late-force step is in place: its launch is the lean instantiation)
    // Tracked steps carry their completion event on a dispatch packet (hipExtLaunchKernel), which a stream capture cannot hold:
    // refuse instead of launching something the graph would silently drop the event of.
    h->last_step_tracked = false;
    if (h->track_steps) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs != hipStreamCaptureStatusNone) {
            h->err = "tracked control steps (ndp_track_steps) cannot be launched on a stream that is being captured: switch tracking off "
                     "and order the exchange through the stream (ndp_xchg_begin's after_stream)";
            return -15;
        }
    }
    int rc = begin_timing(h, s, 0, true);
    if (rc) return rc;
    // timed launch of a single-kernel step: the pair rides on the dispatch packet (otherwise recorded around the launches)
    const bool ext_timing = h->timing_open && !q && !pr && !(so && so->done) && !h->track_steps;
    if (h->timing_open && !ext_timing) NDP_HIP(h, hipEventRecord(h->events.back().a, s));
    if (pr && fused) { h->err = "qp_precision != 0 supports f / no disturbance only (run ndp_downwash first)"; return -12; }
    // tracked steps: the LAST launch of the step carries the completion event (in-place kernel, or the work list's reset launch; the
    // precision studies, not on the exchange's fast path, record it behind their launch)
    hipEvent_t stop = nullptr;
    if (so && so->done) stop = so->done;
    else if (h->track_steps) { stop = h->stepDone[++h->step_seq & 3]; h->last_step_tracked = true; }
    if (h->sens_level > 0 && (prefetched || tick1)) { h->err = "launch_rti: the late-force and tick forms have no sensitivity kernel"; return -2; }
    launch_kern(h, rti_pick(h, fused, tick1, prefetched, q ? 1 : 0), s, ka, sa, ext_timing ? h->events.back().a : nullptr,
                ext_timing ? h->events.back().b : q || pr ? nullptr : stop);
    if (ext_timing) h->timing_open = false;     // (end_timing has nothing left to record)
    NDP_HIP(h, hipGetLastError());
    if (q) {
        // work list: producer (every instance: one solve with the kept set's pins, done or defer), consumer (the deferred ones, from
        // scratch: active-set iterations, then the interior-point loop if need be; several RTI iterations: the automatic rule per
        // iteration), a one-wave launch that empties the list for the next step.  The consumer reads the fused producer's
        // force from dForce.
        KernArgs kc = ka;
        kc.bp.f = fused ? h->dForce : d_f;
        kc.ma.frag = nullptr; kc.ma.other = nullptr;
        // (active-set iterations off: a listed instance needs the interior-point loop, the consumer goes straight to it; on: the
        // producer lists every instance whose first solve -- with the kept set's pins -- did not settle, the consumer iterates on the set)
        if (h->cfg.n_rti == 1 && h->cfg.as_iter_max <= 0) kc.P.qp_mode = QP_IPM_ALWAYS;
        launch_kern(h, rti_pick(h, fused, tick1, prefetched, 2), s, kc, sa);
        NDP_HIP(h, hipGetLastError());
        if (stop) hipExtLaunchKernelGGL(queue_reset_kernel, dim3(1), dim3(64), 0, s, nullptr, stop, 0, h->dQctr.get(), qa.ipm_total);
        else hipLaunchKernelGGL(queue_reset_kernel, dim3(1), dim3(64), 0, s, h->dQctr, qa.ipm_total);
        NDP_HIP(h, hipGetLastError());
    } else if (pr && stop) NDP_HIP(h, hipEventRecord(stop, s));
    const int rce = end_timing(h, s);
    queue_policy(h, s);
    return rce;
}

// downwash inside the RTI launch when one 32-row tile covers the horizon; otherwise mlp_kernel first
bool can_fuse(const ndp_handle *h)
{
    return h->cfg.qp_precision == 0 && h->cfg.N + 1 <= 32 && slots_for(h->cfg.N) <= 3 &&
           (size_t)h->lds_per_wave * sizeof(double) * h->waves >= FR_TOTAL * sizeof(float);
}

// one control step on device pointers: [mlp_kernel ->] rti_kernel (no locking, no sync)
int enqueue_step(ndp_handle *h, const double *d_x0, const double *d_xr, const double *d_ur, const float *d_f,
                 const Neigh &nb, double *d_u0, double *d_dbg, hipStream_t s, const StepOut *so)
{
    // The unfused step at a run-time horizon has no parameter-sensitivity kernel (rti_psens_kernel): that instantiation of the shared body
    // sits at the register limit and would carry a scratch-memory frame.  The fused step (any N <= 27) and the N = 20 kernels serve them.
    if (h->dPSensXr && !(nb.other && can_fuse(h)) && !(h->cfg.N == 20 && h->waves == 4)) {
        h->err = "ndp_step: parameter sensitivities at N != 20 (or 2 instances per workgroup) need the fused step (neighbour windows "
                 "given): the unfused kernel of a run-time horizon has none";
        return -2;
    }
    if ((d_f || nb.other) && !h->cfg.use_fd) { h->err = "ndp_step: a disturbance force needs use_fd = 1 (NDP model)"; return -8; }
    if (nb.other) {
        if (d_f) { h->err = "ndp_step: pass either f or other, not both"; return -7; }
        if (nb.stride != 10 && nb.stride != 6) { h->err = "ndp_step: other_stride must be 10 or 6"; return -13; }
        if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
        if (can_fuse(h)) return launch_rti(h, d_x0, d_xr, d_ur, nullptr, d_u0, d_dbg, s, &nb, so);
        int rc = launch_mlp(h, nb, d_xr, h->dForce, s, so ? so->xr_pitch : 0);
        if (rc) return rc;
        d_f = h->dForce;
    }
    return launch_rti(h, d_x0, d_xr, d_ur, d_f, d_u0, d_dbg, s, nullptr, so);
}

int ndp_reset_device(ndp_handle *h, const void *d_xr, const void *d_ur, void *stream)
{
    Entry g(h, d_xr && d_ur, stream);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipMemcpyAsync(h->dX, d_xr, nxs(h) * 8, hipMemcpyDefault, g.s));
    NDP_HIP(h, hipMemcpyAsync(h->dU, d_ur, nus(h) * 8, hipMemcpyDefault, g.s));
    NDP_HIP(h, hipMemsetAsync(h->dAct, 0, act_bytes(h), g.s));      // a new iterate: the QPs start from an empty active set
    return g.noted(0);
}

int ndp_reset(ndp_handle *h, const double *xr, const double *ur)
{
    Entry g(h, xr && ur);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(h->dX, xr, nxs(h) * 8, hipMemcpyDefault, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->dU, ur, nus(h) * 8, hipMemcpyDefault, h->stream));
    NDP_HIP(h, hipMemsetAsync(h->dAct, 0, act_bytes(h), h->stream));
    return g.synced(0);
}

int ndp_step_device_ex(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                       const void *d_other, int other_stride, const void *d_other_index, const void *d_ego_xy,
                       void *d_u0, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_u0, stream);
    if (g.rc) return g.rc;
    Neigh nb;
    nb.other = (const double *)d_other; nb.stride = other_stride; nb.index = (const int *)d_other_index; nb.ego_xy = (const double *)d_ego_xy;
    return g.noted(enqueue_step(h, (const double *)d_x0, (const double *)d_xr, (const double *)d_ur, (const float *)d_f, nb,
                                (double *)d_u0, nullptr, g.s));
}

int ndp_step_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                    const void *d_other, const void *d_ego_xy, void *d_u0, void *stream)
{
    return ndp_step_device_ex(h, d_x0, d_xr, d_ur, d_f, d_other, NX, nullptr, d_ego_xy, d_u0, stream);
}

// ---- host-array step: ndp_step_begin (pack -> H2D -> kernel -> D2H, nothing waits) + ndp_step_end (wait, hand the results over)
int ensure_slots(ndp_handle *h)
{
    if (h->slots_ready) return 0;
    for (int i = 0; i < 2; ++i) {
        ndp_handle::HostSlot &sl = h->slot[i];
        // (only what is missing: a call that failed part-way left the members it did allocate, and they are reused)
        NDP_HIP(h, sl.hIn.ensure(h->in_bytes));
        if (!sl.hOut) {
            NDP_HIP(h, sl.hOut.alloc(h->out_all));
            memset(sl.hOut, 0, h->out_bytes);
        }
        NDP_HIP(h, sl.evOut.ensure(hipEventDisableTiming));
    }
    // pack threads: NDP_PACK_THREADS, else half the cores this process may really use, at most 8; the caller packs too, so small blocks
    // need none.  (Rounds 3-5 counted the machine's hardware threads: in a container whose CPU quota is a fraction of the machine that
    // put seven spinning threads on two or three cores' worth of time -- the same ndp_step_begin / _end leg measured 4.5 M solves/s on one
    // box and 11.5 M on another.)
    int nt = 0;
    h->host_cores = usable_cores();
    if (const char *e = getenv("NDP_PACK_THREADS")) nt = atoi(e);
    else if (h->in_bytes > 2 * PACK_CHUNK) nt = (h->host_cores / 2 > 8 ? 8 : h->host_cores / 2) - 1;
    h->pack_threads = nt > 0 ? (nt > 64 ? 64 : nt) : 0;
    h->pool.reset(new (std::nothrow) PackPool(h->pack_threads));
    if (!h->pool) { h->err = "ensure_slots: out of memory"; return -4; }
    h->slots_ready = true;
    return 0;
}

static int step_begin_locked(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                             const double *other, const double *ego_xy, bool want_iter, double *dump, bool f_f64 = false)
{
    const size_t B = h->cfg.batch;
    hipStream_t s = h->stream;
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = ensure_slots(h);
    if (rc) return rc;
    if (h->slots_busy == 2) { h->err = "ndp_step_begin: two steps are already in flight (call ndp_step_end first)"; return -14; }
    if (h->ev_pending && (rc = wait_all(h))) return rc;       // work a caller left on its own stream comes first
    ndp_handle::HostSlot &sl = h->slot[h->slot_head];
    // the slot's previous use is over: its results were handed out by ndp_step_end (busy is false), so the kernel that read
    // its input mirror and wrote its output mirror has completed and both are free to overwrite
    // the block of THIS step: the arrays that were given, one behind the other (256-byte aligned), so that one transfer moves
    // exactly what the kernel reads; neighbour windows as their 6 position / velocity columns
    struct Seg { size_t off; const void *src; size_t len; size_t rows, row_len, src_stride; };
    Seg segs[6];
    int ns = 0;
    size_t o = 0;
    auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    auto add = [&](const void *src, size_t len, size_t rows = 0, size_t row_len = 0, size_t src_stride = 0) {
        segs[ns] = {o, src, len, rows, row_len, src_stride};
        o += up256(len);
        return segs[ns++].off;
    };
    const size_t rows_o = B * (size_t)(h->cfg.N + 1);
    const size_t o_x0 = add(x0, B * NX * 8), o_xr = add(xr, nxs(h) * 8), o_ur = add(ur, nus(h) * 8);
    const size_t o_f = f ? add(f, nfs(h) * (f_f64 ? 8 : 4)) : 0;
    const size_t o_other = other ? add(other, rows_o * 6 * 8, rows_o, 6 * 8, NX * 8) : 0;
    const size_t o_ego = ego_xy ? add(ego_xy, B * 2 * 8) : 0;
    const size_t used = o;          // <= in_bytes (the mirror holds every array at full width)
    std::vector<PackJob> jobs;
    for (int i = 0; i < ns; ++i) {
        if (segs[i].rows) {
            const size_t rows_per = PACK_CHUNK / segs[i].src_stride;
            for (size_t r = 0; r < segs[i].rows; r += rows_per) {
                const size_t n = segs[i].rows - r < rows_per ? segs[i].rows - r : rows_per;
                jobs.push_back({sl.hIn + segs[i].off + r * segs[i].row_len, (const unsigned char *)segs[i].src + r * segs[i].src_stride,
                                segs[i].row_len, n, segs[i].src_stride});
            }
            continue;
        }
        for (size_t c = 0; c < segs[i].len; c += PACK_CHUNK) {
            const size_t n = segs[i].len - c < PACK_CHUNK ? segs[i].len - c : PACK_CHUNK;
            jobs.push_back({sl.hIn + segs[i].off + c, (const unsigned char *)segs[i].src + c, n});
        }
    }
    const int nj = (int)jobs.size();
    PackPool &pool = *h->pool;
    const auto tp0 = std::chrono::steady_clock::now();
    pool.post(jobs.data(), nj);      // from here to pool.finish() nothing returns early: the workers read `jobs`
    for (int i = 0; i < nj; ++i) pool.wait_job(i);
    pool.finish();
    const auto tp1 = std::chrono::steady_clock::now();
    // Zero-copy: the kernel reads the input mirror itself over PCIe and writes u0 | status | iterations (| the new iterate, when
    // asked for) into the output mirror itself: page-locked host memory, device-accessible, no DMA operation.  (One transfer of
    // the block per step into an HBM copy on a stream of its own, beside the previous tick's kernel, was built and measured in
    // four sessions: 85-103 us per step at batch 1024 against 90-96 this way, 290-343 against 315-342 at 4096 -- between 8 %
    // better and 10 % worse, one tick at a time always 5 % worse.  PCIe moves ~40-48 GB/s here whoever issues the reads.  Not kept.)
    const unsigned char *ib = sl.hIn;
    (void)used;
    Neigh nb;
    nb.other = other ? (const double *)(ib + o_other) : nullptr;
    nb.stride = 6;
    nb.ego_xy = ego_xy ? (const double *)(ib + o_ego) : nullptr;
    StepOut so;
    so.status = (int *)(sl.hOut + h->off_st); so.iters = (int *)(sl.hOut + h->off_it);
    if (want_iter) { so.Xm = (double *)(sl.hOut + h->out_bytes); so.Um = so.Xm + nxs(h); }
    so.f_f64 = f_f64;
    // one packet less between the kernel's end and the host seeing it: the completion event rides on the step's last dispatch packet
    const bool ext_done = !dump && h->cfg.qp_precision == 0 && (!other || can_fuse(h)) && !getenv("NDP_HOST_EVENT_RECORD");
    if (ext_done) so.done = sl.evOut;
    rc = enqueue_step(h, (const double *)(ib + o_x0), (const double *)(ib + o_xr), (const double *)(ib + o_ur),
                      f ? (const float *)(ib + o_f) : nullptr, nb, (double *)(sl.hOut + h->off_u0), dump ? h->sdbg : nullptr, s, &so);
    if (rc) return rc;
    // (sl.evOut was marked by the step's own dispatch packet -- so.done -- unless the step ran the separate downwash launch path,
    // a debug dump or a precision study, where it is recorded behind the launches as usual)
    if (!ext_done) NDP_HIP(h, hipEventRecord(sl.evOut, s));
    sl.busy = true; sl.want_iter = want_iter; sl.dump = dump;
    h->host_us[0] = std::chrono::duration<double, std::micro>(tp1 - tp0).count();
    h->host_us[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tp1).count();
    h->slot_head ^= 1;
    ++h->slots_busy;
    return 0;
}

static int step_end_locked(ndp_handle *h, double *u0, double *X_out, double *U_out, int32_t *status_out, int32_t *iters_out)
{
    const size_t B = h->cfg.batch;
    if (h->slots_busy == 0) { h->err = "ndp_step_end: no step in flight (ndp_step_begin first)"; return -14; }
    if (h->tslot[h->slot_tail].busy) { h->err = "ndp_step_end: the oldest call in flight is a tick (ndp_tick_end it)"; return -14; }
    ndp_handle::HostSlot &sl = h->slot[h->slot_tail];
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    if ((X_out || U_out) && !sl.want_iter) { h->err = "ndp_step_end: the iterate was not requested at ndp_step_begin (flags bit 0)"; return -15; }
    // the step is a few tens of microseconds from done: poll the event before blocking on it (a blocking wait adds its wake-up)
    const auto tw0 = std::chrono::steady_clock::now();
    hipError_t e = hipErrorNotReady;
    for (int spin = 0; spin < 4000 && e == hipErrorNotReady; ++spin) e = hipEventQuery(sl.evOut);
    if (e == hipErrorNotReady) e = hipEventSynchronize(sl.evOut);
    if (e == hipSuccess && sl.dump)
        e = hipMemcpy(sl.dump, h->sdbg, (size_t)(lds_doubles(h->cfg.N) + DBG_EXTRA) * 8, hipMemcpyDeviceToHost);
    sl.busy = false;
    h->slot_tail ^= 1;
    --h->slots_busy;
    NDP_HIP(h, e);
    const auto tw1 = std::chrono::steady_clock::now();
    const unsigned char *ho = sl.hOut;
    if (u0) memcpy(u0, ho + h->off_u0, B * NU * 8);
    const int32_t *st = (const int32_t *)(ho + h->off_st);
    if (status_out) memcpy(status_out, st, B * 4);
    if (iters_out) copy_ipm_iters(iters_out, reinterpret_cast<const int32_t *>(ho + h->off_it), B);
    if (X_out) memcpy(X_out, ho + h->out_bytes, nxs(h) * 8);
    if (U_out) memcpy(U_out, ho + h->out_bytes + nxs(h) * 8, nus(h) * 8);
    int w = 0;
    for (size_t i = 0; i < B; ++i) w = st[i] > w ? st[i] : w;
    h->host_us[2] = std::chrono::duration<double, std::micro>(tw1 - tw0).count();
    h->host_us[3] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw1).count();
    return w;
}

int ndp_debug_host_info(ndp_handle *h, int32_t *out3)
{
    if (!h || !out3) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    out3[0] = (int32_t)std::thread::hardware_concurrency();
    out3[1] = h->slots_ready ? h->host_cores : usable_cores();
    out3[2] = h->slots_ready ? h->pack_threads : -1;
    return 0;
}

int ndp_debug_rti_launched(ndp_handle *h, uint64_t *mask, int32_t *out3)
{
    if (!h) return -1;
    if (mask) *mask = h->rti_launched.exchange(0, std::memory_order_relaxed);
    if (out3) {
        out3[0] = RTI_KERNELS;
        out3[1] = h->waves;
        out3[2] = can_fuse(h) ? 1 : 0;
    }
    return 0;
}

int ndp_debug_host_timing(ndp_handle *h, double *out4)
{
    if (!h || !out4) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < 4; ++i) out4[i] = h->host_us[i];
    return 0;
}

int ndp_step_begin(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                   const double *other, const double *ego_xy, int flags)
{
    if (!h || !x0 || !xr || !ur) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    return step_begin_locked(h, x0, xr, ur, f, other, ego_xy, (flags & 1) != 0, nullptr);
}

int ndp_step_end(ndp_handle *h, double *u0, double *X_out, double *U_out, int32_t *status_out, int32_t *iters_out)
{
    if (!h || !u0) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    return step_end_locked(h, u0, X_out, U_out, status_out, iters_out);
}

// The synchronous form: begin + end under ONE lock (a concurrent caller cannot slip a step in between).
static int step_host(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                     const double *other, const double *ego_xy, double *u0, double *X_out, double *U_out,
                     int32_t *status_out, int32_t *iters_out, double *dump, bool f_f64 = false)
{
    if (!h || !x0 || !xr || !ur || !u0) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->slots_busy) { h->err = "ndp_step: steps begun with ndp_step_begin are still in flight (ndp_step_end them first)"; return -14; }
    int rc = step_begin_locked(h, x0, xr, ur, f, other, ego_xy, X_out || U_out, dump, f_f64);
    if (rc) return rc;
    return step_end_locked(h, u0, X_out, U_out, status_out, iters_out);
}

int ndp_step(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
             const double *other, const double *ego_xy, double *u0)
{
    return step_host(h, x0, xr, ur, f, other, ego_xy, u0, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int ndp_step_ex(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                const double *other, const double *ego_xy, double *u0, double *X_out, double *U_out,
                int32_t *status_out, int32_t *iters_out)
{
    return step_host(h, x0, xr, ur, f, other, ego_xy, u0, X_out, U_out, status_out, iters_out, nullptr);
}

int ndp_step_ex_f64(ndp_handle *h, const double *x0, const double *xr, const double *ur, const double *f, double *u0,
                    double *X_out, double *U_out, int32_t *status_out, int32_t *iters_out)
{
    return step_host(h, x0, xr, ur, reinterpret_cast<const float *>(f), nullptr, nullptr, u0, X_out, U_out, status_out, iters_out, nullptr, f != nullptr);
}

int ndp_step_debug(ndp_handle *h, const double *x0, const double *xr, const double *ur, const float *f,
                   const double *other, const double *ego_xy, double *u0, double *lds_dump)
{
    if (h && h->cfg.batch != 1) { h->err = "ndp_step_debug: batch must be 1"; return -9; }
    return step_host(h, x0, xr, ur, f, other, ego_xy, u0, nullptr, nullptr, nullptr, nullptr, lds_dump);
}

int ndp_get_iterate(ndp_handle *h, double *X, double *U)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if (X) NDP_HIP(h, hipMemcpy(X, h->dX, nxs(h) * 8, hipMemcpyDefault));
    if (U) NDP_HIP(h, hipMemcpy(U, h->dU, nus(h) * 8, hipMemcpyDefault));
    return 0;
}

int ndp_set_iterate(ndp_handle *h, const double *X, const double *U)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if (X) NDP_HIP(h, hipMemcpy(h->dX, X, nxs(h) * 8, hipMemcpyDefault));
    if (U) NDP_HIP(h, hipMemcpy(h->dU, U, nus(h) * 8, hipMemcpyDefault));
    NDP_HIP(h, hipMemset(h->dAct, 0, act_bytes(h)));
    return 0;
}

int ndp_get_active_set(ndp_handle *h, int32_t *sweeps, int8_t *act)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t B = (size_t)h->cfg.batch;
    if (sweeps) {
        NDP_HIP(h, hipMemcpy(sweeps, h->lastIters, B * 4, hipMemcpyDefault));
        for (size_t i = 0; i < B; ++i) sweeps[i] = (int32_t)((uint32_t)sweeps[i] >> ITERS_SWEEP_SHIFT);
    }
    if (act) NDP_HIP(h, hipMemcpy(act, h->dAct, act_bytes(h), hipMemcpyDefault));
    return 0;
}

int ndp_set_active_set(ndp_handle *h, const int8_t *act)
{
    Entry g(h, act);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t n = act_bytes(h);
    for (size_t i = 0; i < n; ++i)
        if (act[i] < -1 || act[i] > 1) { h->err = "ndp_set_active_set: entries are -1, 0 or +1"; return -1; }
    NDP_HIP(h, hipMemcpy(h->dAct, act, n, hipMemcpyDefault));
    return 0;
}

int ndp_get_status(ndp_handle *h, int32_t *status, int32_t *ipm_iters)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    int rc = wait_all(h);
    if (rc) return rc;
    if (status) NDP_HIP(h, hipMemcpy(status, h->lastStatus, (size_t)h->cfg.batch * 4, hipMemcpyDefault));
    if (ipm_iters) {
        NDP_HIP(h, hipMemcpy(ipm_iters, h->lastIters, (size_t)h->cfg.batch * 4, hipMemcpyDefault));
        copy_ipm_iters(ipm_iters, ipm_iters, (size_t)h->cfg.batch);
    }
    return 0;
}

// test/profiling hook: every instance writes its phase stamps (shader clock) to [B][NDP_NSTAMP] doubles
int ndp_debug_stamps(ndp_handle *h, int enable, double *out)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    NDP_HIP(h, hipDeviceSynchronize());
    const size_t bytes = (size_t)h->cfg.batch * NDP_NSTAMP * 8;
    if (out && h->dStamps) NDP_HIP(h, hipMemcpy(out, h->dStamps, bytes, hipMemcpyDeviceToHost));
    if (enable && !h->dStamps) {
        NDP_HIP(h, h->dStamps.alloc(bytes));
        NDP_HIP(h, hipMemset(h->dStamps, 0, bytes));
    } else if (!enable) h->dStamps.reset();
    return 0;
}

void *ndp_device_iterate_x(ndp_handle *h) { return h ? h->dX : nullptr; }
void *ndp_device_iterate_u(ndp_handle *h) { return h ? h->dU : nullptr; }
void *ndp_device_force(ndp_handle *h) { return h ? h->dForce : nullptr; }
int ndp_work_queue_enabled(ndp_handle *h) { return h ? (int)h->use_queue : -1; }

// ---- the sensitivity buffers: created on enabling, NaN until a step has written them
static int nan_buffer(ndp_handle *h, DevBuf<double> &p, size_t n)
{
    if (p) return 0;
    NDP_HIP(h, p.alloc(n * 8));
    NDP_HIP(h, hipMemsetAsync(p, 0xff, n * 8, h->stream));
    return 0;
}
static int copy_out(ndp_handle *h, double *dst, const double *src, size_t n)
{
    if (dst) NDP_HIP(h, hipMemcpy(dst, src, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

// ---- initial-state sensitivities (rti_sens_kernel, RtiWave::sens_out)
int ndp_sens_enable(ndp_handle *h, int level)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (level < 0 || level > 2) { h->err = "ndp_sens_enable: level must be 0 (off), 1 (du0/dx0) or 2 (also dU/dx0 and dX/dx0)"; return -2; }
    if (level > 0) {
        if (slots_for(h->cfg.N) > 3) { h->err = "ndp_sens_enable: sensitivities are served for N <= 27 only (the five-slot kernels of N >= 28 have none)"; return -2; }
        if (h->cfg.qp_precision != 0) { h->err = "ndp_sens_enable: sensitivities need qp_precision 0 (the fp64 product path)"; return -2; }
        if (h->cfg.n_rti != 1) { h->err = "ndp_sens_enable: sensitivities need n_rti = 1 (the derivative of the step's one QP)"; return -2; }
        if (h->waves != 4 && h->waves != 2) { h->err = "ndp_sens_enable: the sensitivity kernels run 2 or 4 instances per workgroup"; return -2; }
    }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);                 // (steps in flight may still write the buffers)
    if (rc) return rc;
    const size_t B = h->cfg.batch, N = h->cfg.N;
    const size_t n0 = B * (size_t)sens_u0_pitch(), nu = B * (size_t)sens_u_pitch((int)N), nx = B * (size_t)sens_x_pitch((int)N);
    if (level < 2) { h->dSensU.reset(); h->dSensX.reset(); }
    if (level == 0) { for (DevBuf<double> *p : {&h->dSensU0, &h->dPSensXr, &h->dPSensUr, &h->dPSensF}) p->reset(); h->sens_level = 0; return 0; }
    if ((rc = nan_buffer(h, h->dSensU0, n0))) return rc;
    if (level == 2 && ((rc = nan_buffer(h, h->dSensU, nu)) || (rc = nan_buffer(h, h->dSensX, nx)))) return rc;
    const char *what = nullptr;
    NDP_HIP(h, rti_set_lds(true, (int)((size_t)h->lds_per_wave * sizeof(double) * h->waves), &what));
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    h->sens_level = level;
    return 0;
}

int ndp_sens_level(ndp_handle *h) { return h ? h->sens_level : -1; }

int ndp_get_sens(ndp_handle *h, double *du0_dx0, double *dU_dx0, double *dX_dx0)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->sens_level < 1) { h->err = "ndp_get_sens: sensitivities are not enabled (ndp_sens_enable)"; return -2; }
    if ((dU_dx0 || dX_dx0) && h->sens_level < 2) { h->err = "ndp_get_sens: dU/dx0 and dX/dx0 need sensitivity level 2"; return -2; }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t B = h->cfg.batch;
    if ((rc = copy_out(h, du0_dx0, h->dSensU0, B * sens_u0_pitch()))) return rc;
    if ((rc = copy_out(h, dU_dx0, h->dSensU, B * sens_u_pitch(h->cfg.N)))) return rc;
    return copy_out(h, dX_dx0, h->dSensX, B * sens_x_pitch(h->cfg.N));
}

void *ndp_device_sens_u0(ndp_handle *h) { return h ? h->dSensU0 : nullptr; }
void *ndp_device_sens_u(ndp_handle *h) { return h ? h->dSensU : nullptr; }
void *ndp_device_sens_x(ndp_handle *h) { return h ? h->dSensX : nullptr; }

// ---- parameter sensitivities (rti_psens_kernel, RtiWave::psens_out)
int ndp_sens_params_enable(ndp_handle *h, int on)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (on && h->sens_level < 1) {
        h->err = "ndp_sens_params_enable: parameter sensitivities need initial-state sensitivities on (ndp_sens_enable(h, 1 or 2) first)";
        return -2;
    }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);                 // (steps in flight may still write the buffers)
    if (rc) return rc;
    if (!on) {
        for (DevBuf<double> *p : {&h->dPSensXr, &h->dPSensUr, &h->dPSensF}) p->reset();
        return 0;
    }
    const size_t B = h->cfg.batch;
    const int N = h->cfg.N;
    if ((rc = nan_buffer(h, h->dPSensXr, B * (size_t)psens_xr_pitch(N))) || (rc = nan_buffer(h, h->dPSensUr, B * (size_t)psens_ur_pitch(N))) ||
        (rc = nan_buffer(h, h->dPSensF, B * (size_t)psens_f_pitch(N))))
        return rc;
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ndp_sens_params_enabled(ndp_handle *h) { return h ? (int)(h->dPSensXr != nullptr) : -1; }

int ndp_get_sens_params(ndp_handle *h, double *du0_dxr, double *du0_dur, double *du0_df)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->dPSensXr) { h->err = "ndp_get_sens_params: parameter sensitivities are not enabled (ndp_sens_params_enable)"; return -2; }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);
    if (rc) return rc;
    const size_t B = h->cfg.batch;
    const int N = h->cfg.N;
    if ((rc = copy_out(h, du0_dxr, h->dPSensXr, B * psens_xr_pitch(N)))) return rc;
    if ((rc = copy_out(h, du0_dur, h->dPSensUr, B * psens_ur_pitch(N)))) return rc;
    return copy_out(h, du0_df, h->dPSensF, B * psens_f_pitch(N));
}

void *ndp_device_sens_xr(ndp_handle *h) { return h ? h->dPSensXr : nullptr; }
void *ndp_device_sens_ur(ndp_handle *h) { return h ? h->dPSensUr : nullptr; }
void *ndp_device_sens_f(ndp_handle *h) { return h ? h->dPSensF : nullptr; }

// ---- adjoint of the control step (rti_vjp_kernel, RtiWave::vjp_out)
void *ndp_device_active_set(ndp_handle *h) { return h ? h->dAct : nullptr; }

// The refusals all of the entries that recompute a recorded step make (struct Tape, host.hpp), in their order: the configuration's and the
// required pointers', then `own` -- the entry's refusals of its own arguments, or null -- then the force's.  Empty: none.  noun: what the
// entry's texts call the derivative.
extern "C++" {
std::string recompute_refusal(const ndp_cfg &c, const char *noun, const Tape &t, const char *own)
{
    const std::string the = std::string("the ") + noun;
    if (c.n_rti != 1) return the + " needs n_rti = 1 (the derivative of the step's one QP)";
    if (c.qp_precision != 0) return the + " needs qp_precision 0 (the fp64 product path)";
    if (slots_for(c.N) > 3) return the + " is served for N <= 27 only (the five-slot kernels of N >= 28 have none)";
    if (!t.x0 || !t.xr || !t.ur || !t.X_lin || !t.U_lin) return "x0, xr, ur and the tape's iterate (X_lin, U_lin) are required";
    if (own) return own;
    if (t.f && !c.use_fd) return "a disturbance force needs use_fd = 1 (NDP model)";
    return "";
}
}  // extern "C++"

// The launch, in two parts.  recompute_workspace: the handle's workspace (first call).  recompute_on_workspace: the step's kernel arguments
// on the workspace's copy of the tape (t.X_lin, U_lin, act_lin are NOT read: whoever calls it has put them there on stream s), then the
// kernel for the horizon (fn20: the compile-time N = 20, else fn0) with a1, a2 behind them (a2: null if it takes two).
int recompute_workspace(ndp_handle *h)
{
    const size_t B = h->cfg.batch;
    NDP_HIP(h, h->dVjp.ensure((nxs(h) + nus(h) + B * NU) * 8));
    NDP_HIP(h, h->dVjpSt.ensure(B * 2 * 4));
    NDP_HIP(h, h->dVjpAct.ensure(act_bytes(h)));
    return 0;
}

int recompute_on_workspace(ndp_handle *h, hipStream_t s, const Tape &t, const void *fn20, const void *fn0, void *a1, void *a2)
{
    const ndp_cfg &c = h->cfg;
    const size_t B = c.batch;
    double *X = h->dVjp, *U = X + nxs(h), *u0 = U + nus(h);
    int *st = h->dVjpSt, *it = st + B;
    BatchPtrs bp{h->dKC, h->dTables, (const double *)t.x0, (const double *)t.xr, (const double *)t.ur, (const float *)t.f, X, U,
                 t.u0_check ? (double *)t.u0_check : u0, t.status_check ? (int *)t.status_check : st, it, nullptr, nullptr, nullptr, nullptr,
                 (size_t)(c.N + 1) * NX, (size_t)c.N * NU, (size_t)NX, nullptr, nullptr, nullptr, c.mass, 0, h->dVjpAct};
    KernArgs ka{h->P, bp, (int)B, h->lds_per_wave, MlpArgs{}, QueueArgs{}, LateArgs{}, TickArgs{}};
    const int W = h->waves;
    const void *fn = c.N == 20 ? fn20 : fn0;
    void *args[] = {&ka, a1, a2};
    NDP_HIP(h, hipLaunchKernel(fn, dim3((unsigned)((B + W - 1) / W)), dim3(64 * W), args, (size_t)h->lds_per_wave * sizeof(double) * W, s));
    NDP_HIP(h, hipGetLastError());
    return 0;
}

// The entries below: the workspace, the tape copied into it on the entry's stream, the launch.
static int recompute_launch(ndp_handle *h, Entry &g, const Tape &t, const void *fn20, const void *fn0, void *a1, void *a2)
{
    hipStream_t s = g.s;
    int rc = recompute_workspace(h);
    if (rc) return rc;
    double *X = h->dVjp, *U = X + nxs(h);
    NDP_HIP(h, hipMemcpyAsync(X, t.X_lin, nxs(h) * 8, hipMemcpyDeviceToDevice, s));
    NDP_HIP(h, hipMemcpyAsync(U, t.U_lin, nus(h) * 8, hipMemcpyDeviceToDevice, s));
    if (t.act_lin) NDP_HIP(h, hipMemcpyAsync(h->dVjpAct, t.act_lin, act_bytes(h), hipMemcpyDeviceToDevice, s));
    else NDP_HIP(h, hipMemsetAsync(h->dVjpAct, 0, act_bytes(h), s));
    if ((rc = recompute_on_workspace(h, s, t, fn20, fn0, a1, a2))) return rc;
    return g.noted(0);
}

// model: the entry is ndp_step_vjp_model_device (rti_wvjp_kernel; d_gmodel required), else ndp_step_vjp_device (rti_vjp_kernel)
static int step_vjp(ndp_handle *h, const Tape &t, const void *d_gu0, const void *d_gX, const void *d_gU,
                    void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *stream, bool model, void *d_gmodel)
{
    Entry g(h, true, stream);
    if (g.rc) return g.rc;
    std::string why = recompute_refusal(h->cfg, "adjoint", t, !d_gu0 && !d_gX && !d_gU ? "no upstream gradient (gu0, gX and gU all NULL)" : nullptr);
    if (why.empty() && model && !d_gmodel) why = "gmodel is required (without it: ndp_step_vjp_device)";
    if (!why.empty()) { h->err = std::string(model ? "ndp_step_vjp_model_device: " : "ndp_step_vjp_device: ") + why; return -2; }
    VjpArgs va{(const double *)d_gu0, (const double *)d_gX, (const double *)d_gU, (double *)d_gx0, (double *)d_gxr, (double *)d_gur,
               (double *)d_gf};
    double *gm = (double *)d_gmodel;
    if (model) return recompute_launch(h, g, t, recompute_kernel(RC_WVJP, true), recompute_kernel(RC_WVJP, false), &va, &gm);
    return recompute_launch(h, g, t, recompute_kernel(RC_VJP, true), recompute_kernel(RC_VJP, false), &va, nullptr);
}

int ndp_step_vjp_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                        const void *d_X_lin, const void *d_U_lin, const void *d_act_lin,
                        const void *d_gu0, const void *d_gX, const void *d_gU,
                        void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_u0_check, void *d_status_check, void *stream)
{
    return step_vjp(h, Tape{d_x0, d_xr, d_ur, d_f, d_X_lin, d_U_lin, d_act_lin, d_u0_check, d_status_check}, d_gu0, d_gX, d_gU, d_gx0, d_gxr,
                    d_gur, d_gf, stream, false, nullptr);
}

int ndp_step_vjp_model_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                              const void *d_X_lin, const void *d_U_lin, const void *d_act_lin,
                              const void *d_gu0, const void *d_gX, const void *d_gU,
                              void *d_gx0, void *d_gxr, void *d_gur, void *d_gf, void *d_gmodel, void *d_u0_check, void *d_status_check,
                              void *stream)
{
    return step_vjp(h, Tape{d_x0, d_xr, d_ur, d_f, d_X_lin, d_U_lin, d_act_lin, d_u0_check, d_status_check}, d_gu0, d_gX, d_gU, d_gx0, d_gxr,
                    d_gur, d_gf, stream, true, d_gmodel);
}

// ---- forward mode of the control step (rti_jvp_kernel, RtiWave::jvp_out): the adjoint's recompute, workspace and tape rules
// model: the entry is ndp_step_jvp_model_device (rti_mjvp_kernel; d_tmodel required, the data tangents may all be NULL), else
// ndp_step_jvp_device (rti_jvp_kernel)
static int step_jvp(ndp_handle *h, const Tape &t, int n_tan, const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf,
                    void *d_du0, void *d_dX, void *d_dU, void *stream, bool model, const void *d_tmodel)
{
    Entry g(h, true, stream);
    if (g.rc) return g.rc;
    const char *own = nullptr;
    if (n_tan < 1 || n_tan > NDP_JVP_MAX_TANGENTS) own = "n_tan must be 1..8 (directions per call)";
    else if (!model && !d_tx0 && !d_txr && !d_tur && !d_tf) own = "no tangent (tx0, txr, tur and tf all NULL)";
    else if (!d_du0 && !d_dX && !d_dU) own = "no output asked for (du0, dX and dU all NULL)";
    std::string why = recompute_refusal(h->cfg, "derivative", t, own);
    if (why.empty() && d_tf && !h->cfg.use_fd) why = "a force tangent needs use_fd = 1 (NDP model)";
    if (why.empty() && model && !d_tmodel) why = "tmodel is required (without it: ndp_step_jvp_device)";
    if (!why.empty()) { h->err = std::string(model ? "ndp_step_jvp_model_device: " : "ndp_step_jvp_device: ") + why; return -2; }
    JvpArgs ja{(const double *)d_tx0, (const double *)d_txr, (const double *)d_tur, (const double *)d_tf, (double *)d_du0, (double *)d_dX,
               (double *)d_dU, n_tan};
    const double *tm = (const double *)d_tmodel;
    if (model) return recompute_launch(h, g, t, recompute_kernel(RC_MJVP, true), recompute_kernel(RC_MJVP, false), &ja, &tm);
    return recompute_launch(h, g, t, recompute_kernel(RC_JVP, true), recompute_kernel(RC_JVP, false), &ja, nullptr);
}

int ndp_step_jvp_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                        const void *d_X_lin, const void *d_U_lin, const void *d_act_lin, int n_tan,
                        const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf,
                        void *d_du0, void *d_dX, void *d_dU, void *d_u0_check, void *d_status_check, void *stream)
{
    return step_jvp(h, Tape{d_x0, d_xr, d_ur, d_f, d_X_lin, d_U_lin, d_act_lin, d_u0_check, d_status_check}, n_tan, d_tx0, d_txr, d_tur, d_tf,
                    d_du0, d_dX, d_dU, stream, false, nullptr);
}

int ndp_step_jvp_model_device(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, const void *d_f,
                              const void *d_X_lin, const void *d_U_lin, const void *d_act_lin, int n_tan,
                              const void *d_tx0, const void *d_txr, const void *d_tur, const void *d_tf, const void *d_tmodel,
                              void *d_du0, void *d_dX, void *d_dU, void *d_u0_check, void *d_status_check, void *stream)
{
    return step_jvp(h, Tape{d_x0, d_xr, d_ur, d_f, d_X_lin, d_U_lin, d_act_lin, d_u0_check, d_status_check}, n_tan, d_tx0, d_txr, d_tur, d_tf,
                    d_du0, d_dX, d_dU, stream, true, d_tmodel);
}

// ---- the model of a live handle: cost weights and mass
int ndp_set_model(ndp_handle *h, const double *Qd, const double *Rd, double mass)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    ndp_cfg c = h->cfg;
    const char *why = nullptr;
    if (Qd)
        for (int i = 0; i < 10; ++i) {
            if (!std::isfinite(Qd[i]) || Qd[i] < 0.0) why = "ndp_set_model: every Qd must be finite and >= 0";
            c.Qd[i] = Qd[i];
        }
    if (Rd)
        for (int i = 0; i < 4; ++i) {
            if (!std::isfinite(Rd[i]) || !(Rd[i] > 0.0)) why = "ndp_set_model: every Rd must be finite and > 0";
            c.Rd[i] = Rd[i];
        }
    if (std::isinf(mass)) why = "ndp_set_model: the mass must be finite (<= 0 or NaN: keep)";
    else if (mass > 0.0) c.mass = mass;
    if (!why && !as_gamma_holds(c, c.Rd))
        why = "ndp_set_model: as_gamma must be at least 1e8 * max(dt * Rd) when as_iter_max > 0 (ndp_create's rule: a weaker pin does not hold "
              "its input on the bound)";
    if (why) { h->err = why; return -2; }
    NDP_HIP(h, hipSetDevice(c.device));
    int rc = wait_all(h);                  // launches in flight read dKC; the copy below must not overtake them
    if (rc) return rc;
    // cfg, P (kernel arguments: the attitude weights, 1 / mass) and the constants table (KC_QD, KC_RD in LDS) change together; every
    // other reader of the mass (plant, actuator command, thrust estimator, reference flatness, BatchPtrs) takes it from cfg per call
    const RtiParams P = to_params(c);
    double kc[KC_HOST];
    fill_kc(P, kc);
    NDP_HIP(h, hipMemcpy(h->dKC, kc, sizeof(kc), hipMemcpyHostToDevice));
    h->cfg = c;
    h->P = P;
    return 0;
}
int ndp_refine_active(ndp_handle *h) { return h ? (int)(h->cfg.ipm_refine > 0 && slots_for(h->cfg.N) <= 3 && h->cfg.qp_precision == 0) : -1; }

int ndp_synchronize(ndp_handle *h)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    return wait_all(h);
}

int ndp_timing_enable(ndp_handle *h, int on)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    h->events.clear();
    h->timing = on > 0 ? on : 0;
    h->launch_no[0] = h->launch_no[1] = 0;
    return 0;
}

int ndp_timing_read(ndp_handle *h, const char *name, double *total_ms, int64_t *launches)
{
    if (!h || !name) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    const int kind = (name[0] == 'm') ? 1 : 0;
    double tot = 0.0;
    int64_t n = 0;
    for (auto &e : h->events) {
        if (e.kind != kind) continue;
        NDP_HIP(h, hipEventSynchronize(e.b));
        float ms = 0.0f;
        NDP_HIP(h, hipEventElapsedTime(&ms, e.a, e.b));
        tot += ms;
        ++n;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return n ? 0 : -10;
}

}  // extern "C"
