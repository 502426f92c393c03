// exchange.hip -- the neighbour exchange between GPUs / processes: peer-mapped windows (peer_publish_kernel, peer_epoch_kernel) and the
// RCCL all-gather of the ranks' windows (pack_pv_kernel, pack_pv_list_kernel, ndp_xchg_*), with the remote tick that runs the exchange
// one control period ahead.
#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

#include "host.hpp"
#define NDP_PEER_FN __host__ __device__ inline
#include "peer_epoch.hpp"

namespace ndp {

// ------------------------------------------------------------------------------------------ peer windows: per-tick publish
// peer_epoch.hpp's protocol on the device.  TWO launches per control tick and rank, in front of the control-step launch:
//  peer_publish_kernel (<= 256 blocks)
//   thread 0 of block 0   : reader role -- acknowledge tick t-1 in the neighbour's header (its slot may be overwritten now)
//   thread 0 of each block: owner role  -- wait until the own slot t & 1 is free (the reader's acknowledgement of tick t-2)
//   all threads           : copy this tick's windows (src, the reference generator's output) into the own slot, plain stores;
//                           the end of the launch is what makes them visible system-wide
//  peer_epoch_kernel (one wave)
//   epoch[t & 1] := t (release, system scope), then -- reader role -- wait for the neighbour's epoch of tick t.  When this launch
//   has completed, the control-step kernel launched next on the same stream may read the neighbour's slot t & 1 (kernel
//   boundary = system-scope acquire).
// (One launch that counts its finished blocks with an atomic and lets the last one publish was the first form: agent-scope atomics
// on one address serialise at 30-60 ns each -- 8.7 us for 1.7 MB of windows against 4.7 us this way, 15-114 us against 7-9 us
// for 20 MB depending on the block count; scripts/ubench/publish_copy.hip.)
struct PeerDevMem {
    typedef unsigned long long u64;
    static __device__ __forceinline__ u64 load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM); }
    static __device__ __forceinline__ u64 peek(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
    static __device__ __forceinline__ void store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
    static __device__ __forceinline__ u64 now_us() { return __builtin_amdgcn_s_memrealtime() / 100; }   // 100 MHz constant clock
};

struct PeerPubArgs {
    const double *src;              // [n] doubles: this rank's windows of the tick
    unsigned long long *own;        // this rank's buffer (header + two slots)
    unsigned long long *nb;         // the neighbour rank's buffer, mapped (== own with one rank)
    size_t n;
    int slot;                       // the slot parity the host baked into the control-step launch that follows
    unsigned timeout_us;
};

// No LDS and no barrier: the launch may have to run BESIDE a control step whose workgroups hold the CU's whole LDS (the one-tick-ahead
// form), where a workgroup that asks for any would wait for a control-step workgroup to leave.  Every wave reads the tick and waits for the
// slot by itself (the same two words).
__global__ __launch_bounds__(256) void peer_publish_kernel(PeerPubArgs a)
{
    typedef PeerProto<PeerDevMem> PP;
    typedef unsigned long long u64;
    u64 t = 0;
    if ((threadIdx.x & 63u) == 0) {
        t = PP::next_tick(a.own);                    // (the epochs only change in peer_epoch_kernel, behind this launch)
        if (blockIdx.x == 0 && threadIdx.x == 0) PP::ack_previous(a.nb, t);
        const bool freed = PP::wait_slot_free(a.own, t, a.timeout_us);
        if (blockIdx.x == 0 && threadIdx.x == 0 && !freed) a.own[PEER_W_STAT + PEER_STAT_ACK_TIMEOUT] += 1;
    }
    const unsigned par = (unsigned)__builtin_amdgcn_readfirstlane((int)(t & 1));
    double2 *dst = reinterpret_cast<double2 *>(reinterpret_cast<unsigned char *>(a.own) + peer_slot_offset(a.n, (int)par));
    const double2 *src = reinterpret_cast<const double2 *>(a.src);
    const size_t n2 = a.n / 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
    if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<double *>(dst)[a.n - 1] = a.src[a.n - 1];
}

__global__ void peer_epoch_kernel(PeerPubArgs a)
{
    typedef PeerProto<PeerDevMem> PP;
    typedef unsigned long long u64;
    if (threadIdx.x != 0) return;
    const u64 t = PP::next_tick(a.own);
    PP::set_epoch(a.own, t);
    a.own[PEER_W_STAT + PEER_STAT_TICKS] = t;
    if ((int)(t & 1) != a.slot) a.own[PEER_W_STAT + PEER_STAT_DESYNC] += 1;
    if (!PP::wait_epoch(a.nb, t, a.timeout_us)) a.own[PEER_W_STAT + PEER_STAT_EPOCH_TIMEOUT] += 1;
}

// ------------------------------------------------------------------------------------------ RCCL exchange: the pack
// rows x [10] reference windows -> rows x [6]: the position / velocity columns, all that travels (downwash_nn.py:22).  One 16-byte
// piece per thread: piece p of row r = columns 2p, 2p + 1.
__global__ __launch_bounds__(256) void pack_pv_kernel(const double *__restrict__ xr, double *__restrict__ pv, size_t rows)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * 3) return;
    const size_t r = i / 3, p = i - r * 3;
    reinterpret_cast<double2 *>(pv)[i] = *reinterpret_cast<const double2 *>(xr + r * NX + 2 * p);
}

// the same for windows that lie in the reference list (ndp_tick): window row k of vehicle b = list row base + b * pitch + k * 10
__global__ __launch_bounds__(256) void pack_pv_list_kernel(const double *__restrict__ base, size_t pitch, int np1, double *__restrict__ pv, size_t B)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * (size_t)np1 * 3) return;
    const size_t r = i / 3, p = i - r * 3, b = r / (size_t)np1, k = r - b * (size_t)np1;
    reinterpret_cast<double2 *>(pv)[i] = *reinterpret_cast<const double2 *>(base + b * pitch + k * NX + 2 * p);
}

}  // namespace ndp

extern "C" {

// Address ranges this process mapped from other processes / GPUs (ndp_peer_open): neighbour windows inside one are read with
// system-scope loads (MlpArgs::other_sys).  A handful of entries, looked up once per launch.
struct PeerRange { uintptr_t lo, hi; };
static std::mutex g_peer_mu;
static std::vector<PeerRange> g_peer_ranges;
int peer_mapped(const void *p)
{
    if (!p) return 0;
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(g_peer_mu);
    for (const PeerRange &r : g_peer_ranges)
        if (a >= r.lo && a < r.hi) return 1;
    return 0;
}


// ------------------------------------------------------------------------------------------ peer windows (multi-GPU)
// The reference's neighbour exchange is publish / subscribe of the 21x10 float64 reference window (PredXU: nmpc_node.py:116-133
// publishes, ndp_nmpc_leader_node.py:40,60-76 subscribes).  One process per GPU: the publisher keeps its windows in a buffer
// whose IPC handle it hands to the subscriber's process once; the subscriber maps it and its control-step kernel reads the
// neighbour's window straight out of the publisher's HBM over xGMI (peer access) -- no per-step collective, no extra launch.
int ndp_peer_alloc(int device, size_t bytes, void **ptr, unsigned char *handle64)
{
    if (!ptr || !handle64 || bytes == 0) return -1;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "ndp_peer_*: the handle is passed as 64 bytes");
    if (hipSetDevice(device) != hipSuccess) return -2;
    // Fine-grained device memory: coherent between agents while kernels run (the epoch / acknowledgement words are polled by
    // running kernels of two GPUs, the slots are written here and read there one launch later).  Ordinary (coarse-grained)
    // memory if the runtime refuses, or when NDP_PEER_COARSE=1 asks for it; the protocol's accesses are system-scope either way.
    void *p = nullptr;
    const char *coarse = getenv("NDP_PEER_COARSE");
    if ((coarse && coarse[0] == '1') || hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) != hipSuccess || !p) {
        (void)hipGetLastError();
        p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return -3;
    }
    if (hipMemset(p, 0, bytes) != hipSuccess) { (void)hipFree(p); return -3; }      // epochs, acknowledgements, counters start at 0
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipFree(p); return -3; }
    hipIpcMemHandle_t hd;
    if (hipIpcGetMemHandle(&hd, p) != hipSuccess) { (void)hipFree(p); return -4; }
    memcpy(handle64, &hd, 64);
    *ptr = p;
    return 0;
}

int ndp_peer_open(int device, const unsigned char *handle64, void **ptr)
{
    if (!ptr || !handle64) return -1;
    if (hipSetDevice(device) != hipSuccess) return -2;
    hipIpcMemHandle_t hd;
    memcpy(&hd, handle64, 64);
    void *p = nullptr;
    if (hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); return -3; }
    {   // remember the mapped range: windows inside it are read with system-scope loads (see peer_mapped)
        void *base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, p) != hipSuccess || !base || size == 0) {
            (void)hipGetLastError();
            base = p; size = (size_t)1 << 40;       // extent unknown: err on the side of system-scope loads
        }
        std::lock_guard<std::mutex> lk(g_peer_mu);
        g_peer_ranges.push_back({(uintptr_t)base, (uintptr_t)base + size});
    }
    *ptr = p;
    return 0;
}

int ndp_peer_close(int device, void *ptr)
{
    if (!ptr) return -1;
    if (hipSetDevice(device) != hipSuccess) return -2;
    {
        std::lock_guard<std::mutex> lk(g_peer_mu);
        for (size_t i = 0; i < g_peer_ranges.size(); ++i)
            if ((uintptr_t)ptr >= g_peer_ranges[i].lo && (uintptr_t)ptr < g_peer_ranges[i].hi) { g_peer_ranges.erase(g_peer_ranges.begin() + i); break; }
    }
    return hipIpcCloseMemHandle(ptr) == hipSuccess ? 0 : -3;
}

int ndp_peer_free(int device, void *ptr)
{
    if (!ptr) return -1;
    if (hipSetDevice(device) != hipSuccess) return -2;
    return hipFree(ptr) == hipSuccess ? 0 : -3;
}


// ---- per-tick publish / subscribe through such buffers (peer_epoch.hpp)
int ndp_peer_layout(size_t n_doubles, size_t *buffer_bytes, size_t *slot0_offset, size_t *slot_stride)
{
    if (buffer_bytes) *buffer_bytes = peer_buffer_bytes(n_doubles);
    if (slot0_offset) *slot0_offset = peer_slot_offset(n_doubles, 0);
    if (slot_stride) *slot_stride = peer_slot_bytes(n_doubles);
    return 0;
}

int ndp_peer_publish_device(int device, const void *d_src, size_t n_doubles, void *own_buf, void *nb_buf, int slot,
                            unsigned timeout_us, void *stream)
{
    if (!d_src || !own_buf || !nb_buf || n_doubles == 0 || (slot & ~1)) return -1;
    if (hipSetDevice(device) != hipSuccess) return -2;
    PeerPubArgs a{(const double *)d_src, (unsigned long long *)own_buf, (unsigned long long *)nb_buf, n_doubles, slot, timeout_us};
    size_t blocks = (n_doubles / 2 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 256) blocks = 256;        // all resident at once: every block's first thread may wait on the reader
    hipLaunchKernelGGL(peer_publish_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(peer_epoch_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int ndp_track_steps(ndp_handle *h, int on)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    if (on)
        for (Event &e : h->stepDone) NDP_HIP(h, e.ensure(hipEventDisableTiming));
    h->track_steps = on != 0;
    return 0;
}

int ndp_last_step_event(ndp_handle *h, void **event)
{
    if (!h || !event) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->track_steps || h->step_seq == 0) { h->err = "ndp_last_step_event: no tracked step yet (ndp_track_steps first)"; return -14; }
    if (!h->last_step_tracked) {
        h->err = "ndp_last_step_event: the control step launched last carried no completion event (launched while tracking was off, or "
                 "through a path that does not mark one): ordering a gather behind an OLDER step's event could overwrite a buffer the "
                 "last step still reads";
        return -14;
    }
    *event = (void *)h->stepDone[h->step_seq & 3];
    return 0;
}

// ---- The north star's collective issued by the library itself: one RCCL all-gather per control tick of the ranks' position /
// velocity windows, on a HIP stream of its own beside the control-step kernel (ordered by events, no host wait).  RCCL is bound at
// run time (dlopen of the library the process already holds -- torch's -- or the system's): the C-ABI library carries no link-time
// dependency on it and every other entry point works without it.
namespace {
typedef struct { char internal[128]; } rccl_uid;
typedef int (*fn_uid)(rccl_uid *);
typedef int (*fn_init)(void **, int, rccl_uid, int);
typedef int (*fn_ag)(const void *, void *, size_t, int, void *, hipStream_t);
typedef int (*fn_destroy)(void *);
typedef const char *(*fn_errstr)(int);
struct RcclApi {
    void *lib = nullptr;
    fn_uid uid = nullptr; fn_init init = nullptr; fn_ag allgather = nullptr; fn_destroy destroy = nullptr; fn_errstr errstr = nullptr;
};
std::mutex g_rccl_mu;
RcclApi g_rccl;
int rccl_bind(const char *path)
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return 0;
    void *l = nullptr;
    if (path && path[0]) l = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!l) l = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!l) l = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!l) return -20;
    RcclApi a;
    a.lib = l;
    a.uid = (fn_uid)dlsym(l, "ncclGetUniqueId"); a.init = (fn_init)dlsym(l, "ncclCommInitRank");
    a.allgather = (fn_ag)dlsym(l, "ncclAllGather"); a.destroy = (fn_destroy)dlsym(l, "ncclCommDestroy");
    a.errstr = (fn_errstr)dlsym(l, "ncclGetErrorString");
    if (!a.uid || !a.init || !a.allgather || !a.destroy) { dlclose(l); return -21; }
    g_rccl = a;
    return 0;
}
}  // namespace

struct ndp_xchg {
    int device = 0, rank = 0, world = 1;
    void *comm = nullptr;
    Stream cs;                                // the exchange's own stream (another priority level: its own hardware queue); declared in
                                              // front of the events and the buffer: destroyed behind them
    Event evReady, evDone;
    DevBuf<double> send;                      // packed windows of this rank
    size_t send_doubles = 0;                  // its capacity
    // the remote tick with the exchange ahead of the control steps (ndp_xchg_tick_begin / _step): begins are numbered 1, 2, ...; begin n
    // lives in slot n % 3 (at most two are ahead of the steps, and step k consumes begin k) and fills whichever gather buffer the
    // caller names -- two buffers (begin i+1 behind step i) or three (begin i+2 behind step i: the gather then never waits for a step)
    Event evGather[3];                               // slot's gather is complete
    unsigned long long win_n[3] = {0, 0, 0};         // the list position its windows belong to
    const void *buf[3] = {nullptr, nullptr, nullptr};   // the gather buffer it fills
    struct Reader { const void *ptr = nullptr; unsigned seq = 0; hipStream_t stream = nullptr; unsigned age = 0; };
    Reader readers[4];                               // per gather buffer: the control step that read it last (seq: its tracked number, 0 = untracked)
    unsigned steps = 0;                              // control steps taken (step k consumes begin k)
    int ahead = 0;                                   // gathers begun and not yet stepped on (0 .. 2)
    // ndp_xchg_tick_async: the exchange stream's launches of a begin (wait, advance + columns, ncclAllGather, event record: ~15 us of
    // host time) are made by a thread of the exchange's own; the caller's begin only describes them (~2 us).  One host thread's
    // launches are what bounds the remote tick one period ahead; with two the device does.
    struct Job {
        bool adv = false;
        TickPre a{};                                  // adv: the advance (+ columns) launch
        const double *pack_base = nullptr;            // !adv: the columns of the window that is there
        size_t pack_pitch = 0, B = 0, rows = 0;
        int np1 = 0, p = 0;
        void *gathered = nullptr;
        hipEvent_t wait_ev = nullptr;
    };
    Job job[3];                                      // begin n's launches: job[n % 3]
    unsigned job_n[3] = {0, 0, 0};                   // ... and n itself
    std::atomic<unsigned> posted{0}, done{0};
    std::atomic<int> async_rc{0};
    std::atomic<bool> stop{false};
    std::thread worker;
    bool async = false;
    std::string err;
};

int ndp_xchg_destroy(ndp_xchg *x);

int ndp_xchg_unique_id(const char *rccl_path, unsigned char *id128)
{
    if (!id128) return -1;
    int rc = rccl_bind(rccl_path);
    if (rc) return rc;
    rccl_uid u;
    if (g_rccl.uid(&u) != 0) return -22;
    memcpy(id128, u.internal, 128);
    return 0;
}

int ndp_xchg_create(int device, int rank, int world, const unsigned char *id128, const char *rccl_path, ndp_xchg **out)
{
    if (!id128 || !out || world < 1 || rank < 0 || rank >= world) return -1;
    *out = nullptr;
    int rc = rccl_bind(rccl_path);
    if (rc) return rc;
    if (hipSetDevice(device) != hipSuccess) return -2;
    std::unique_ptr<ndp_xchg> x(new (std::nothrow) ndp_xchg);
    if (!x) return -4;
    x->device = device; x->rank = rank; x->world = world;
    rccl_uid u;
    memcpy(u.internal, id128, 128);
    if (g_rccl.init(&x->comm, world, u, rank) != 0) return -22;      // collective: every rank calls it
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || x->cs.ensure(hipStreamNonBlocking, hi) != hipSuccess ||
        x->evReady.ensure(hipEventDisableTiming) != hipSuccess || x->evDone.ensure(hipEventDisableTiming) != hipSuccess ||
        x->evGather[0].ensure(hipEventDisableTiming) != hipSuccess || x->evGather[1].ensure(hipEventDisableTiming) != hipSuccess ||
        x->evGather[2].ensure(hipEventDisableTiming) != hipSuccess) {
        (void)ndp_xchg_destroy(x.release());      // (releases whatever exists: communicator, stream, events)
        return -3;
    }
    *out = x.release();
    return 0;
}

// the send buffer holds `rows` rows of 6 doubles: grown behind whatever may still read the old one -- the exchange's thread's pending
// launches, the exchange's stream and `also` (the caller's stream when it carries the pack / gather, else null)
static hipError_t grow_send(ndp_xchg *x, size_t rows, hipStream_t also)
{
    if (x->send_doubles >= rows * 6) return hipSuccess;
    while (x->done.load(std::memory_order_acquire) != x->posted.load(std::memory_order_relaxed)) __builtin_ia32_pause();
    if (x->send) {
        (void)hipStreamSynchronize(x->cs);
        if (also) (void)hipStreamSynchronize(also);
    }
    x->send_doubles = 0;
    const hipError_t e = x->send.alloc(rows * 6 * sizeof(double));
    if (e == hipSuccess) x->send_doubles = rows * 6;
    return e;
}

// rows = B_local * (N + 1) windows rows of d_xr ([rows][10] doubles) -> d_gathered ([world * rows][6]); everything `after_stream`
// holds so far comes first (null: the windows are in place, no ordering needed), nothing waits on the host
int ndp_xchg_begin(ndp_xchg *x, const void *d_xr, size_t rows, void *d_gathered, void *after_stream, void *after_event)
{
    if (!x || !d_xr || !d_gathered || rows == 0) return -1;
    if (hipSetDevice(x->device) != hipSuccess) return -2;
    if (grow_send(x, rows, nullptr) != hipSuccess) return -3;
    // (every event operation is a packet the queue's command processor retires in order: ~3 us each on the stream that also
    // carries the control steps -- callers whose windows are in place already pass no stream)
    if (after_stream && (hipEventRecord(x->evReady, (hipStream_t)after_stream) != hipSuccess || hipStreamWaitEvent(x->cs, x->evReady, 0) != hipSuccess))
        return -3;
    if (after_event && hipStreamWaitEvent(x->cs, (hipEvent_t)after_event, 0) != hipSuccess) return -3;
    const size_t pieces = rows * 3;
    hipLaunchKernelGGL(pack_pv_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, x->cs, (const double *)d_xr, x->send, rows);
    if (hipGetLastError() != hipSuccess) return -3;
    const int r = g_rccl.allgather(x->send, d_gathered, rows * 6, /* ncclFloat64 */ 8, x->comm, x->cs);
    if (r != 0) { x->err = g_rccl.errstr ? g_rccl.errstr(r) : "ncclAllGather failed"; return -22; }
    return hipEventRecord(x->evDone, x->cs) == hipSuccess ? 0 : -3;
}

// `stream` waits (on the device) for the gather started last
int ndp_xchg_end(ndp_xchg *x, void *stream)
{
    if (!x) return -1;
    return hipStreamWaitEvent((hipStream_t)stream, x->evDone, 0) == hipSuccess ? 0 : -3;
}

// One call per control tick of the pipelined form: `stream` waits for the gather begun last (this tick's windows), then the NEXT tick's
// gather is begun behind the last reader of its buffer -- the completion event of the control step launched last for h when the steps
// are tracked (ndp_track_steps), else everything `stream` holds so far.
int ndp_xchg_tick(ndp_xchg *x, ndp_handle *h, void *stream, const void *d_xr_next, size_t rows, void *d_gathered_next)
{
    void *ev = nullptr;
    if (h) {
        std::lock_guard<std::mutex> lk(h->mu);
        if (h->sens_level) return sens_refuse(h, "ndp_xchg_tick");
        if (h->track_steps && h->step_seq && h->last_step_tracked) ev = (void *)h->stepDone[h->step_seq & 3];
    }
    int rc = ndp_xchg_end(x, stream);
    if (rc) return rc;
    return ndp_xchg_begin(x, d_xr_next, rows, d_gathered_next, ev ? nullptr : stream, ev);
}

const char *ndp_xchg_last_error(const ndp_xchg *x) { return x ? x->err.c_str() : "null exchange"; }

static void xchg_worker_stop(ndp_xchg *x)
{
    if (x->worker.joinable()) {
        x->stop.store(true, std::memory_order_release);
        x->worker.join();
        x->stop.store(false, std::memory_order_release);
    }
    x->async = false;
}

int ndp_xchg_destroy(ndp_xchg *x)
{
    if (!x) return -1;
    xchg_worker_stop(x);
    (void)hipSetDevice(x->device);
    if (x->cs) (void)hipStreamSynchronize(x->cs);
    if (x->comm) (void)g_rccl.destroy(x->comm);
    delete x;
    return 0;
}

int ndp_peer_stats(int device, const void *own_buf, unsigned long long *out4)
{
    if (!own_buf || !out4) return -1;
    if (hipSetDevice(device) != hipSuccess) return -2;
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    return hipMemcpy(out4, (const unsigned long long *)own_buf + PEER_W_STAT, PEER_STAT_N * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

// pack_pv_list_kernel: the position / velocity columns of B windows in the list (window b's row k at base + b * pitch + k * 10)
void launch_pack_pv_list(const double *base, size_t pitch, int np1, double *pv, size_t B, hipStream_t s)
{
    const size_t n = B * (size_t)np1 * 3;
    hipLaunchKernelGGL(pack_pv_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, base, pitch, np1, pv, B);
}

// Stage 2 and the exchange in one call, on the tick's own stream: this tick's window columns packed out of the list into the
// exchange's send buffer, then ncclAllGather into d_gathered ([world * B][N+1][6]) -- both on `stream`, behind the list advance and in
// front of ndp_tick_step_device by stream order alone (no event operation, no second stream: the tick's chain is serial anyway).
int ndp_xchg_tick_windows(ndp_xchg *x, ndp_handle *h, void *d_gathered, void *stream)
{
    Entry g(h, x && d_gathered, stream, "ndp_xchg_tick_windows");
    if (g.rc) return g.rc;
    if (x->device != h->cfg.device) { h->err = "ndp_xchg_tick_windows: the exchange and the handle live on different devices"; return -1; }
    hipStream_t s = g.s;
    if (!h->dRingX) { h->err = "ndp_xchg_tick_windows: no reference list"; return -11; }
    const RingGeom rg = ring_geom(h);
    const size_t B = h->cfg.batch, rows = B * (size_t)(h->cfg.N + 1);
    NDP_HIP(h, grow_send(x, rows, s));
    launch_pack_pv_list(h->dRingX + rg.slot(h->list_n) * 10, rg.px(), h->cfg.N + 1, x->send, B, s);
    NDP_HIP(h, hipGetLastError());
    const int r = g_rccl.allgather(x->send, d_gathered, rows * 6, /* ncclFloat64 */ 8, x->comm, s);
    if (r != 0) { x->err = g_rccl.errstr ? g_rccl.errstr(r) : "ncclAllGather failed"; h->err = "ndp_xchg_tick_windows: " + x->err; return -22; }
    return g.noted(0);
}

// ---- the remote tick with the exchange ONE CONTROL PERIOD AHEAD.  A vehicle's window is a function of time alone (the list advance
// reads the trajectory, not the odometry): the list advance of tick i+1, its window columns and their all-gather run on the exchange's
// own stream BESIDE the control step of tick i, into the other one of two gather buffers.  Per control period
//     ndp_xchg_tick_step(tick i: estimator, wait for gather i on the device, control step)   then   ndp_xchg_tick_begin(tick i+1)
// (one begin in front of the first step).  What orders what:
//   gather i+1 writes the buffer step i-1 read      -> the exchange stream waits for that step's completion event (ndp_track_steps: it
//                                                      rides on the step's dispatch packet; untracked: for everything its stream holds)
//   advance i+1 writes list entries                  -> of another phase row than window i's (RingGeom: entries per node spacing >= 2,
//                                                      refused otherwise), so it may run beside step i
//   step i reads window i and gather buffer i        -> its stream waits for its begin's event, recorded behind advance i, pack, gather
//   the estimator reads the thrust step i-1 commanded -> same stream as the steps, in front of step i
// the exchange stream's launches of one begin; returns 0 or the error code (the caller's thread or the exchange's own)
static int xchg_job_run(ndp_xchg *x, const ndp_xchg::Job &j)
{
    if (j.wait_ev && hipStreamWaitEvent(x->cs, j.wait_ev, 0) != hipSuccess) return -3;
    if (j.adv) launch_tick_pre(j.a, x->cs);
    else launch_pack_pv_list(j.pack_base, j.pack_pitch, j.np1, x->send, j.B, x->cs);
    if (hipGetLastError() != hipSuccess) return -3;
    const int r = g_rccl.allgather(x->send, j.gathered, j.rows * 6, /* ncclFloat64 */ 8, x->comm, x->cs);
    if (r != 0) { x->err = g_rccl.errstr ? g_rccl.errstr(r) : "ncclAllGather failed"; return -22; }
    return hipEventRecord(x->evGather[j.p], x->cs) == hipSuccess ? 0 : -3;
}

static void xchg_worker(ndp_xchg *x)
{
    (void)hipSetDevice(x->device);
    int idle = 0;
    for (;;) {
        const unsigned want = x->done.load(std::memory_order_relaxed) + 1;
        if ((int)(x->posted.load(std::memory_order_acquire) - want) >= 0) {
            const int rc = xchg_job_run(x, x->job[want % 3]);
            if (rc) x->async_rc.store(rc, std::memory_order_relaxed);
            x->done.store(want, std::memory_order_release);
            idle = 0;
        } else if (x->stop.load(std::memory_order_acquire)) break;
        else if (++idle < 200000) __builtin_ia32_pause();                     // (~ a millisecond of spinning behind the last job, then naps)
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// on: begins are described by the caller and LAUNCHED by a thread of the exchange's own (see ndp_xchg::Job); off: launched by the caller
int ndp_xchg_tick_async(ndp_xchg *x, int on)
{
    if (!x) return -1;
    if (x->ahead != 0) { x->err = "ndp_xchg_tick_async: gathers are ahead of the control steps (step on them first)"; return -14; }
    if (on && !x->worker.joinable()) {
        x->stop.store(false);
        try { x->worker = std::thread(xchg_worker, x); } catch (...) { x->err = "ndp_xchg_tick_async: no thread"; return -4; }
        x->async = true;
    } else if (!on) xchg_worker_stop(x);
    return 0;
}

int ndp_xchg_tick_begin(ndp_xchg *x, ndp_handle *h, const void *d_t, int flags, void *d_gathered)
{
    Entry g(h, x && d_gathered, nullptr, "ndp_xchg_tick_begin");
    if (g.rc) return g.rc;
    if (x->device != h->cfg.device) { h->err = "ndp_xchg_tick_begin: the exchange and the handle live on different devices"; return -1; }
    int rc = ensure_tick(h);
    if (rc) return rc;
    if (!h->dRingX) { h->err = "ndp_xchg_tick_begin: no reference list"; return -11; }
    if (d_t && !h->dTraj) { h->err = "ndp_xchg_tick_begin: a trajectory time was given but ndp_ref_set_trajectory was never called"; return -11; }
    if (x->ahead >= 2) { h->err = "ndp_xchg_tick_begin: two gathers are already ahead of the control steps (ndp_xchg_tick_step first)"; return -14; }
    if ((rc = x->async_rc.load(std::memory_order_relaxed))) { h->err = "ndp_xchg_tick_begin: an earlier begin failed on the exchange's thread: " + x->err; return rc; }
    const RingGeom rg = ring_geom(h);
    if (d_t && rg.step < 2) { h->err = "ndp_xchg_tick_begin: the list's entries are one node spacing apart -- the advance would overwrite the window a control step may be reading (use the serial form: ndp_tick_advance_device, ndp_xchg_tick_windows, ndp_tick_step_device)"; return -17; }
    // a second begin ahead writes list entry n + step N + 2 while the step on window n (entries n, n + step, ..., n + step N) may still
    // run: with step 2 that entry lands in the same residue class as the window, i.e. on one of its nodes (RingGeom::slot)
    if (d_t && x->ahead == 1 && rg.step < 3) { h->err = "ndp_xchg_tick_begin: the list's entries are two per node spacing -- a second begin ahead would overwrite the window the step before it may be reading (one begin ahead only: the two-buffer form)"; return -17; }
    const size_t B = h->cfg.batch, rows = B * (size_t)(h->cfg.N + 1);
    NDP_HIP(h, grow_send(x, rows, nullptr));
    const unsigned n_job = x->posted.load(std::memory_order_relaxed) + 1;
    const int p = (int)(n_job % 3u);
    ndp_xchg::Job &j = x->job[p];                  // (free: at most two are ahead, and a step waits for its begin's launches)
    j = ndp_xchg::Job{};
    j.p = p; j.B = B; j.rows = rows; j.np1 = h->cfg.N + 1; j.gathered = d_gathered;
    // the gather overwrites a buffer: behind the control step that read it last
    const ndp_xchg::Reader *rd = nullptr;
    for (const ndp_xchg::Reader &r : x->readers) if (r.ptr == d_gathered) rd = &r;
    for (int q = 0; q < 3; ++q)                    // (a begin that is still ahead of its step names the same buffer: the caller cycles too few)
        if (x->buf[q] == d_gathered && (int)(x->job_n[q] - x->steps) > 0) { h->err = "ndp_xchg_tick_begin: this gather buffer holds a tick that has not been stepped on yet"; return -14; }
    if (rd) {
        const bool precise = h->track_steps && rd->seq && h->step_seq - rd->seq < 4u;
        if (precise) {
            j.wait_ev = h->stepDone[rd->seq & 3];
        } else {
            NDP_HIP(h, hipEventRecord(x->evReady, rd->stream));
            j.wait_ev = x->evReady;
        }
    } else if (n_job == 1) {            // the first gather: behind whatever made the list (ndp_ref_list_reset / ndp_tick_reset on the handle's stream)
        NDP_HIP(h, hipEventRecord(x->evReady, h->stream));
        j.wait_ev = x->evReady;
    }
    if (d_t) {
        const bool uni = (flags & TICK_T_UNIFORM) != 0;
        // (no estimator here: it belongs to the step's side) ... and the advanced window's columns in the same launch
        j.a = tick_pre(h, true, uni ? nullptr : (const double *)d_t, uni ? *(const double *)d_t : 0.0, false, nullptr, h->dTickThrust,
                       nullptr, x->send);
        j.adv = true;
        ++h->list_n;
    } else {
        j.pack_base = h->dRingX + rg.slot(h->list_n) * 10; j.pack_pitch = rg.px();
    }
    x->job_n[p] = n_job;
    x->buf[p] = d_gathered;
    if (x->async) x->posted.store(n_job, std::memory_order_release);          // the exchange's thread takes it from here
    else {
        rc = xchg_job_run(x, j);
        x->posted.store(n_job, std::memory_order_relaxed);
        x->done.store(n_job, std::memory_order_relaxed);
        if (rc) { h->err = "ndp_xchg_tick_begin: " + (rc == -22 ? x->err : std::string("a HIP call on the exchange's stream failed")); return rc; }
    }
    x->win_n[p] = h->list_n;
    ++x->ahead;
    return 0;
}

int ndp_xchg_tick_step(ndp_xchg *x, ndp_handle *h, const void *d_x_odom, const void *d_vz, const void *d_throttle, int flags,
                       void *d_cmd, void *d_u0, const void *d_gathered, void *stream)
{
    Entry g(h, x && d_x_odom && d_cmd && d_gathered, stream, "ndp_xchg_tick_step");
    if (g.rc) return g.rc;
    hipStream_t s = g.s;
    if (x->ahead < 1) { h->err = "ndp_xchg_tick_step: no gather was begun for this tick (ndp_xchg_tick_begin first)"; return -14; }
    int rc = ensure_tick(h);
    if (rc) return rc;
    const size_t B = h->cfg.batch;
    const unsigned k = x->steps + 1;               // this step consumes begin k
    const int p = (int)(k % 3u);
    if (x->buf[p] != d_gathered || x->job_n[p] != k) { h->err = "ndp_xchg_tick_step: this tick's gather was begun into another buffer"; return -14; }
    if (flags & TICK_ESTIMATE) {
        const TickPre a = tick_pre(h, false, nullptr, 0.0, true, (const double *)d_x_odom, (const double *)d_vz, (const double *)d_throttle);
        launch_tick_pre(a, s);
        NDP_HIP(h, hipGetLastError());
    }
    // (asynchronous begins: the event must have been RECORDED by the exchange's thread before this stream is told to wait for it)
    while ((int)(x->done.load(std::memory_order_acquire) - k) < 0) __builtin_ia32_pause();
    if ((rc = x->async_rc.load(std::memory_order_relaxed))) { h->err = "ndp_xchg_tick_step: this tick's begin failed on the exchange's thread: " + x->err; return rc; }
    NDP_HIP(h, hipStreamWaitEvent(s, x->evGather[p], 0));
    rc = tick_step_enqueue(h, s, (const double *)d_x_odom, (double *)d_cmd, (double *)d_u0, (const double *)d_gathered, x->win_n[p]);
    if (rc) return rc;
    ndp_xchg::Reader *slot = nullptr;              // this buffer's entry, else the one not touched for longest
    for (ndp_xchg::Reader &r : x->readers) if (r.ptr == d_gathered) slot = &r;
    if (!slot) { slot = &x->readers[0]; for (ndp_xchg::Reader &r : x->readers) if (r.age < slot->age) slot = &r; }
    slot->ptr = d_gathered; slot->stream = s; slot->age = k;
    slot->seq = (h->track_steps && h->last_step_tracked) ? h->step_seq : 0u;
    x->steps = k;
    --x->ahead;
    if (slot->seq) { h->track_pending = true; return 0; }     // (the getters wait for the step's own completion event: no second one)
    return g.noted(0);
}

}  // extern "C"
