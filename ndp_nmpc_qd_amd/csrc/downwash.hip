// downwash.hip -- the downwash network's forward pass as launches of its own, and their entry points.
//   mlp_kernel  : DownwashNN.update + r_horiz gate for all (instance, horizon row) pairs.  The kernel, launch_mlp and mlp_prepare
//                 are in rti_kernels.hip (see there: it shares stage_fragments with the fused control step); its entry points are here.
//   mlp_stream_kernel + prefetch_gate_kernel / prefetch_done_kernel : the downwash of the NEXT tick on a second stream, LDS-free
//                 (weights out of L2), ordered against the control step by per-tile epochs (LateArgs / PF_* words).
//   plant_force_kernel : f4, the downwash force on the plant from the vehicles' actual states, one row per vehicle (ndp_plant_force*).
//   mlp_multi_kernel / plant_force_multi_kernel : the prediction and the plant force with K neighbours per vehicle, forces summed
//                 (ndp_downwash_multi*, ndp_plant_force_multi*).
// Host side: launch_plant_force launches either force kernel; plant_force_host / downwash_host: the host-array entries, single and multi.
// (The fused form runs inside the control step: rti_kernels.hip.  The backward pass: mlp_vjp.hip.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"
#include "mlp_common.hpp"
#include "mlp_tile.hpp"

namespace ndp {

// ---- LDS-free form of the tile (measurement: downwash of the NEXT tick in a second stream beside the control-step kernel, which
// holds all of a CU's LDS and 320 of its 512 registers per lane).  The weight records come straight from global memory (L2),
// NPRE records requested ahead; biases, first- and last-layer weights likewise.  Same arithmetic, same fragment blob.
typedef const float *__restrict__ g_cf32;
__device__ __forceinline__ void load_w_g(g_cf32 fr, int rec, int lane, Split2 &w)
{
    const h16x8 *p = reinterpret_cast<const h16x8 *>(fr + FR_HF) + rec * 128 + lane;
    w.hi = p[0]; w.lo = p[64];
}

__device__ __forceinline__ void mlp_tile_stream(g_cf32 fr, const float zb[3], int lane, float o[3])
{
    typedef float f4_t __attribute__((ext_vector_type(4)));
    constexpr int NPRE = 2;
    const int h = lane >> 5;
    Split2 wq[NPRE];
#pragma unroll
    for (int i = 0; i < NPRE; ++i) load_w_g(fr, i, lane, wq[i]);        // in flight under layer 1
    Split2 x1[4][2], x2[2][2];
    const f4_t *w4 = reinterpret_cast<const f4_t *>(fr + FR_W4);
    o[0] = o[1] = o[2] = 0.0f;
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
        f16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fr[FR_B1 + ot * 32 + f0(r) + 4 * h];
#pragma unroll
        for (int s = 0; s < 3; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[FR_L1 + (ot * 3 + s) * 64 + lane], zb[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = relu_cap(acc[r]);
        split2(acc, 0, x1[ot][0]);
        split2(acc, 1, x1[ot][1]);
        __builtin_amdgcn_sched_barrier(0);     // keep the phases apart: left alone the scheduler hoists every later load up front (254 registers)
    }
    f16_t acc, accl;
#pragma unroll
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const bool first = l2 ? (q % 8 == 0) : (q % 4 == 0), last = l2 ? (q % 8 == 7) : (q % 4 == 3);
        const Split2 wc = wq[rec % NPRE];
        if (rec + NPRE < 32) load_w_g(fr, rec + NPRE, lane, wq[rec % NPRE]);
        if (first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = fr[(l2 ? FR_B2 : FR_B3) + ot * 32 + f0(r) + 4 * h];
                accl[r] = 0.0f;
            }
        }
        mm3(wc, l2 ? x1[it][s] : x2[it][s], acc, accl);
        if (last) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = fmaf(accl[r], NDP_LO_INV, acc[r]);
                acc[r] = l2 ? relu_cap(v) : fmaxf(v, 0.0f);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (l2) { split2(acc, 0, x2[ot][0]); split2(acc, 1, x2[ot][1]); }
            else {      // last layer (128 -> 3) on this output tile at once: its 32 hidden features need not stay live
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const f4_t qv = w4[ot * 32 + f0(r) + 4 * h];
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = fmaf(qv[c], acc[r], o[c]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = o[c] + __shfl_xor(o[c], 32, 64) + fr[FR_B4 + c];
}

// one wave = one 32-row tile, four per workgroup, no LDS and no barrier, ~180 registers per lane (control step: 320 -- the two fit on
// a SIMD together; ensure_prefetch checks it).  proto != null: launch m of the prefetch protocol (see LateArgs).
__global__ __launch_bounds__(256)
void mlp_stream_kernel(const float *__restrict__ fr, const double *__restrict__ other, const double *__restrict__ ego,
                       const double *__restrict__ ego_xy, float *__restrict__ fout, float *__restrict__ fout1, int rows, int np1, double r2,
                       int other_stride, const int *__restrict__ other_index, unsigned long long *proto, int other_sys)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (rows + 31) / 32;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= ntiles) return;
    unsigned long long m = 0;
    if (proto) {
        m = proto[PF_CUR_M];                        // written by the gate launch in front of this one (plain load)
        if (m & 1) fout = fout1;
    }
    const int row = tile * 32 + j;
    const bool valid = row < rows;
    const int rowc = valid ? row : rows - 1;
    const int inst = rowc / np1, k = rowc - inst * np1;
    const int orow = other_index ? other_index[inst] : inst;
    const double *oth = other + (size_t)(orow < 0 ? 0 : orow) * np1 * other_stride;
    bool open = valid && orow >= 0;
    if (ego_xy) {
        const double oxy[2] = {ld_other(oth, other_sys), ld_other(oth + 1, other_sys)};
        open = open && gate_open(oxy, ego_xy + inst * 2, r2);
    }
    float zb[3], o[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        zb[s] = (float)(ld_other(oth + (size_t)k * other_stride + 2 * s + h, other_sys) - ego[(size_t)rowc * NX + 2 * s + h]);
    mlp_tile_stream(fr, zb, lane, o);
    if (!proto) {
        if (valid && h == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) fout[(size_t)row * 3 + c] = open ? o[c] : 0.0f;
        }
        return;
    }
    // the rows go out past this XCD's L2 (agent-scope stores: the reader runs on other XCDs, now), then -- once they are complete --
    // the tile's epoch word
    if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            __hip_atomic_store(reinterpret_cast<unsigned *>(fout) + (size_t)row * 3 + c, __float_as_uint(open ? o[c] : 0.0f),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The rows were written THROUGH to memory (sc1 stores): what is needed before the epoch word goes out is their COMPLETION, i.e.
    // s_waitcnt vmcnt(0) -- stores of one wave to different addresses / channels may complete out of order.  Not an agent-scope
    // release: its buffer_wbl2 writes back the XCD's whole L2, the control step's dirty iterate included (one per wave, 672 per
    // launch, made the control step beside it 50 % slower).  And not a workgroup-scope release fence alone: on gfx950 it emits NO
    // vmcnt wait (the ISA had the three row stores followed directly by the epoch store) -- the wait is spelled out;
    // the fence stays as the compiler-level barrier.  scripts/isa_audit.py checks the instruction is there.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0)
        __hip_atomic_store(proto + PF_EPOCH + (m & 1) * (unsigned)ntiles + tile, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- f4: the downwash force ON THE PLANT, one network row per vehicle (the closed-loop formation rollout's truth).  Vehicle v with
// o = other_index[v]: the network at (x[o] - x[v])[0:6] (fp64 difference rounded to fp32, as mlp_kernel forms (other - ego_ref)[0:6]),
// behind the r_horiz gate on |x[o].xy - x[v].xy| (gate_open: strict, the same individually rounded expression); f[v] = scale * (double)net
// in fp64 (what plant_kernel reads), exactly 0 when the gate is closed or there is no neighbour (other_index null, o < 0 -- or o >= B,
// which is never read); xy[v] = x[v][0:2], the dense ego-odometry buffer the fused control step takes.
// The tile is the LDS-free stream form (mlp_tile_stream): a batch is a few tiles at most (B / 32), so parking the 72-KB fragment image in
// LDS per workgroup would cost more than the tile itself; the weights come out of L2.  Its arithmetic is mlp_tile's, instruction for
// instruction, so the force is bit-equal to ndp_downwash_device's for the same six inputs.  One wave = 32 vehicles; a workgroup has
// blockDim.x / 64 waves (launch_plant_force: 1 to 4).  Control flow around the matrix instructions is wave-uniform: a wave leaves as a
// whole (its tile is past the batch, or none of its rows is open); the lanes past B in the last tile recompute vehicle B - 1 and store
// nothing.  It reads x only and writes f / xy only: every force is made from the states of one tick, so it is a launch of its own in
// front of the in-place plant_kernel.
__global__ __launch_bounds__(256)
void plant_force_kernel(const float *__restrict__ fr, const double *__restrict__ x, const int *__restrict__ other_index,
                        double *__restrict__ f, double *__restrict__ xy, int B, double r2, int gate, double scale)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int tile = (int)blockIdx.x * nw + wave;
    if (tile * 32 >= B) return;
    const int v = tile * 32 + j;
    const bool valid = v < B;
    const int vc = valid ? v : B - 1;
    const int o = other_index ? other_index[vc] : -1;
    const bool has = o >= 0 && o < B;
    const double *xe = x + (size_t)vc * NX, *xo = x + (size_t)(has ? o : vc) * NX;
    bool open = valid && has;
    if (gate) open = open && gate_open(xo, xe, r2);
    if (xy && valid && h == 1) { xy[(size_t)v * 2] = xe[0]; xy[(size_t)v * 2 + 1] = xe[1]; }
    float zb[3], out[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 3; ++s) zb[s] = (float)(xo[2 * s + h] - xe[2 * s + h]);
    if (__ballot(open) != 0ull) mlp_tile_stream(fr, zb, lane, out);      // (a 64-bit mask in scalar registers: the branch is the wave's)
    if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) f[(size_t)v * 3 + c] = open ? scale * (double)out[c] : 0.0;
    }
}

// ---- K neighbours per vehicle, forces superposed (a modelling assumption: the network was trained on pairs).  other_index is int32[B][K],
// 1 <= K <= NDP_MAX_NEIGH; a slot is one neighbour, gated on its own; slots are summed in slot order, the first open slot's value taken as
// it is, closed slots adding nothing.  Both kernels run the slots as a ROLLED loop around the tile: every weight load is then loop-invariant,
// and left alone the compiler hoists the weights out of the loop into registers (rti_kernels.hip: mlp_kernel; mlp_jvp.hip) -- the weights'
// base is made opaque at the head of every round.  A slot none of whose 32 rows is open is skipped as a whole (wave-uniform ballot).
struct MlpMultiArgs {
    const float *fr;
    const double *other, *ego, *ego_xy;     // other [rows][np1][other_stride], ego [B][np1][10], ego_xy [B][2] or null
    const int *other_index;                 // [B][K]
    float *fout;                            // [B][np1][3]
    int rows, np1, K, other_stride, other_sys;
    double r2;
};

// The controller's prediction: row (instance i, node n) = sum over the slots of what mlp_kernel gives for neighbour other_index[i][k], in
// fp32.  mlp_kernel's mapping (one wave per 32-row tile, four per workgroup) and its tile, mlp_tile, on the fragment image parked in LDS
// once per workgroup: the K slots reuse it, which is what one launch buys over K launches of mlp_kernel (K transfers) plus an add.
__global__ __launch_bounds__(256) void mlp_multi_kernel(MlpMultiArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (A.rows + 31) / 32;
    const int tile = (int)blockIdx.x * 4 + wave;
    stage_fragments(A.fr, (lds_f32)wsm, (int)threadIdx.x, 256);
    __syncthreads();
    if (tile >= ntiles) return;
    const int row = tile * 32 + j;
    const bool valid = row < A.rows;
    const int rowc = valid ? row : A.rows - 1;
    const int inst = rowc / A.np1, k = rowc - inst * A.np1;
    double e[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) e[s] = A.ego[(size_t)rowc * NX + 2 * s + h];
    float f[3] = {0.0f, 0.0f, 0.0f};
    bool any = false;
#pragma unroll 1
    for (int q = 0; q < A.K; ++q) {
        unsigned base = 0;
        asm volatile("" : "+s"(base));       // (the image is the same in every round: see above)
        lds_cf32 wl = (lds_cf32)wsm + base;
        const int orow = A.other_index[(size_t)inst * A.K + q];
        const double *oth = A.other + (size_t)(orow < 0 ? 0 : orow) * A.np1 * A.other_stride;
        bool open = valid && orow >= 0;
        if (A.ego_xy) {
            const double oxy[2] = {ld_other(oth, A.other_sys), ld_other(oth + 1, A.other_sys)};
            open = open && gate_open(oxy, A.ego_xy + (size_t)inst * 2, A.r2);
        }
        if (__ballot(open) == 0ull) continue;
        float zb[3], o[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) zb[s] = (float)(ld_other(oth + (size_t)k * A.other_stride + 2 * s + h, A.other_sys) - e[s]);
        mlp_tile(wl, zb, lane, o);
        if (open) {
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = any ? f[c] + o[c] : o[c];
            any = true;
        }
    }
    if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A.fout[(size_t)row * 3 + c] = f[c];
    }
}

// The force on the plant: plant_force_kernel with K slots per vehicle, f[v] = sum over the open slots of scale * (double)net(x[o_k] - x[v])
// in fp64 (products and sums individually rounded: the sum of K ndp_plant_force results, bit for bit).  A slot with o < 0 or o >= B
// contributes exactly 0 and is never read.  The same stream tile, launch shape and tail rule as plant_force_kernel.
__global__ __launch_bounds__(256)
void plant_force_multi_kernel(const float *__restrict__ fr, const double *__restrict__ x, const int *__restrict__ other_index, int K,
                              double *__restrict__ f, double *__restrict__ xy, int B, double r2, int gate, double scale)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int tile = (int)blockIdx.x * nw + wave;
    if (tile * 32 >= B) return;
    const int v = tile * 32 + j;
    const bool valid = v < B;
    const int vc = valid ? v : B - 1;
    const double *xe = x + (size_t)vc * NX;
    if (xy && valid && h == 1) { xy[(size_t)v * 2] = xe[0]; xy[(size_t)v * 2 + 1] = xe[1]; }
    double e[3], acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 3; ++s) e[s] = xe[2 * s + h];
    bool any = false;
#pragma unroll 1
    for (int q = 0; q < K; ++q) {
        unsigned base = 0;
        asm volatile("" : "+s"(base));       // (the weights are the same in every round: see above; an opaque OFFSET, so that fr stays a
        g_cf32 frq = fr + base;              // global-memory pointer -- an opaque pointer is a generic one, and its loads flat loads)
        const int o = other_index[(size_t)vc * K + q];
        const bool has = o >= 0 && o < B;
        const double *xo = x + (size_t)(has ? o : vc) * NX;
        bool open = valid && has;
        if (gate) open = open && gate_open(xo, xe, r2);
        if (__ballot(open) == 0ull) continue;
        float zb[3], out[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) zb[s] = (float)(xo[2 * s + h] - e[s]);
        mlp_tile_stream(frq, zb, lane, out);
        if (open) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = nc_mul(scale, (double)out[c]);
                acc[c] = any ? nc_add(acc[c], p) : p;
            }
            any = true;
        }
    }
    if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) f[(size_t)v * 3 + c] = acc[c];
    }
}

// One wave, in front of downwash launch m on the second stream: takes the number, waits until the control step that read force
// slot m & 1 last (number m - 2) holds its values, publishes the number for the launch behind it.  A single wave polling gently
// costs nothing (waves of the downwash kernel polling on every CU kept registers the next control-step workgroups needed).
__global__ void prefetch_gate_kernel(unsigned long long *proto, unsigned timeout_us, unsigned groups_rti)
{
    if (threadIdx.x != 0) return;
    const unsigned long long m = proto[PF_CUR_M] + 1;
    if (m > 2) {
        const unsigned long long want = (m - 2) * groups_rti;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(proto + PF_RTI_C2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
            __builtin_amdgcn_s_sleep(16);
            if (__builtin_amdgcn_s_memrealtime() - t0 > 100ull * timeout_us) {
                atomicAdd(reinterpret_cast<int *>(proto + PF_GATE_TIMEOUT), 1);
                break;
            }
        }
    }
    proto[PF_CUR_M] = m;
}

// behind downwash launch m in its stream: that launch is complete
__global__ void prefetch_done_kernel(unsigned long long *proto)
{
    if (threadIdx.x == 0) __hip_atomic_store(proto + PF_MLP_DONE, proto[PF_CUR_M], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace ndp

using namespace ndp;

// host: blob (W1 b1 W2 b2 W3 b3 W4 b4, row-major [out][in]) -> fragment order
static uint16_t f16_rn(float x)
{   // round-to-nearest-even f32 -> fp16 bits, subnormals included (the weights and their residuals are finite and small)
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t ax = u & 0x7FFFFFFFu;
    if (ax >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);               // >= 65536: inf (never for these data)
    if (ax < 0x33000000u) return sign;                                       // < 2^-25: 0
    const int e = (int)(ax >> 23) - 127;
    uint32_t m = (ax & 0x7FFFFFu) | 0x800000u;                               // 24-bit significand
    const int shift = e < -14 ? 13 + (-14 - e) : 13;                         // bits to drop (subnormal: more)
    const uint32_t keep = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t r = keep + ((rem > half || (rem == half && (keep & 1u))) ? 1u : 0u);
    // normal: r has the hidden bit at position 10; adding the exponent field lets a mantissa carry roll into it
    const uint32_t bits = e < -14 ? r : (uint32_t)((e + 15 - 1) << 10) + r;
    return (uint16_t)(sign | bits);
}
static float f16_f32(uint16_t b)
{
    const uint32_t sign = (uint32_t)(b & 0x8000u) << 16, ex = (b >> 10) & 0x1Fu, mant = b & 0x3FFu;
    float x;
    if (ex == 0) {
        x = (float)mant * 5.9604644775390625e-08f;                           // 2^-24
        uint32_t u; memcpy(&u, &x, 4); u |= sign; memcpy(&x, &u, 4);
        return x;
    }
    const uint32_t u = sign | ((ex + 112u) << 23) | (mant << 13);
    memcpy(&x, &u, 4);
    return x;
}

static void make_fragments(const float *blob, std::vector<float> &fr)
{
    const float *W1 = blob, *b1 = W1 + 128 * 6, *W2 = b1 + 128, *b2 = W2 + 64 * 128;
    const float *W3 = b2 + 64, *b3 = W3 + 128 * 64, *W4 = b3 + 128, *b4 = W4 + 3 * 128;
    fr.assign(FR_TOTAL, 0.0f);
    for (int ot = 0; ot < 4; ++ot)
        for (int s = 0; s < 3; ++s)
            for (int l = 0; l < 64; ++l) fr[FR_L1 + (ot * 3 + s) * 64 + l] = W1[(ot * 32 + (l & 31)) * 6 + 2 * s + (l >> 5)];
    for (int i = 0; i < 128; ++i) fr[FR_B1 + i] = b1[i];
    for (int i = 0; i < 64; ++i) fr[FR_B2 + i] = b2[i];
    for (int i = 0; i < 128; ++i) fr[FR_B3 + i] = b3[i];
    for (int f = 0; f < 128; ++f)
        for (int c = 0; c < 3; ++c) fr[FR_W4 + f * 4 + c] = W4[c * 128 + f];
    for (int i = 0; i < 3; ++i) fr[FR_B4 + i] = b4[i];
    // layers 2, 3: record = (out tile, in tile, k-step); lane (r = l&31, h = l>>5) element j holds
    // W[ot*32 + r][it*32 + 16 s + 8 (j>>2) + 4 h + (j&3)] split into hi + lo / 2^11
    uint16_t *hf = reinterpret_cast<uint16_t *>(fr.data() + FR_HF);
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const float *W = l2 ? W2 : W3;
        const int nin = l2 ? 128 : 64;
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int kin = it * 32 + 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3);
                const float w = W[(ot * 32 + (l & 31)) * nin + kin];
                const uint16_t hi = f16_rn(w);
                const float r1 = w - f16_f32(hi);
                const uint16_t lo = f16_rn(r1 * NDP_LO_SCALE);
                uint16_t *rp = hf + (size_t)rec * 2 * 512;
                rp[0 * 512 + l * 8 + j] = hi;
                rp[1 * 512 + l * 8 + j] = lo;
            }
    }
}

extern "C" {

int ndp_set_mlp_weights(ndp_handle *h, const float *blob, size_t n)
{
    if (!h || !blob) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (n != NDP_MLP_NPARAM) { h->err = "ndp_set_mlp_weights: expected 17859 floats"; return -2; }
    // refused before anything is touched (the weights installed before stay in force): a non-finite parameter, and a W2 / W3 entry
    // whose fp16 hi part would not be finite (layers 2 and 3 run on fp16 pairs: include/ndp_nmpc.h)
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(blob[i])) {
            h->err = "ndp_set_mlp_weights: parameter " + std::to_string(i) + " is not finite";
            return -2;
        }
    const size_t w2 = 128 * 6 + 128, w3 = w2 + 64 * 128 + 64;
    for (size_t i = 0; i < 64 * 128; ++i)
        if (std::fabs(blob[w2 + i]) >= NDP_MLP_W23_LIMIT || std::fabs(blob[w3 + i]) >= NDP_MLP_W23_LIMIT) {
            h->err = "ndp_set_mlp_weights: |W2|, |W3| must be below 65504 (layers 2 and 3 run on fp16 pairs); entry " + std::to_string(i) +
                     " of " + (std::fabs(blob[w2 + i]) >= NDP_MLP_W23_LIMIT ? "W2" : "W3") + " is not";
            return -2;
        }
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    std::vector<float> fr;
    make_fragments(blob, fr);
    std::vector<float> frt(FRT_TOTAL);
    make_fragments_t(blob, frt.data());          // the backward pass's records (mlp_vjp.hip)
    NDP_HIP(h, hipMemcpyAsync(h->dFrag, fr.data(), FR_TOTAL * 4, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipMemcpyAsync(h->dFragT, frt.data(), FRT_TOTAL * 4, hipMemcpyHostToDevice, h->stream));
    NDP_HIP(h, hipStreamSynchronize(h->stream));
    h->have_mlp = true;
    return 0;
}

// ---- downwash one tick ahead (second stream) + the control step that consumes it
static int ensure_prefetch(ndp_handle *h)
{
    if (h->aux) return 0;
    if (!h->cfg.use_fd) { h->err = "downwash prefetch needs use_fd = 1 (NDP model)"; return -8; }
    if (h->use_queue && !h->queue_auto) { h->err = "downwash prefetch is not combined with the interior-point work list (set cfg.work_queue = 2)"; return -16; }
    if (h->cfg.qp_precision) { h->err = "downwash prefetch serves the fp64 product path only"; return -12; }
    if (h->cfg.N + 1 > 32) { h->err = "downwash prefetch needs N + 1 <= 32 (an instance's rows in at most two 32-row tiles)"; return -12; }
    if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
    // (h->aux, created last, marks completion; members a failed earlier call did allocate are reused, not allocated again)
    for (int i = 0; i < 2; ++i) {
        NDP_HIP(h, h->dForceAB[i].ensure(nfs(h) * 4));
        NDP_HIP(h, hipMemset(h->dForceAB[i], 0, nfs(h) * 4));
    }
    h->pf_ntiles = (unsigned)((h->cfg.batch * (h->cfg.N + 1) + 31) / 32);
    const size_t proto_words = (size_t)PF_EPOCH + 2 * (size_t)h->pf_ntiles;
    NDP_HIP(h, h->dProto.ensure(proto_words * 8));
    NDP_HIP(h, hipMemset(h->dProto, 0, proto_words * 8));
    {
        const unsigned grid_rti = (unsigned)((h->cfg.batch + h->waves - 1) / h->waves);
        h->pf_groups_rti = grid_rti < PF_GROUPS ? grid_rti : PF_GROUPS;
    }
    // its own hardware queue: the downwash launch has to RUN beside the control step (a stream that shares the caller's hardware
    // queue would execute behind it).  Streams of another priority level get queues of their own.
    int lo = 0, hi = 0;
    NDP_HIP(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    NDP_HIP(h, h->evFork.ensure(hipEventDisableTiming));
    NDP_HIP(h, h->evJoin.ensure(hipEventDisableTiming));
    NDP_HIP(h, h->aux.ensure(hipStreamNonBlocking, hi));
    return 0;
}

int ndp_downwash_prefetch_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index,
                                 const void *d_ego_ref, const void *d_ego_xy, void *after_stream, void *on_stream)
{
    Entry g(h, d_other && d_ego_ref);
    if (g.rc) return g.rc;
    int rc = ensure_prefetch(h);
    if (rc) return rc;
    if (other_stride != 10 && other_stride != 6) { h->err = "ndp_downwash_prefetch_device: other_stride must be 10 or 6"; return -13; }
    hipStream_t a = on_stream ? (hipStream_t)on_stream : h->aux;
    if (after_stream) {      // the windows are produced on that stream (and, inside a capture, this is what brings the second stream in)
        NDP_HIP(h, hipEventRecord(h->evFork, (hipStream_t)after_stream));
        NDP_HIP(h, hipStreamWaitEvent(a, h->evFork, 0));
    }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int ntiles = (rows + 31) / 32;
    hipLaunchKernelGGL(prefetch_gate_kernel, dim3(1), dim3(64), 0, a, h->dProto, h->prefetch_timeout_us, h->pf_groups_rti);
    hipLaunchKernelGGL(mlp_stream_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, a, (const float *)h->dFrag, (const double *)d_other,
                       (const double *)d_ego_ref, (const double *)d_ego_xy, h->dForceAB[0], h->dForceAB[1], rows, np1,
                       h->cfg.r_horiz * h->cfg.r_horiz, other_stride, (const int *)d_other_index, h->dProto, peer_mapped(d_other));
    hipLaunchKernelGGL(prefetch_done_kernel, dim3(1), dim3(64), 0, a, h->dProto);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

int ndp_prefetch_join(ndp_handle *h, void *stream)
{
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->aux) return 0;
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    NDP_HIP(h, hipEventRecord(h->evJoin, h->aux));
    NDP_HIP(h, hipStreamWaitEvent(stream ? (hipStream_t)stream : h->stream, h->evJoin, 0));
    return 0;
}

int ndp_step_device_prefetched(ndp_handle *h, const void *d_x0, const void *d_xr, const void *d_ur, void *d_u0, void *stream)
{
    Entry g(h, d_x0 && d_xr && d_ur && d_u0, stream, "ndp_step_device_prefetched");
    if (g.rc) return g.rc;
    int rc = ensure_prefetch(h);
    if (rc) return rc;
    return g.noted(launch_rti(h, (const double *)d_x0, (const double *)d_xr, (const double *)d_ur, nullptr, (double *)d_u0, nullptr, g.s,
                              nullptr, nullptr, true));
}

int ndp_prefetch_stats(ndp_handle *h, unsigned long long *out4 /* [5] */)
{
    if (!h || !out4) return -1;
    std::lock_guard<std::mutex> lk(h->mu);
    out4[0] = out4[1] = out4[2] = out4[3] = out4[4] = 0;
    if (!h->aux) return 0;
    NDP_HIP(h, hipSetDevice(h->cfg.device));
    int rc = wait_all(h);
    if (rc) return rc;
    NDP_HIP(h, hipStreamSynchronize(h->aux));
    std::vector<unsigned long long> w(PF_EPOCH);
    NDP_HIP(h, hipMemcpy(w.data(), h->dProto, (size_t)PF_EPOCH * 8, hipMemcpyDeviceToHost));
    out4[0] = w[PF_CUR_M]; out4[1] = w[PF_RTI_C2] / h->pf_groups_rti;
    out4[2] = (unsigned)(w[PF_MISSED] & 0xffffffffu); out4[3] = (unsigned)(w[PF_GATE_TIMEOUT] & 0xffffffffu);
    out4[4] = (unsigned)(w[PF_SLOW] & 0xffffffffu);
    return 0;
}

void *ndp_device_force_slot(ndp_handle *h, int slot) { return h && (slot == 0 || slot == 1) ? h->dForceAB[slot] : nullptr; }

int ndp_downwash_device(ndp_handle *h, const void *d_other, const void *d_ego_ref, const void *d_ego_xy,
                        void *d_f_out, void *stream)
{
    Entry g(h, d_other && d_ego_ref && d_f_out, stream);
    if (g.rc) return g.rc;
    Neigh nb;
    nb.other = (const double *)d_other; nb.ego_xy = (const double *)d_ego_xy;
    return g.noted(launch_mlp(h, nb, (const double *)d_ego_ref, (float *)d_f_out, g.s));
}


// measurement hook: the LDS-free downwash kernel (see mlp_stream_kernel) on a caller's stream
int ndp_debug_downwash_stream_device(ndp_handle *h, const void *d_other, const void *d_ego_ref, const void *d_ego_xy,
                                     void *d_f_out, void *stream)
{
    Entry g(h, d_other && d_ego_ref && d_f_out, stream);
    if (g.rc) return g.rc;
    if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int ntiles = (rows + 31) / 32;
    hipLaunchKernelGGL(mlp_stream_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, g.s, (const float *)h->dFrag, (const double *)d_other,
                       (const double *)d_ego_ref, (const double *)d_ego_xy, (float *)d_f_out, (float *)d_f_out, rows, np1,
                       h->cfg.r_horiz * h->cfg.r_horiz, NX, (const int *)nullptr, (unsigned long long *)nullptr, peer_mapped(d_other));
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

// ---- f4: the downwash force on the plant, single form (K = 0, d_index int32[B]: plant_force_kernel) and K neighbours per vehicle (d_index
// int32[B][K]: plant_force_multi_kernel).  No locking, no sync, K not checked (check_neigh).  d_index null: nobody has a neighbour -- the
// single kernel with a null index writes the zeros, no network pass, no weights needed.
int launch_plant_force(ndp_handle *h, const double *d_x, const int *d_index, int K, int gate, double scale, double *d_f, double *d_xy,
                       hipStream_t s)
{
    if (d_index && !h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
    const int B = h->cfg.batch, ntiles = (B + 31) / 32;
    const int nw = ntiles < 4 ? ntiles : 4;          // waves per workgroup: no idle wave in a batch of up to 96 vehicles
    const dim3 grid((ntiles + nw - 1) / nw), block(64 * nw);
    const double r2 = h->cfg.r_horiz * h->cfg.r_horiz;
    if (d_index && K) hipLaunchKernelGGL(plant_force_multi_kernel, grid, block, 0, s, (const float *)h->dFrag, d_x, d_index, K, d_f, d_xy, B, r2, gate ? 1 : 0, scale);
    else hipLaunchKernelGGL(plant_force_kernel, grid, block, 0, s, (const float *)h->dFrag, d_x, d_index, d_f, d_xy, B, r2, gate ? 1 : 0, scale);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

// ---- K neighbours per vehicle (mlp_multi_kernel).  No locking, no sync.
// allow mlp_multi_kernel's dynamic-LDS launch (ndp_create)
hipError_t mlp_multi_prepare(void)
{
    return hipFuncSetAttribute((const void *)mlp_multi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(FR_TOTAL * sizeof(float)));
}

// -2 (nothing enqueued) unless 1 <= K <= NDP_MAX_NEIGH
int check_neigh(ndp_handle *h, const char *who, int K)
{
    if (K >= 1 && K <= NDP_MAX_NEIGH) return 0;
    h->err = std::string(who) + ": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle), got " + std::to_string(K);
    return -2;
}

int launch_mlp_multi(ndp_handle *h, const double *d_other, int other_stride, const int *d_index, int K, const double *d_ego,
                     const double *d_ego_xy, float *d_f, hipStream_t s)
{
    if (!h->have_mlp) { h->err = "downwash requested but ndp_set_mlp_weights was never called"; return -6; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int ntiles = (rows + 31) / 32;
    MlpMultiArgs a{h->dFrag, d_other, d_ego, d_ego_xy, d_index, d_f, rows, np1, K, other_stride, peer_mapped(d_other),
                   h->cfg.r_horiz * h->cfg.r_horiz};
    hipLaunchKernelGGL(mlp_multi_kernel, dim3((ntiles + 3) / 4), dim3(256), FR_TOTAL * sizeof(float), s, a);
    NDP_HIP(h, hipGetLastError());
    return 0;
}

// What a multi entry tries first, behind its frame: K (-2) IN FRONT OF the -1 of a missing argument (an index array of K = 0 may well be NULL).
// The single forms have no K and give their -1 in the frame.
static int neigh_args(ndp_handle *h, const char *who, int K, bool args)
{
    const int rc = check_neigh(h, who, K);
    return rc ? rc : args ? 0 : -1;
}

// ---- the device-pointer entries
int ndp_plant_force_device(ndp_handle *h, const void *d_x, const void *d_other_index, int gate, double scale, void *d_f, void *d_xy,
                           void *stream)
{
    Entry g(h, d_x && d_f, stream);
    if (g.rc) return g.rc;
    return g.noted(launch_plant_force(h, (const double *)d_x, (const int *)d_other_index, 0, gate, scale, (double *)d_f, (double *)d_xy, g.s));
}

int ndp_plant_force_multi_device(ndp_handle *h, const void *d_x, const void *d_other_index, int K, int gate, double scale, void *d_f,
                                 void *d_xy, void *stream)
{
    Entry g(h, true, stream);
    if (g.rc) return g.rc;
    const int rc = neigh_args(h, "ndp_plant_force_multi_device", K, d_x && d_f);
    if (rc) return rc;
    return g.noted(launch_plant_force(h, (const double *)d_x, (const int *)d_other_index, K, gate, scale, (double *)d_f, (double *)d_xy, g.s));
}

int ndp_downwash_multi_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, int K, const void *d_ego_ref,
                              const void *d_ego_xy, void *d_f_out, void *stream)
{
    Entry g(h, true, stream);
    if (g.rc) return g.rc;
    const int rc = neigh_args(h, "ndp_downwash_multi_device", K, d_other && d_other_index && d_ego_ref && d_f_out);
    if (rc) return rc;
    if (other_stride != 10 && other_stride != 6) { h->err = "ndp_downwash_multi_device: other_stride must be 10 or 6"; return -13; }
    return g.noted(launch_mlp_multi(h, (const double *)d_other, other_stride, (const int *)d_other_index, K, (const double *)d_ego_ref,
                                    (const double *)d_ego_xy, (float *)d_f_out, g.s));
}

// ---- the host-array entries, one body per single / multi pair (who: the multi entry's name, null: the single form, K not read).  What
// they stage in sThr (11 B doubles), written once:
//   the plant force   f fp64 [B][3] | index int32 [B][K]   3 B + K B / 2 doubles: 7 B at K = NDP_MAX_NEIGH = 8
//   the prediction    index int32 [B][K]                   K B / 2 doubles: 4 B at K = 8 (the force is h->dForce)
static int *sthr_force_index(const ndp_handle *h) { return reinterpret_cast<int *>(h->sThr + 3 * (size_t)h->cfg.batch); }
static int *sthr_index(const ndp_handle *h) { return reinterpret_cast<int *>(h->sThr.get()); }

static int plant_force_host(ndp_handle *h, const char *who, const double *x, const int32_t *other_index, int K, int gate, double scale, double *f)
{
    Entry g(h, who || (x && f));
    if (g.rc) return g.rc;
    int rc;
    if (who && (rc = neigh_args(h, who, K, x && f))) return rc;
    const size_t B = h->cfg.batch;
    hipStream_t s = h->stream;
    int *d_index = sthr_force_index(h);
    NDP_HIP(h, hipMemcpyAsync(h->sx0, x, B * NX * 8, hipMemcpyHostToDevice, s));
    if (other_index) NDP_HIP(h, hipMemcpyAsync(d_index, other_index, B * (who ? K : 1) * 4, hipMemcpyHostToDevice, s));
    if ((rc = launch_plant_force(h, h->sx0, other_index ? d_index : nullptr, who ? K : 0, gate, scale, h->sThr, nullptr, s))) return rc;
    NDP_HIP(h, hipMemcpyAsync(f, h->sThr, B * 3 * 8, hipMemcpyDeviceToHost, s));
    return g.synced(0);
}

int ndp_plant_force(ndp_handle *h, const double *x, const int32_t *other_index, int gate, double scale, double *f)
{
    return plant_force_host(h, nullptr, x, other_index, 0, gate, scale, f);
}

int ndp_plant_force_multi(ndp_handle *h, const double *x, const int32_t *other_index, int K, int gate, double scale, double *f)
{
    return plant_force_host(h, "ndp_plant_force_multi", x, other_index, K, gate, scale, f);
}

static int downwash_host(ndp_handle *h, const char *who, const double *other, const int32_t *other_index, int K, const double *ego_ref,
                         const double *ego_xy, float *f_out)
{
    Entry g(h, who || (other && ego_ref && f_out));
    if (g.rc) return g.rc;
    int rc;
    if (who && (rc = neigh_args(h, who, K, other && other_index && ego_ref && f_out))) return rc;      // (multi: the index is required)
    const size_t B = h->cfg.batch;
    hipStream_t s = h->stream;
    NDP_HIP(h, hipMemcpyAsync(h->sother, other, nxs(h) * 8, hipMemcpyHostToDevice, s));
    NDP_HIP(h, hipMemcpyAsync(h->sxr, ego_ref, nxs(h) * 8, hipMemcpyHostToDevice, s));
    if (who) NDP_HIP(h, hipMemcpyAsync(sthr_index(h), other_index, B * K * 4, hipMemcpyHostToDevice, s));
    if (ego_xy) NDP_HIP(h, hipMemcpyAsync(h->sego, ego_xy, B * 2 * 8, hipMemcpyHostToDevice, s));
    Neigh nb;
    nb.other = h->sother; nb.ego_xy = ego_xy ? h->sego : nullptr;
    if (who) rc = launch_mlp_multi(h, nb.other, NX, sthr_index(h), K, h->sxr, nb.ego_xy, h->dForce, s);
    else rc = launch_mlp(h, nb, h->sxr, h->dForce, s);
    if (rc) return rc;
    NDP_HIP(h, hipMemcpyAsync(f_out, h->dForce, nfs(h) * 4, hipMemcpyDeviceToHost, s));
    return g.synced(0);
}

int ndp_downwash(ndp_handle *h, const double *other, const double *ego_ref, const double *ego_xy, float *f_out)
{
    return downwash_host(h, nullptr, other, nullptr, 0, ego_ref, ego_xy, f_out);
}

int ndp_downwash_multi(ndp_handle *h, const double *other, const int32_t *other_index, int K, const double *ego_ref, const double *ego_xy,
                       float *f_out)
{
    return downwash_host(h, "ndp_downwash_multi", other, other_index, K, ego_ref, ego_xy, f_out);
}

}  // extern "C"
