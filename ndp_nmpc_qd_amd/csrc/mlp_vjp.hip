// mlp_vjp.hip -- the backward pass of the downwash network (nn_net.py:7-18, 6-128-64-128-3) and its weights set from device memory.
//
// Kernels
//   mlp_vjp_kernel        : per 32-row tile and wave (the row -> (instance, node) mapping, gate and addressing of mlp_kernel): the
//                           forward recomputed with mlp_tile's arithmetic (its ReLU masks are the forward's own), then
//                             data path    d4 = gf, d3 = (W4' d4) m3 on the VALU, d2 = (W3' d3) m2 and d1 = (W2' d2) m1 with
//                                          v_mfma_f32_32x32x2_f32 over transposed fp32 records (dFragT), g_z = W1' d1 on the VALU;
//                             weight path  dW_l = sum over rows d_l (x) a_(l-1): a contraction over ROWS, which sit on lanes -- the four
//                                          waves park d_l and a_(l-1) of their tiles in LDS as [feature][row] and every wave contracts
//                                          its share of dW_l's 32x32 tiles over the workgroup's 128 rows, in registers across the
//                                          grid-stride loop; biases by a column sum out of the same LDS image.
//                           All products are exact fp32 (the accuracy bar of the gradient decides, not speed).  Per-workgroup partial
//                           gradients go to a workspace of the handle, no atomics.
//   mlp_vjp_multi_kernel  : the same body (mlp_vjp_body.inc) over virtual rows, K neighbour slots per instance, one upstream row per instance.
//   mlp_vjp_reduce_kernel : sums the partials in a fixed order into the caller's buffer (two calls are bit-identical).
//   mlp_frag_kernel       : builds dFrag and dFragT from a blob in device memory (ndp_set_mlp_weights_device), bit for bit what
//                           make_fragments / make_fragments_t build on the host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"
#include "mlp_common.hpp"

namespace ndp {

typedef __attribute__((address_space(3))) float *lds_f32;
typedef const __attribute__((address_space(3))) float *lds_cf32;

// blob order of ndp_set_mlp_weights: W1[128][6] b1 W2[64][128] b2 W3[128][64] b3 W4[3][128] b4
enum { PW1 = 0, PB1 = PW1 + 128 * 6, PW2 = PB1 + 128, PB2 = PW2 + 64 * 128, PW3 = PB2 + 64, PB3 = PW3 + 128 * 64, PW4 = PB3 + 128,
       PB4 = PW4 + 3 * 128, PTOTAL = PB4 + 3 };
static_assert(PTOTAL == NDP_MLP_NPARAM, "blob layout");

// dFragT: the A operands of the backward data path, one 64-lane fp32 record per v_mfma_f32_32x32x2_f32.
//   FRT_L3 + ((it * 4 + st) * 16 + r) * 64 + l = W3[st*32 + f0(r) + 4 (l>>5)][it*32 + (l&31)]   d2 tile it  <-  d3 tile st, register r
//   FRT_L2 + ((it * 2 + st) * 16 + r) * 64 + l = W2[st*32 + f0(r) + 4 (l>>5)][it*32 + (l&31)]   d1 tile it  <-  d2 tile st, register r
// (register r of a 32x32 accumulator holds the feature pair {f0(r), f0(r) + 4} of the two half-waves: the K = 2 of one instruction.)
enum { FRT_L3 = 0, FRT_L2 = 128 * 64 };
static_assert(FRT_L2 + 128 * 64 == FRT_TOTAL, "dFragT size");

// index into the blob of the weight that float i of dFragT holds (ndp_nmpc_qd_amd/mlp_frag.py restates it for the tests)
__host__ __device__ inline int fragt_source(int i)
{
    const bool l3 = i < FRT_L2;
    const int q = l3 ? i : i - FRT_L2;
    const int l = q & 63, r = (q >> 6) & 15, t = q >> 10;            // t = it * nst + st
    const int it = l3 ? t >> 2 : t >> 1, st = l3 ? t & 3 : t & 1;
    const int out = st * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), in = it * 32 + (l & 31);
    return l3 ? PW3 + out * 64 + in : PW2 + out * 128 + in;
}

// the 32-bit word i of dFrag (make_fragments in downwash.hip is the definition; this is the same map read per word)
__device__ inline unsigned frag_word(const float *__restrict__ blob, int i)
{
    using namespace frag;
    float v = 0.0f;
    if (i < B1) {
        const int rec = i >> 6, l = i & 63, ot = rec / 3, s = rec - ot * 3;
        v = blob[PW1 + (ot * 32 + (l & 31)) * 6 + 2 * s + (l >> 5)];
    } else if (i < B2) v = blob[PB1 + i - B1];
    else if (i < B3) v = blob[PB2 + i - B2];
    else if (i < W4) v = blob[PB3 + i - B3];
    else if (i < B4) {
        const int f = (i - W4) >> 2, c = (i - W4) & 3;
        v = c < 3 ? blob[PW4 + c * 128 + f] : 0.0f;
    } else if (i < HF) v = i - B4 < 3 ? blob[PB4 + i - B4] : 0.0f;
    else if (i < USED) {
        unsigned w = 0;
#pragma unroll
        for (int e2 = 0; e2 < 2; ++e2) {
            const int e = 2 * (i - HF) + e2;                  // 16-bit element of the fp16 region
            const int rec = e >> 10, split = (e >> 9) & 1, l = (e >> 3) & 63, j = e & 7;
            const bool l2 = rec < 16;
            const int q = l2 ? rec : rec - 16;
            const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
            const int kin = it * 32 + 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3);
            const float x = l2 ? blob[PW2 + (ot * 32 + (l & 31)) * 128 + kin] : blob[PW3 + (ot * 32 + (l & 31)) * 64 + kin];
            const _Float16 hi = (_Float16)x;                  // round to nearest even, as f16_rn
            const _Float16 lo = (_Float16)((x - (float)hi) * NDP_LO_SCALE);
            const _Float16 pick = split ? lo : hi;
            unsigned short bits;
            __builtin_memcpy(&bits, &pick, 2);
            w |= (unsigned)bits << (16 * e2);
        }
        return w;
    }
    return __float_as_uint(v);
}

__global__ __launch_bounds__(256) void mlp_frag_kernel(const float *__restrict__ blob, unsigned *__restrict__ fr, float *__restrict__ frt)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < frag::TOTAL) fr[i] = frag_word(blob, i);
    if (i < FRT_TOTAL) frt[i] = blob[fragt_source(i)];
}

// ---------------------------------------------------------------------------------------------------------------- the backward pass
// LDS image of the weight path: per wave 192 feature rows (d_l first, a_(l-1) behind it) of 32 rows each, feature pitch 33 floats (the
// operand reads walk features across lanes: pitch 32 would put all of them on one bank)
enum { VJ_PITCH = 33, VJ_WAVE = 192 * VJ_PITCH, VJ_FLAGS = 4 * VJ_WAVE, VJ_LDS_FLOATS = VJ_FLAGS + 4 };

struct MlpVjpArgs {
    const float *fr, *frt;
    const double *other, *ego, *ego_xy, *gf;
    double *gz;             // [rows][6] or null
    float *part;            // [gridDim.x][NDP_MLP_NPARAM] or null (no weight gradient asked for)
    int rows, np1;
    double r2;
    int other_stride;
    const int *other_index;
    int other_sys;
    size_t other_pitch, ego_pitch, ego_xy_pitch;
};

// The weights come from global memory in fully unrolled loops; left alone the compiler requests hundreds of records ahead and spills the
// accumulators.  A compiler-only memory fence (no instruction) between groups of 16 bounds what is in flight.
#define VJP_FENCE() asm volatile("" ::: "memory")

__device__ __forceinline__ void load_w_vjp(const float *fr, int rec, int lane, Split2 &w)
{
    const h16x8 *p = reinterpret_cast<const h16x8 *>(fr + frag::HF) + rec * 128 + lane;
    w.hi = p[0]; w.lo = p[64];
}

// one 32-feature tile of the first layer's activations (mlp_tile's layer 1)
__device__ __forceinline__ f16_t vjp_layer1(const float *fr, const float zb[3], int lane, int ot)
{
    f16_t acc;
    VJP_FENCE();
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fr[frag::B1 + ot * 32 + f0(r) + 4 * (lane >> 5)];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[frag::L1 + (ot * 3 + s) * 64 + lane], zb[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = relu_cap(acc[r]);
    return acc;
}

// mlp_tile's forward (mlp_tile.hpp) with the weights read from global memory, keeping the activations: the same matrix instructions in the
// same order on the same operands, so the activations -- and with them the ReLU masks -- are those of the force the step used.  a1 is
// not kept (64 registers for the whole backward pass): vjp_layer1 computes it again where the second layer's gradient needs it.
__device__ __forceinline__ void vjp_forward(const float *fr, const float zb[3], int lane, f16_t a2[2], f16_t a3[4])
{
    const int h = lane >> 5;
    Split2 x1[4][2], x2[2][2];
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
        const f16_t acc = vjp_layer1(fr, zb, lane, ot);
        split2(acc, 0, x1[ot][0]);
        split2(acc, 1, x1[ot][1]);
    }
    f16_t acc, accl;
#pragma unroll
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const bool first = l2 ? (q % 8 == 0) : (q % 4 == 0), last = l2 ? (q % 8 == 7) : (q % 4 == 3);
        Split2 wc;
        VJP_FENCE();
        load_w_vjp(fr, rec, lane, wc);
        if (first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = fr[(l2 ? frag::B2 : frag::B3) + ot * 32 + f0(r) + 4 * h];
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
            if (l2) { a2[ot] = acc; split2(acc, 0, x2[ot][0]); split2(acc, 1, x2[ot][1]); }
            else a3[ot] = acc;
        }
    }
}

// derivative of relu_cap: 1 strictly inside (0, cap), 0 on both flat branches
__device__ __forceinline__ float mask_cap(float a, float d) { return a > 0.0f && a < NDP_H16_CAP ? d : 0.0f; }

// one 32-feature tile of a wave's [feature][row] registers into its LDS image at feature row `tile * 32`
__device__ __forceinline__ void park(lds_f32 dst, const f16_t &v, int tile, int lane)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[(tile * 32 + f0(r) + 4 * (lane >> 5)) * VJ_PITCH + (lane & 31)] = v[r];
}

// acc[m][n] += sum over the rows of the open tiles of  D[mt*32 + m][row] A[nt*32 + n][row]; D at feature row 0 of every wave's image, A
// at feature row `arow`.  dlim / alim: features of the tile that exist (the others read as 0); aone: feature of A that reads as 1 (bias
// column) or -1.
__device__ __forceinline__ void contract(lds_cf32 buf, const int open[4], int mt, int nt, int arow, int dlim, int alim, int aone, int lane,
                                         f16_t &acc)
{
    const int m = lane & 31, h = lane >> 5;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        if (!open[w]) continue;
        lds_cf32 base = buf + w * VJ_WAVE;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const float a = m < dlim ? base[(mt * 32 + m) * VJ_PITCH + 2 * ks + h] : 0.0f;
            const float b = m < alim ? base[(arow + nt * 32 + m) * VJ_PITCH + 2 * ks + h] : (m == aone ? 1.0f : 0.0f);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
}

// bias gradient of one layer: thread t sums feature t & 127 of the image's D part over the rows of two waves (t >> 7)
__device__ __forceinline__ float bias_rows(lds_cf32 buf, const int open[4], int nfeat, int tid)
{
    const int f = tid & 127, half = tid >> 7;
    float s = 0.0f;
    if (f < nfeat) {
#pragma unroll
        for (int ww = 0; ww < 2; ++ww) {
            const int w = 2 * half + ww;
            if (!open[w]) continue;
            lds_cf32 p = buf + w * VJ_WAVE + f * VJ_PITCH;
            for (int j = 0; j < 32; ++j) s += p[j];
        }
    }
    return s;
}

// The body of both backward kernels is mlp_vjp_body.inc, included as text: a template or an inlined function around it changed the
// registers the compiler gives mlp_vjp_kernel, and that kernel's code object is held fixed.  The body names the instance whose ego window,
// ego xy and upstream row it reads through two macros.
#define VJP_EGO inst
#define VJP_FROW (size_t)row
__global__ __launch_bounds__(256) void mlp_vjp_kernel(MlpVjpArgs A)
{
#include "mlp_vjp_body.inc"
}
#undef VJP_EGO
#undef VJP_FROW

// K slots per instance (ndp_downwash_multi_vjp_device), other_index int32[B][K] (required): one launch instead of K launches, K reductions
// and K - 1 adds.  The rows are VIRTUAL rows (i K + k) (N+1) + n, A.rows = B K (N+1) of them: the pair (instance i, slot k) plays the part of
// the instance -- its neighbour row and gate come from other_index[i][k], which is entry i K + k of the flat array, the body's own
// expression -- while the ego window, the ego xy and the upstream row are those of the real instance i (f is the sum of the slots, so its
// gradient is shared by them).  g_z goes out as the virtual rows lie, [B][K][N+1][6]; the weight gradient accumulates over all (row, slot)
// in the same registers.  A tile none of whose rows is open -- a closed or empty slot's -- costs its gate and nothing else.  Nothing else
// differs, so at K = 1 this is mlp_vjp_kernel's arithmetic in mlp_vjp_kernel's order.
#define VJP_EGO (inst / K)
#define VJP_FROW ((size_t)(inst / K) * A.np1 + k)
__global__ __launch_bounds__(256) void mlp_vjp_multi_kernel(MlpVjpArgs A, int K)
{
#include "mlp_vjp_body.inc"
}
#undef VJP_EGO
#undef VJP_FROW

__global__ __launch_bounds__(256) void mlp_vjp_reduce_kernel(const float *__restrict__ part, int groups, float *__restrict__ out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= PTOTAL) return;
    float s = 0.0f;
    for (int g = 0; g < groups; ++g) s += part[(size_t)g * PTOTAL + i];      // fixed order
    out[i] = s;
}

}  // namespace ndp

using namespace ndp;

extern "C" {

void make_fragments_t(const float *blob, float *frt)
{
    for (int i = 0; i < FRT_TOTAL; ++i) frt[i] = blob[fragt_source(i)];
}

hipError_t mlp_vjp_prepare(void)
{
    const hipError_t e = hipFuncSetAttribute((const void *)mlp_vjp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(VJ_LDS_FLOATS * sizeof(float)));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)mlp_vjp_multi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(VJ_LDS_FLOATS * sizeof(float)));
}

int ndp_downwash_vjp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, const void *d_ego_ref,
                            const void *d_ego_xy, const void *d_gf, void *d_gz, void *d_gw, void *stream)
{
    Entry g(h, d_other && d_ego_ref, stream);
    if (g.rc) return g.rc;
    const char *why = nullptr;
    if (!h->have_mlp) { h->err = "ndp_downwash_vjp_device: ndp_set_mlp_weights was never called"; return -6; }
    if (other_stride != 6 && other_stride != NX) why = "ndp_downwash_vjp_device: other_stride must be 6 or 10";
    else if (!d_gf) why = "ndp_downwash_vjp_device: d_gf is required (the upstream gradient of the force)";
    else if (!d_gz && !d_gw) why = "ndp_downwash_vjp_device: no output asked for (d_gz and d_gw both NULL)";
    if (why) { h->err = why; return -2; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int G = mlp_vjp_groups(h);
    MlpVjpArgs a{h->dFrag, h->dFragT, (const double *)d_other, (const double *)d_ego_ref, (const double *)d_ego_xy, (const double *)d_gf,
                 (double *)d_gz, d_gw ? h->dGwPart : nullptr, rows, np1, h->cfg.r_horiz * h->cfg.r_horiz, other_stride,
                 (const int *)d_other_index, peer_mapped(d_other), (size_t)np1 * other_stride, (size_t)np1 * NX, (size_t)2};
    hipLaunchKernelGGL(mlp_vjp_kernel, dim3(G), dim3(256), VJ_LDS_FLOATS * sizeof(float), g.s, a);
    NDP_HIP(h, hipGetLastError());
    if (d_gw) {
        hipLaunchKernelGGL(mlp_vjp_reduce_kernel, dim3((PTOTAL + 255) / 256), dim3(256), 0, g.s, (const float *)h->dGwPart, G, (float *)d_gw);
        NDP_HIP(h, hipGetLastError());
    }
    return g.noted(0);
}

int ndp_downwash_multi_vjp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, int K,
                                  const void *d_ego_ref, const void *d_ego_xy, const void *d_gf, void *d_gz, void *d_gw, void *stream)
{
    Entry g(h, d_other && d_ego_ref, stream);
    if (g.rc) return g.rc;
    const char *why = nullptr;
    if (!h->have_mlp) { h->err = "ndp_downwash_multi_vjp_device: ndp_set_mlp_weights was never called"; return -6; }
    if (K < 1 || K > NDP_MAX_NEIGH) why = "ndp_downwash_multi_vjp_device: K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle)";
    else if (!d_other_index) why = "ndp_downwash_multi_vjp_device: d_other_index is required (int32 [B][K])";
    else if (other_stride != 6 && other_stride != NX) why = "ndp_downwash_multi_vjp_device: other_stride must be 6 or 10";
    else if (!d_gf) why = "ndp_downwash_multi_vjp_device: d_gf is required (the upstream gradient of the summed force)";
    else if (!d_gz && !d_gw) why = "ndp_downwash_multi_vjp_device: no output asked for (d_gz and d_gw both NULL)";
    if (why) { h->err = why; return -2; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * K * np1;          // virtual rows
    // the workspace is ndp_downwash_vjp_device's, [mlp_vjp_groups][NDP_MLP_NPARAM]: never more workgroups than it has rows (the grid-stride
    // loop takes the rest); at K = 1 this is ndp_downwash_vjp_device's grid, hence its summation order
    const int ngroups = ((rows + 31) / 32 + 3) / 4, cap = mlp_vjp_groups(h), G = ngroups < cap ? ngroups : cap;
    MlpVjpArgs a{h->dFrag, h->dFragT, (const double *)d_other, (const double *)d_ego_ref, (const double *)d_ego_xy, (const double *)d_gf,
                 (double *)d_gz, d_gw ? h->dGwPart : nullptr, rows, np1, h->cfg.r_horiz * h->cfg.r_horiz, other_stride,
                 (const int *)d_other_index, peer_mapped(d_other), (size_t)np1 * other_stride, (size_t)np1 * NX, (size_t)2};
    hipLaunchKernelGGL(mlp_vjp_multi_kernel, dim3(G), dim3(256), VJ_LDS_FLOATS * sizeof(float), g.s, a, K);
    NDP_HIP(h, hipGetLastError());
    if (d_gw) {
        hipLaunchKernelGGL(mlp_vjp_reduce_kernel, dim3((PTOTAL + 255) / 256), dim3(256), 0, g.s, (const float *)h->dGwPart, G, (float *)d_gw);
        NDP_HIP(h, hipGetLastError());
    }
    return g.noted(0);
}

int ndp_set_mlp_weights_device(ndp_handle *h, const void *d_blob, void *stream)
{
    Entry g(h, d_blob != nullptr, stream);
    if (g.rc) return g.rc;
    hipLaunchKernelGGL(mlp_frag_kernel, dim3((frag::TOTAL + 255) / 256), dim3(256), 0, g.s, (const float *)d_blob, (unsigned *)h->dFrag, h->dFragT);
    NDP_HIP(h, hipGetLastError());
    h->have_mlp = true;
    return g.noted(0);
}

int ndp_debug_mlp_fragments(ndp_handle *h, void *frag_out, float *fragt_out)
{
    Entry g(h, true);
    if (g.rc) return g.rc;
    NDP_HIP(h, hipDeviceSynchronize());
    if (frag_out) NDP_HIP(h, hipMemcpy(frag_out, h->dFrag, frag::TOTAL * sizeof(float), hipMemcpyDeviceToHost));
    if (fragt_out) NDP_HIP(h, hipMemcpy(fragt_out, h->dFragT, FRT_TOTAL * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
