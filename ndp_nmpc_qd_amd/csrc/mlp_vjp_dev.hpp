// mlp_vjp_dev.hpp -- the device code of the downwash network's backward pass that two units' kernels inline (mlp_vjp.hip: mlp_vjp_kernel,
// mlp_vjp_multi_kernel; mlp_fit.hip: mlp_fit_rows_kernel, mlp_rows_kernel): the blob's and dFragT's layout, the forward that keeps its
// activations, and the weight path's LDS image with its park / contract / bias_rows.  The rounds themselves are text: mlp_vjp_back.inc,
// mlp_vjp_part.inc.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace ndp
