// mlp_jvp_dev.hpp -- the device code of the downwash network's forward mode that two units' kernels inline (mlp_jvp.hip: mlp_jvp_kernel,
// mlp_jvp_multi_kernel; plant_force_deriv.hip: plant_force_jvp_kernel): the forward that keeps all three hidden activations and the
// pieces of one direction's pass.  The direction itself is text: mlp_jvp_direction.inc, which also needs the blob's layout (PW1 .. PB4).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"
#include "mlp_common.hpp"

namespace ndp {

typedef float f4_t __attribute__((ext_vector_type(4)));

// (as mlp_vjp.hip's VJP_FENCE: the weights come from global memory in fully unrolled loops; a compiler-only memory fence between groups
// bounds what is requested ahead)
#define JVP_FENCE() asm volatile("" ::: "memory")

// four consecutive floats of a direction of the weights; a direction starts at a multiple of 17 859 floats, so only 4-byte alignment holds
__device__ __forceinline__ f4_t ld4(const float *p)
{
    f4_t v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

__device__ __forceinline__ void jvp_load_w(const float *fr, int rec, int lane, Split2 &w)      // copy of mlp_vjp.hip's load_w_vjp
{
    const h16x8 *p = reinterpret_cast<const h16x8 *>(fr + frag::HF) + rec * 128 + lane;
    w.hi = p[0]; w.lo = p[64];
}

// one 32-feature tile of the first layer's activations (mlp_tile's layer 1; copy of mlp_vjp.hip's vjp_layer1)
__device__ __forceinline__ f16_t jvp_layer1(const float *fr, const float zb[3], int lane, int ot)
{
    f16_t acc;
    JVP_FENCE();
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fr[frag::B1 + ot * 32 + f0(r) + 4 * (lane >> 5)];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[frag::L1 + (ot * 3 + s) * 64 + lane], zb[s], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = relu_cap(acc[r]);
    return acc;
}

// mlp_tile's forward (mlp_tile.hpp) with the weights read from global memory, keeping all three hidden activations, and its last layer:
// the same matrix instructions in the same order on the same operands, the same chain of fused multiply-adds behind them, so o[] is
// mlp_kernel's force bit for bit.  (Layers 1..3: copy of mlp_vjp.hip's vjp_forward, which does not keep a1 and has no layer 4.)
__device__ __forceinline__ void jvp_forward(const float *fr, const float zb[3], int lane, f16_t a1[4], f16_t a2[2], f16_t a3[4], float o[3])
{
    const int h = lane >> 5;
    Split2 x1[4][2], x2[2][2];
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
        a1[ot] = jvp_layer1(fr, zb, lane, ot);
        split2(a1[ot], 0, x1[ot][0]);
        split2(a1[ot], 1, x1[ot][1]);
    }
    f16_t acc, accl;
#pragma unroll
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const bool first = l2 ? (q % 8 == 0) : (q % 4 == 0), last = l2 ? (q % 8 == 7) : (q % 4 == 3);
        Split2 wc;
        JVP_FENCE();
        jvp_load_w(fr, rec, lane, wc);
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
    const f4_t *w4 = reinterpret_cast<const f4_t *>(fr + frag::W4);
    o[0] = o[1] = o[2] = 0.0f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        JVP_FENCE();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f4_t q = w4[it * 32 + f0(r) + 4 * h];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = fmaf(q[c], a3[it][r], o[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = o[c] + __shfl_xor(o[c], 32, 64) + fr[frag::B4 + c];
}

// derivative of relu_cap as mlp_vjp.hip's mask_cap defines it: 1 strictly inside (0, cap), 0 on both flat branches
__device__ __forceinline__ float jvp_mask_cap(float a, float d) { return a > 0.0f && a < NDP_H16_CAP ? d : 0.0f; }

// acc += W[out tile][in tiles 0..nit-1] d, W rebuilt from the pair records rec0 + 2 it + s (see the head of this file)
__device__ __forceinline__ void jvp_dense(const float *fr, int rec0, int nit, const f16_t *d, int lane, f16_t &acc)
{
#pragma unroll
    for (int it = 0; it < nit; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            Split2 w;
            JVP_FENCE();
            jvp_load_w(fr, rec0 + 2 * it + s, lane, w);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fmaf((float)w.lo[j], NDP_LO_INV, (float)w.hi[j]), d[it][8 * s + j], acc, 0, 0, 0);
        }
    }
}

// acc += dW[out tile][in tiles 0..nit-1] a; wrow = this lane's row of dW plus 4 (lane >> 5): registers 4 q .. 4 q + 3 of an in-tile are
// its features 8 q + 4 (lane >> 5) + 0..3
__device__ __forceinline__ void jvp_dweight(const float *wrow, int nit, const f16_t *a, f16_t &acc)
{
#pragma unroll
    for (int it = 0; it < nit; ++it) {
        JVP_FENCE();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f4_t v = ld4(wrow + it * 32 + 8 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[i], a[it][4 * q + i], acc, 0, 0, 0);
        }
    }
}

// the accumulator a tile's tangent starts from: the bias direction of its 32 features, or 0
__device__ __forceinline__ f16_t jvp_dbias(const float *tb, int h)
{
    f16_t acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f4_t v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (tb) v = ld4(tb + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * q + i] = v[i];
    }
    return acc;
}

}  // namespace ndp
