// mlp_common.hpp -- what the downwash network's kernels share across translation units (mlp_tile.hpp: mlp_tile; downwash.hip: mlp_kernel; rti_kernels.hip: the fused
// control step; mlp_vjp.hip: the network's backward pass): the fragment blob's offsets, the fp16 pair split, the capped ReLU, the gate and
// the neighbour-window loads.  Device code only; every function is inlined into its caller.
#pragma once
#include <hip/hip_runtime.h>

namespace ndp {

// Individually rounded multiply / add.  hipcc contracts a*b+c into an FMA by default, and HIP's __dmul_rn/__dadd_rn
// are plain operators that get re-fused; the reference evaluates the gate, the Kalman filter and the alpha filter
// in Python/numpy doubles without fusion, so these few expressions are built from non-contractable operations.
__device__ __forceinline__ double nc_mul(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double nc_add(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}

// Neighbour windows that live in ANOTHER agent's memory (peer windows over xGMI) are read with system-scope loads: such lines are
// not kept coherent in this GPU's L2s, and what a kernel boundary invalidates depends on the fence scope the runtime put on the
// dispatch packet (agent scope between back-to-back launches of one queue).  A system-scope load always fetches from the owner's
// memory -- two 8-byte loads per lane and launch instead of one 16-byte load, nothing else changes.  Local windows: plain loads.
typedef double ndp_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double ld_other(const double *p, int sys)
{
    return sys ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : *p;
}
__device__ __forceinline__ ndp_d2 ld_other2(const double *p, int sys)
{
    if (sys) {
        ndp_d2 r;
        r[0] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        r[1] = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return r;
    }
    return *(const ndp_d2 *)p;
}

typedef float f16_t __attribute__((ext_vector_type(16)));

// The fragment blob's offsets in float units (mlp_tile.hpp: enum FR_*, which defines the layout and asserts that these agree with it).
namespace frag {
constexpr int L1 = 0, B1 = L1 + 12 * 64, B2 = B1 + 128, B3 = B2 + 64, W4 = B3 + 128, B4 = W4 + 4 * 128, HF = B4 + 4, REC = 512,
              USED = HF + 32 * REC, TOTAL = (USED + 2047) / 2048 * 8 * 256;
}

__device__ __forceinline__ int f0(int r) { return (r & 3) + 8 * (r >> 2); }

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
struct Split2 { h16x8 hi, lo; };
// 2^11: the low parts are carried scaled by the reciprocal of fp16's relative spacing, |lo| = |x - hi| * 2^11 <= |x|.  That does NOT keep
// them fp16-normal: lo is an fp16 subnormal whenever |x - hi| < 2^-25 -- always for |x| < 2^-14, where hi is subnormal too -- so the pair
// relies on subnormal fp16 operands being honoured by the conversions and by v_mfma_f32_32x32x16_f16 (tests/test_downwash_weights_gpu.py
// holds the tile to that with weights rescaled into this range).  The pair's absolute resolution is 2^-35 (fp16's 2^-24 / 2^11).
#define NDP_LO_SCALE 2048.0f
#define NDP_LO_INV (1.0f / 2048.0f)
#define NDP_H16_CAP 65000.0f            // activations are capped below the fp16 overflow threshold (see split2)

// x = hi + lo / 2^11 with two fp16 terms (11 + 11 significand bits; fp32 has 24): hi = fp16(x), the residual
// x - hi is exact in fp32 and lo = fp16(residual * 2^11).  Error of the pair 2^-22 |x| + 2^-35.
__device__ __forceinline__ void split2(const f16_t &v, int s, Split2 &o)
{
    typedef float f2_t __attribute__((ext_vector_type(2)));
    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < 8; j += 2) {            // two registers at a time: packed f32 subtract / multiply, packed conversions
        const f2_t x = {v[8 * s + j], v[8 * s + j + 1]};
        const h2_t hh = __builtin_convertvector(x, h2_t);
        const f2_t r = (x - __builtin_convertvector(hh, f2_t)) * NDP_LO_SCALE;
        const h2_t ll = __builtin_convertvector(r, h2_t);
        o.hi[j] = hh[0]; o.hi[j + 1] = hh[1];
        o.lo[j] = ll[0]; o.lo[j + 1] = ll[1];
    }
}

// ReLU of a hidden layer that feeds an fp16 split, capped at NDP_H16_CAP: one v_med3_f32, the price of a plain
// v_max_f32.  The cap only acts on inputs ~1000x outside the training envelope, where the reference returns a finite
// meaningless force; uncapped, the fp16 conversion would overflow to inf and turn that into NaN.
__device__ __forceinline__ float relu_cap(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, NDP_H16_CAP); }

// one (output tile, 16-deep k-step): W x = W_hi x_hi + (W_hi x_lo + W_lo x_hi) / 2^11; the dropped W_lo x_lo term is
// below 2^-22 of the result.  Three v_mfma_f32_32x32x16_f16 (products exact in the fp32 accumulators), the cross terms
// in their own accumulator.  16x the f32 MFMA rate per instruction, so the three still run 5x faster than the exact
// f32 form; measured error on the reference fixture 3.7e-6 (bar 1e-5).
__device__ __forceinline__ void mm3(const Split2 &w, const Split2 &x, f16_t &acc_hi, f16_t &acc_lo)
{
    acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(w.lo, x.hi, acc_lo, 0, 0, 0);
    acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(w.hi, x.lo, acc_lo, 0, 0, 0);
    acc_hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(w.hi, x.hi, acc_hi, 0, 0, 0);
}

// gate of ndp_nmpc_leader_node.py:65-68: other.x[0] xy against ego ODOMETRY xy, strict '<'.  Individually rounded
// mul/add (nc_mul / nc_add): the reference evaluates this in Python doubles and must agree at the rim.
__device__ __forceinline__ bool gate_open(const double *other_inst, const double *ego_xy_inst, double r2)
{
    const double dx = other_inst[0] - ego_xy_inst[0];
    const double dy = other_inst[1] - ego_xy_inst[1];
    return nc_add(nc_mul(dx, dx), nc_mul(dy, dy)) < r2;
}

}  // namespace ndp
