// mlp_tile.hpp -- the downwash network's forward tile as device code two units' kernels inline (rti_kernels.hip: the fused control
// step; downwash.hip: mlp_kernel): the fragment blob's layout, its transfer into LDS and the four layers of one 32-row tile.
#pragma once
#include <hip/hip_runtime.h>

#include "mlp_common.hpp"

namespace ndp {

typedef __attribute__((address_space(3))) float *lds_f32;
typedef const __attribute__((address_space(3))) float *lds_cf32;

// ------------------------------------------------------------------------------------------ MLP kernel
// nn_net.py:7-18: Linear(6,128) ReLU Linear(128,64) ReLU Linear(64,128) ReLU Linear(128,3), fp32.
// One wave = 32 horizon rows (columns of the MFMA tile); activations stay transposed [feature][row] in
// the accumulators: the 32x32 f32 accumulator holds feature (r&3)+8(r>>2)+4(lane>>5) of row lane&31 in
// register r, which is exactly the B-operand shape of the next layer's 32x32x2 step when that step
// contracts the feature pair {f0(r), f0(r)+4}.  The weights are pre-permuted on the host into that
// "fragment order" (one 64-float record per MFMA), so A operands are coalesced 256-byte loads.
// Fragment blob (built on the host by make_fragments, parked in LDS during the MLP phase), in float units:
//   FR_L1  12 x 64 f32     layer-1 A operands for v_mfma_f32_32x32x2_f32 (K = 6 inputs)
//   FR_B1/B2/B3, FR_W4 ([128 features][4]: w0 w1 w2 0), FR_B4
//   FR_HF  layers 2 and 3 as fp16 pairs: 32 records (16 per layer) x 2 splits (hi, lo * 2^11) x 64 lanes x 8 halves
// The blob is moved by LDS-DMA in 1-KB pieces (one global_load_lds_dwordx4 per wave): its size is a multiple of 256 floats.
enum { FR_L1 = 0, FR_B1 = FR_L1 + 12 * 64, FR_B2 = FR_B1 + 128, FR_B3 = FR_B2 + 64, FR_W4 = FR_B3 + 128,
       FR_B4 = FR_W4 + 4 * 128, FR_HF = FR_B4 + 4, FR_REC = 2 * 64 * 8 / 2 /* floats per record */,
       FR_USED = FR_HF + 32 * FR_REC,
       // (a multiple of 8 pieces: every wave of a 1- / 2- / 4- / 8-wave workgroup moves the SAME number of them -- see stage_fragments)
       FR_CHUNKS = (FR_USED + 2047) / 2048 * 8, FR_TOTAL = FR_CHUNKS * 256 };
static_assert(FR_HF % 4 == 0 && FR_W4 % 4 == 0, "16-byte alignment of the LDS image");
static_assert(FR_L1 == frag::L1 && FR_B1 == frag::B1 && FR_B2 == frag::B2 && FR_B3 == frag::B3 && FR_W4 == frag::W4 && FR_B4 == frag::B4 &&
              FR_HF == frag::HF && FR_REC == frag::REC && FR_TOTAL == frag::TOTAL, "mlp_common.hpp: frag:: restates this enum for mlp_vjp.hip");


// The workgroup copies the fragment blob (FR_TOTAL floats, L2-resident) into LDS by LDS-DMA: each wave issues one
// global_load_lds_dwordx4 per 1-KB piece (64 lanes x 16 B, lane-linear destination), nothing passes through VGPRs and
// all pieces are in flight at once; the caller's __syncthreads() (which waits vmcnt(0)) retires them.  Through
// registers (global_load_dwordx4 + ds_write_b128 per thread and pass) the same copy took 7.5k cycles per workgroup.
// Streaming the weights per wave straight from L2 instead made 1024 waves fetch the same lines in lockstep (channel
// hot-spotting: the MLP tile took 33k cycles at B = 1024 against 25k alone).
__device__ __forceinline__ void stage_fragments(const float *__restrict__ fr, lds_f32 dst, int tid, int nthreads)
{
    // the wave index is uniform: keep the piece loop scalar (derived from threadIdx it would run under an exec mask), a
    // compile-time number of rounds with a uniform guard on the last one
    // The number of pieces per wave must not depend on the wave: with a guarded last round the compiler cannot count the transfers
    // in flight and makes the NEXT wait of the wave -- whatever it is for -- a wait for all of them (s_waitcnt vmcnt(0)); the one-launch
    // tick's polynomial work, meant to run under the transfer, then started behind it (+2 600 cycles per tick).
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nw = nthreads >> 6;
#pragma unroll
    for (int i = 0; i < FR_CHUNKS; ++i) {
        if (i * nw >= FR_CHUNKS) break;
        const int c = wave + i * nw;
        if ((i + 1) * nw <= FR_CHUNKS || c < FR_CHUNKS)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(fr + c * 256 + lane * 4),
                                             (__attribute__((address_space(3))) void *)(dst + c * 256), 16, 0, 0);
    }
}

__device__ __forceinline__ void load_w(lds_cf32 fr, int rec, int lane, Split2 &w)
{
    const __attribute__((address_space(3))) h16x8 *p = (const __attribute__((address_space(3))) h16x8 *)(fr + FR_HF) + rec * 128 + lane;
    w.hi = p[0]; w.lo = p[64];
}

// The four layers for one 32-row tile held by one wave.  zb[s] = input feature 2s + (lane>>5) of row lane&31;
// returns the three outputs of row lane&31 in o[] (both half-waves hold the full sums).
// Measured (scripts/ubench/mfma_f16_valu_overlap.hip, profiles/r02_ubench_mfma_f16_valu_overlap.txt): a wave's f32 VALU work is
// NOT hidden behind its own v_mfma_f32_32x32x16_f16 -- 35 cycles per instruction alone, 35 + 6 + 2.5 per v_fma_f32 issued
// behind it -- so a software-pipelined form of this tile (conversions of one layer issued between the matrix instructions
// of the next) ran no faster than this layer-by-layer form (9.46 k against 9.18 k cycles); what counts is the instruction
// count.  No scheduling fences here: the compiler's own order is 0.84 k cycles shorter than a fenced one.
// Activations stay transposed [feature][row] in the accumulators.  Registers 8s..8s+7 of a 32x32 accumulator,
// converted to fp16 pairs, ARE the B operand of k-step s of the next layer (feature 16s + 8(j>>2) + 4(lane>>5) + (j&3) in
// element j); the weights are stored in that k order.
__device__ __forceinline__ void mlp_tile(lds_cf32 fr, const float zb[3], int lane, float o[3])
{
    typedef float f4_t __attribute__((ext_vector_type(4)));
    const int h = lane >> 5;
    Split2 x1[4][2], x2[2][2];
    f16_t h3[4];
    float bc[16];
    // layer 1 (6 -> 128): exact f32 MFMA, K = 2 per instruction
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
#pragma unroll
        for (int r = 0; r < 16; ++r) bc[r] = fr[FR_B1 + ot * 32 + f0(r) + 4 * h];
        f16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bc[r];        // the bias rides in the accumulator
#pragma unroll
        for (int s = 0; s < 3; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[FR_L1 + (ot * 3 + s) * 64 + lane], zb[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = relu_cap(acc[r]);
        split2(acc, 0, x1[ot][0]);
        split2(acc, 1, x1[ot][1]);
    }
    // layers 2 (128 -> 64) and 3 (64 -> 128) as one stream of 32 weight records, the next record requested before
    // the current record's six MFMAs issue
    Split2 wc, wn;
    load_w(fr, 0, lane, wc);
    f16_t acc, accl;
#pragma unroll
    for (int rec = 0; rec < 32; ++rec) {
        const bool l2 = rec < 16;
        const int q = l2 ? rec : rec - 16;
        const int ot = l2 ? q / 8 : q / 4, it = l2 ? (q / 2) % 4 : (q / 2) % 2, s = q % 2;
        const bool first = l2 ? (q % 8 == 0) : (q % 4 == 0), last = l2 ? (q % 8 == 7) : (q % 4 == 3);
        if (rec + 1 < 32) load_w(fr, rec + 1, lane, wn);
        if (first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = fr[(l2 ? FR_B2 : FR_B3) + ot * 32 + f0(r) + 4 * h];   // the bias rides in the accumulator
                accl[r] = 0.0f;
            }
        }
#ifdef NDP_DEV_HALF_TILE        // (measurement only: half of the tile's matrix instructions, wrong forces -- what a tile shared by two waves would cost at best)
        if (!(rec & 1))
#endif
        mm3(wc, l2 ? x1[it][s] : x2[it][s], acc, accl);
        if (last) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = fmaf(accl[r], NDP_LO_INV, acc[r]);
                acc[r] = l2 ? relu_cap(v) : fmaxf(v, 0.0f);
            }
            if (l2) { split2(acc, 0, x2[ot][0]); split2(acc, 1, x2[ot][1]); }
            else h3[ot] = acc;
        }
        wc = wn;
    }
    // last layer (128 -> 3) on the VALU in f32: each half-wave owns 64 of the 128 features of its row; weights come as
    // one 16-byte record per feature, the records of the next 16 features requested before the current ones are used
    const __attribute__((address_space(3))) f4_t *w4 = (const __attribute__((address_space(3))) f4_t *)(fr + FR_W4);
    f4_t qc[16], qn[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) qc[r] = w4[f0(r) + 4 * h];
    o[0] = o[1] = o[2] = 0.0f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        if (it + 1 < 4) {
#pragma unroll
            for (int r = 0; r < 16; ++r) qn[r] = w4[(it + 1) * 32 + f0(r) + 4 * h];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = fmaf(qc[r][c], h3[it][r], o[c]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) qc[r] = qn[r];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = o[c] + __shfl_xor(o[c], 32, 64) + fr[FR_B4 + c];
}

}  // namespace ndp
