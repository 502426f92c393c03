// mlp_jvp.hip -- forward mode (a Jacobian-vector product) of the downwash network (nn_net.py:7-18, 6-128-64-128-3): the mirror of
// mlp_vjp.hip's backward pass.
//
// Kernel
//   mlp_jvp_kernel : per 32-row tile and wave, four waves per workgroup (the row -> (instance, node) mapping, gate and addressing of
//                    mlp_vjp_kernel; one tile per wave, no loop over tiles, no LDS, no barrier): the forward recomputed with mlp_tile's
//                    arithmetic, all three hidden activations kept in registers (their ReLU masks are the forward's own), then for each
//                    of the call's T directions, one rolled loop,
//                      da_l = m_l (W_l da_(l-1) + dW_l a_(l-1) + db_l),  da_0 = dz,  df = W_4 da_3 + dW_4 a_3 + db_4
//                    Layers 1..3 run on v_mfma_f32_32x32x2_f32 (exact fp32 products), layer 4 on the VALU.  The A operands:
//                      W_1         the forward's own records (frag::L1)
//                      W_2, W_3    rebuilt per lane from the forward's fp16 pair records, hi + lo / 2^11 -- element j of record (ot, it, s)
//                                  is the weight that multiplies register 8 s + j of the in-tile, so no data moves between lanes; the pair
//                                  holds the weight to 2^-22 |w| + 2^-35 and honours fp16 subnormals as the forward does
//                      dW_l, db_l  read straight from the caller's blob-ordered buffer (four registers of a lane are 16 contiguous bytes
//                                  of one weight row); none of it runs when no weight direction is given
//                    A tangent is linear: nothing on its path is capped, clamped or converted to fp16, so there is no range limit on
//                    it beyond fp32's own.  Rows go from registers straight to global memory; no atomics, no workspace of the handle.
//   mlp_jvp_multi_kernel : the same with K neighbour slots per instance, a rolled loop over the slots around the per-tile work, the T
//                    directions inside it (mlp_jvp_direction.inc is the text both kernels run per direction); df summed in slot order.
// The device functions both kernels inline are mlp_jvp_dev.hpp (plant_force_deriv.hip's forward-mode kernel inlines them too).
#include <hip/hip_runtime.h>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"
#include "mlp_common.hpp"
#include "mlp_jvp_dev.hpp"

namespace ndp {

// blob order of ndp_set_mlp_weights: W1[128][6] b1 W2[64][128] b2 W3[128][64] b3 W4[3][128] b4 (the same enum as mlp_vjp.hip's)
enum { PW1 = 0, PB1 = PW1 + 128 * 6, PW2 = PB1 + 128, PB2 = PW2 + 64 * 128, PW3 = PB2 + 64, PB3 = PW3 + 128 * 64, PW4 = PB3 + 128,
       PB4 = PW4 + 3 * 128, PTOTAL = PB4 + 3 };
static_assert(PTOTAL == NDP_MLP_NPARAM, "blob layout");

struct MlpJvpArgs {
    const float *fr;
    const double *other, *ego, *ego_xy;
    const double *tz;       // [B][T][np1][6] or null
    const float *tw;        // [T][NDP_MLP_NPARAM] or null
    double *df;             // [B][T][np1][3]
    float *fchk;            // [rows][3] or null
    int rows, np1, ntan;
    double r2;
    int other_stride;
    const int *other_index;
    int other_sys;
    size_t other_pitch, ego_pitch, ego_xy_pitch;
};

__global__ __launch_bounds__(256) void mlp_jvp_kernel(MlpJvpArgs A)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (A.rows + 31) / 32;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= ntiles) return;
    const int T = A.ntan;
    const int row = tile * 32 + j;
    const bool valid = row < A.rows;
    const int rowc = valid ? row : A.rows - 1;
    const int inst = rowc / A.np1, k = rowc - inst * A.np1;
    const int orow = A.other_index ? A.other_index[inst] : inst;
    const double *oth = A.other + (size_t)(orow < 0 ? 0 : orow) * A.other_pitch;
    bool open = valid && orow >= 0;
    if (A.ego_xy) {
        const double oxy[2] = {ld_other(oth, A.other_sys), ld_other(oth + 1, A.other_sys)};
        open = open && gate_open(oxy, A.ego_xy + (size_t)inst * A.ego_xy_pitch, A.r2);
    }
    const int tile_open = __builtin_amdgcn_readfirstlane((int)(__ballot(open) != 0ull));
    const size_t trow = ((size_t)inst * T) * A.np1 + k;        // this row in direction 0; direction t: + t * np1
    if (!tile_open) {                                          // no open row: exact zeros, nothing computed
        if (valid && h == 0) {
#pragma unroll 1
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int c = 0; c < 3; ++c) A.df[(trow + (size_t)t * A.np1) * 3 + c] = 0.0;
            }
            if (A.fchk) {
#pragma unroll
                for (int c = 0; c < 3; ++c) A.fchk[(size_t)row * 3 + c] = 0.0f;
            }
        }
        return;
    }

    float zb[3], o[3];
    f16_t a1[4], a2[2], a3[4];
#pragma unroll
    for (int s = 0; s < 3; ++s)
        zb[s] = (float)(ld_other(oth + (size_t)k * A.other_stride + 2 * s + h, A.other_sys) -
                        A.ego[(size_t)inst * A.ego_pitch + (size_t)k * NX + 2 * s + h]);
    jvp_forward(A.fr, zb, lane, a1, a2, a3, o);
    if (A.fchk && valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A.fchk[(size_t)row * 3 + c] = open ? o[c] : 0.0f;
    }

#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        // (the weight records are the same in every round: keep the compiler from hoisting their loads out of the loop into registers)
        const float *fr = A.fr;
        asm volatile("" : "+s"(fr));
        // (likewise the activations: seen as loop constants, the 160 mask comparisons are hoisted in front of the loop as lane masks in
        // scalar registers, more than there are)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(a1[i]), "+v"(a3[i]));
        asm volatile("" : "+v"(a2[0]), "+v"(a2[1]));
        const float *tw = A.tw ? A.tw + (size_t)t * PTOTAL : nullptr;
        float tzb[3] = {0.0f, 0.0f, 0.0f};
        if (A.tz) {
#pragma unroll
            for (int s = 0; s < 3; ++s) tzb[s] = (float)A.tz[(trow + (size_t)t * A.np1) * 6 + 2 * s + h];
        }
#include "mlp_jvp_direction.inc"
        if (valid && h == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) A.df[(trow + (size_t)t * A.np1) * 3 + c] = open ? (double)g[c] : 0.0;
        }
    }
}

// K neighbour slots per instance (ndp_downwash_multi_jvp_device): other_index int32[B][K] (required), tz [B][T][K][np1][6].  The rows are
// the real rows (instance, node), mlp_jvp_kernel's mapping; the slots run as a ROLLED loop around its per-tile work, as mlp_multi_kernel's
// do around mlp_tile (downwash.hip), the T directions inside the slot loop.  Every weight load is invariant in both loops: the weights'
// base is made opaque at the head of every round of either.  A slot none of whose 32 rows is open is skipped as a whole.
//   f_check : the fp32 sum in slot order, the first open slot's value taken as it is -- mlp_multi_kernel's sum, bit for bit
//   df      : the fp64 sum in slot order of the slots' (double) values, kept in the output itself: the lane that owns the row stores the
//             first open slot's value and adds the later ones to what it stored (its own stores, its own loads: no other lane touches
//             the row); a row with no open slot gets its zeros behind the loop.  No atomics, no workspace.
__global__ __launch_bounds__(256) void mlp_jvp_multi_kernel(MlpJvpArgs A, int K)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (A.rows + 31) / 32;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= ntiles) return;
    const int T = A.ntan;
    const int row = tile * 32 + j;
    const bool valid = row < A.rows;
    const int rowc = valid ? row : A.rows - 1;
    const int inst = rowc / A.np1, k = rowc - inst * A.np1;
    const size_t trow = ((size_t)inst * T) * A.np1 + k;        // this row of df in direction 0; direction t: + t * np1
    double e[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) e[s] = A.ego[(size_t)inst * A.ego_pitch + (size_t)k * NX + 2 * s + h];
    float f[3] = {0.0f, 0.0f, 0.0f};
    bool any = false;
#pragma unroll 1
    for (int slot = 0; slot < K; ++slot) {
        const float *frq = A.fr;
        asm volatile("" : "+s"(frq));
        const int orow = A.other_index[(size_t)inst * K + slot];
        const double *oth = A.other + (size_t)(orow < 0 ? 0 : orow) * A.other_pitch;
        bool open = valid && orow >= 0;
        if (A.ego_xy) {
            const double oxy[2] = {ld_other(oth, A.other_sys), ld_other(oth + 1, A.other_sys)};
            open = open && gate_open(oxy, A.ego_xy + (size_t)inst * A.ego_xy_pitch, A.r2);
        }
        if (__ballot(open) == 0ull) continue;
        float zb[3], o[3];
        f16_t a1[4], a2[2], a3[4];
#pragma unroll
        for (int s = 0; s < 3; ++s) zb[s] = (float)(ld_other(oth + (size_t)k * A.other_stride + 2 * s + h, A.other_sys) - e[s]);
        jvp_forward(frq, zb, lane, a1, a2, a3, o);
        if (open) {
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = any ? f[c] + o[c] : o[c];
        }
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
            // (as mlp_jvp_kernel's T loop: weights and activations made opaque per round)
            const float *fr = A.fr;
            asm volatile("" : "+s"(fr));
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(a1[i]), "+v"(a3[i]));
            asm volatile("" : "+v"(a2[0]), "+v"(a2[1]));
            const float *tw = A.tw ? A.tw + (size_t)t * PTOTAL : nullptr;
            float tzb[3] = {0.0f, 0.0f, 0.0f};
            if (A.tz) {
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    tzb[s] = (float)A.tz[((((size_t)inst * T + t) * K + slot) * A.np1 + k) * 6 + 2 * s + h];
            }
#include "mlp_jvp_direction.inc"
            if (open && h == 0) {
                double *d = A.df + (trow + (size_t)t * A.np1) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = any ? d[c] + (double)g[c] : (double)g[c];
            }
        }
        any = any || open;
    }
    if (valid && h == 0) {
        if (!any) {
#pragma unroll 1
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int c = 0; c < 3; ++c) A.df[(trow + (size_t)t * A.np1) * 3 + c] = 0.0;
            }
        }
        if (A.fchk) {
#pragma unroll
            for (int c = 0; c < 3; ++c) A.fchk[(size_t)row * 3 + c] = f[c];
        }
    }
}

}  // namespace ndp

using namespace ndp;

// The body of ndp_downwash_jvp_device (multi false: d_other_index optional, K not read) and ndp_downwash_multi_jvp_device (K slots, the index
// required): the refusals under `who`, the argument block, the grid (the real rows in both forms), the launch.  multi: as downwash_vjp's.
static int downwash_jvp(ndp_handle *h, const char *who, bool multi, const void *d_other, int other_stride, const void *d_other_index, int K,
                        const void *d_ego_ref, const void *d_ego_xy, int n_tan, const void *d_tz, const void *d_tw, void *d_df,
                        void *d_f_check, void *stream)
{
    Entry g(h, d_other && d_ego_ref, stream);
    if (g.rc) return g.rc;
    const char *why = nullptr;
    // (the weights in front of K here; plant_force_deriv.hip's plant_force_jvp checks K first)
    if (!h->have_mlp) { h->err = std::string(who) + ": ndp_set_mlp_weights was never called"; return -6; }
    if (multi && (K < 1 || K > NDP_MAX_NEIGH)) why = ": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle)";
    else if (multi && !d_other_index) why = ": d_other_index is required (int32 [B][K])";
    else if (other_stride != 6 && other_stride != NX) why = ": other_stride must be 6 or 10";
    else if (n_tan < 1 || n_tan > NDP_JVP_MAX_TANGENTS) why = ": n_tan must be 1..8 (directions per call)";
    else if (!d_tz && !d_tw) why = ": no tangent given (d_tz and d_tw both NULL)";
    // (the two forms word the force differently)
    else if (!d_df) why = multi ? ": d_df is required (the tangent of the summed force)" : ": d_df is required (the tangent of the force)";
    if (why) { h->err = std::string(who) + why; return -2; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * np1;
    const int ntiles = (rows + 31) / 32;
    MlpJvpArgs a{h->dFrag, (const double *)d_other, (const double *)d_ego_ref, (const double *)d_ego_xy, (const double *)d_tz,
                 (const float *)d_tw, (double *)d_df, (float *)d_f_check, rows, np1, n_tan, h->cfg.r_horiz * h->cfg.r_horiz, other_stride,
                 (const int *)d_other_index, peer_mapped(d_other), (size_t)np1 * other_stride, (size_t)np1 * NX, (size_t)2};
    if (multi) hipLaunchKernelGGL(mlp_jvp_multi_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, g.s, a, K);
    else hipLaunchKernelGGL(mlp_jvp_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, g.s, a);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

extern "C" {

int ndp_downwash_jvp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, const void *d_ego_ref,
                            const void *d_ego_xy, int n_tan, const void *d_tz, const void *d_tw, void *d_df, void *d_f_check, void *stream)
{
    return downwash_jvp(h, "ndp_downwash_jvp_device", false, d_other, other_stride, d_other_index, 0, d_ego_ref, d_ego_xy, n_tan, d_tz, d_tw,
                        d_df, d_f_check, stream);
}

int ndp_downwash_multi_jvp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, int K,
                                  const void *d_ego_ref, const void *d_ego_xy, int n_tan, const void *d_tz, const void *d_tw, void *d_df,
                                  void *d_f_check, void *stream)
{
    return downwash_jvp(h, "ndp_downwash_multi_jvp_device", true, d_other, other_stride, d_other_index, K, d_ego_ref, d_ego_xy, n_tan, d_tz,
                        d_tw, d_df, d_f_check, stream);
}

}  // extern "C"
