// plant_force_deriv.hip -- the derivatives of the downwash force ON THE PLANT (ndp_plant_force*_device, downwash.hip: plant_force_kernel,
// plant_force_multi_kernel): f[v] = sum over the slots k of scale * (double)net(fp32((x[o_k] - x[v])[0:6])), o_k = other_index[v][k], behind
// the r_horiz gate on |x[o_k].xy - x[v].xy|.  The derivative is that of this arithmetic: the rounding of z to fp32 counts as the identity,
// the gate is piecewise constant and contributes nothing, the ReLU masks are those of the forward recomputed with its own instructions.
//
// Kernels
//   plant_force_vjp_kernel    : reverse mode.  mlp_vjp_kernel's geometry (256 threads, a 32-row tile per wave and round, a grid-stride loop
//                               over groups of four tiles, the weight gradient in registers across it) over the VIRTUAL rows (vehicle v,
//                               slot k) = entry v K + k of other_index, plant_force_multi_kernel's addressing.  A row loader forms z and
//                               the gate from x and other_index and the upstream fp32(scale * gf[v]) (the product in fp64, rounded once);
//                               behind it the backward pass of mlp_vjp_dev.hpp / mlp_vjp_back.inc / mlp_vjp_part.inc and g_z = W1' d1 as
//                               at the end of mlp_vjp_body.inc.  g_z goes out per network input row, [B][K][6]: the scatter onto the
//                               states (+ to x[o], - to x[v]) is the caller's.
//   plant_force_reduce_kernel : sums the workgroups' partial weight gradients in a fixed order (mlp_vjp_reduce_kernel's loop).
//   plant_force_jvp_kernel    : forward mode.  plant_force_multi_kernel's mapping (one wave per 32 vehicles, 1 to 4 waves per workgroup, no
//                               LDS, no barrier), the slots a rolled loop around jvp_forward, the T directions inside it
//                               (mlp_jvp_direction.inc).  A slot's input direction is gathered here: the fp64 difference
//                               tx[o][t][i] - tx[v][t][i], rounded to fp32 as mlp_jvp_multi_kernel rounds its tz.  df = the fp64 sum in
//                               slot order of scale * (double)tangent, products and sums individually rounded, kept in the output itself
//                               as mlp_jvp_multi_kernel keeps it.
// A unit of its own: the code objects of mlp_vjp_kernel, mlp_jvp_kernel and their siblings are held fixed, and kernels added to their
// units moved their registers before (mlp_fit.hip).  Neither kernel is tuned; both inherit the register budgets of the bodies they host
// (DESIGN 9 has the counts), and nothing here rests on a measured latency or occupancy figure.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"
#include "mlp_common.hpp"
#include "mlp_vjp_dev.hpp"
#include "mlp_jvp_dev.hpp"

namespace ndp {

struct PlantForceVjpArgs {
    const float *fr, *frt;
    const double *x;               // [B][10]
    const int *index;              // [B][K]
    const double *gf;              // [B][3]
    double *gz;                    // [B][K][6] or null
    float *part;                   // [gridDim.x][NDP_MLP_NPARAM] or null (no weight gradient asked for)
    int B, K, gate;
    double r2, scale;
};

__global__ __launch_bounds__(256) void plant_force_vjp_kernel(PlantForceVjpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float vsm[];
    lds_f32 buf = (lds_f32)vsm;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int rows = A.B * A.K, ntiles = (rows + 31) / 32, ngroups = (ntiles + 3) / 4;
    const bool want_w = A.part != nullptr;
    lds_f32 mine = buf + wave * VJ_WAVE;

    f16_t g4, g3[2], g2[2], g1;          // this wave's share of the weight gradient, as in mlp_vjp_body.inc
#pragma unroll
    for (int r = 0; r < 16; ++r) g4[r] = g3[0][r] = g3[1][r] = g2[0][r] = g2[1][r] = g1[r] = 0.0f;
    float gb4 = 0.0f, gb3 = 0.0f, gb2 = 0.0f;

#pragma unroll 1
    for (int grp = (int)blockIdx.x; grp < ngroups; grp += (int)gridDim.x) {
        const float *fr = A.fr, *frt = A.frt;
        asm volatile("" : "+s"(fr), "+s"(frt));          // (see mlp_vjp_body.inc)
        const int tile = grp * 4 + wave;
        const int row = tile * 32 + j;
        const bool valid = row < rows;
        const int rowc = valid ? row : rows - 1;
        const int veh = rowc / A.K;
        const int nb = A.index[rowc];
        const bool has = nb >= 0 && nb < A.B;              // (an empty slot reads the vehicle's own row: z = 0, never another's memory)
        const double *xe = A.x + (size_t)veh * NX, *xo = A.x + (size_t)(has ? nb : veh) * NX;
        bool open = valid && has;
        if (A.gate) open = open && gate_open(xo, xe, A.r2);
        const int tile_open = __builtin_amdgcn_readfirstlane((int)(__ballot(open) != 0ull));
        float d4[3] = {0.0f, 0.0f, 0.0f};
        bool finite = true;
        f16_t a2[2], a3[4], dl[4];
        float zb[3];
        if (tile_open) {
            bool zfin = true;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                zb[s] = (float)(xo[2 * s + h] - xe[2 * s + h]);
                zfin = zfin && __builtin_isfinite(zb[s]);
            }
            // a row whose six inputs are not all finite runs the network on zeros, open or not: its activations meet the weight path with
            // an upstream of 0, and 0 x NaN would poison the sums (every lane takes part in the exchange)
            const int half = (int)zfin, other = __shfl_xor(half, 32, 64);
            zfin = half != 0 && other != 0;
            if (!zfin) zb[0] = zb[1] = zb[2] = 0.0f;
            if (open) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    d4[c] = (float)nc_mul(A.scale, A.gf[(size_t)veh * 3 + c]);
                    finite = finite && __builtin_isfinite(d4[c]);
                }
                finite = finite && zfin;
                // a row whose upstream gradient or input is not finite adds nothing to the weights and gets NaN itself
                if (!finite) d4[0] = d4[1] = d4[2] = 0.0f;
            }
            vjp_forward(fr, zb, lane, a2, a3);
        }

#include "mlp_vjp_back.inc"
        // g_z = W1' d1 (the end of mlp_vjp_body.inc)
        if (A.gz) {
            float gz[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (tile_open) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    VJP_FENCE();
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
#pragma unroll
                        for (int i = 0; i < 6; ++i)
                            gz[i] = fmaf(fr[frag::L1 + (t * 3 + (i >> 1)) * 64 + f0(r) + 4 * h + 32 * (i & 1)], dl[t][r], gz[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) gz[i] += __shfl_xor(gz[i], 32, 64);
            }
            if (valid && h == 0) {
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    A.gz[(size_t)row * 6 + i] = !open ? 0.0 : finite ? (double)gz[i] : (double)__builtin_nanf("");
            }
        }
    }
    if (!want_w) return;

#include "mlp_vjp_part.inc"
}

__global__ __launch_bounds__(256) void plant_force_reduce_kernel(const float *__restrict__ part, int groups, float *__restrict__ out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= PTOTAL) return;
    float s = 0.0f;
    for (int g = 0; g < groups; ++g) s += part[(size_t)g * PTOTAL + i];      // fixed order
    out[i] = s;
}

struct PlantForceJvpArgs {
    const float *fr;
    const double *x;               // [B][10]
    const int *index;              // [B][K]
    const double *tx;              // [B][T][10] or null
    const float *tw;               // [T][NDP_MLP_NPARAM] or null
    double *df;                    // [B][T][3]
    double *fchk;                  // [B][3] or null
    int B, K, ntan, gate;
    double r2, scale;
};

__global__ __launch_bounds__(256) void plant_force_jvp_kernel(PlantForceJvpArgs A)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int tile = (int)blockIdx.x * nw + wave;
    if (tile * 32 >= A.B) return;
    const int T = A.ntan;
    const int veh = tile * 32 + j;
    const bool valid = veh < A.B;
    const int vehc = valid ? veh : A.B - 1;
    const double *xe = A.x + (size_t)vehc * NX;
    double e[3], f[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 3; ++s) e[s] = xe[2 * s + h];
    bool any = false;
#pragma unroll 1
    for (int slot = 0; slot < A.K; ++slot) {
        const float *frq = A.fr;
        asm volatile("" : "+s"(frq));       // (the weights are the same in every round: mlp_jvp_multi_kernel)
        const int nb = A.index[(size_t)vehc * A.K + slot];
        const bool has = nb >= 0 && nb < A.B;
        const int nbc = has ? nb : vehc;
        const double *xo = A.x + (size_t)nbc * NX;
        bool open = valid && has;
        if (A.gate) open = open && gate_open(xo, xe, A.r2);
        if (__ballot(open) == 0ull) continue;
        float zb[3], o4[3];
        f16_t a1[4], a2[2], a3[4];
#pragma unroll
        for (int s = 0; s < 3; ++s) zb[s] = (float)(xo[2 * s + h] - e[s]);
        jvp_forward(frq, zb, lane, a1, a2, a3, o4);
        if (open) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = nc_mul(A.scale, (double)o4[c]);
                f[c] = any ? nc_add(f[c], p) : p;
            }
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
            if (A.tx) {
                const double *to = A.tx + ((size_t)nbc * T + t) * NX, *te = A.tx + ((size_t)vehc * T + t) * NX;
#pragma unroll
                for (int s = 0; s < 3; ++s) tzb[s] = (float)(to[2 * s + h] - te[2 * s + h]);
            }
#include "mlp_jvp_direction.inc"
            if (open && h == 0) {
                double *d = A.df + ((size_t)veh * T + t) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double p = nc_mul(A.scale, (double)g[c]);
                    d[c] = any ? nc_add(d[c], p) : p;
                }
            }
        }
        any = any || open;
    }
    if (valid && h == 0) {
        if (!any) {
#pragma unroll 1
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int c = 0; c < 3; ++c) A.df[((size_t)veh * T + t) * 3 + c] = 0.0;
            }
        }
        if (A.fchk) {
#pragma unroll
            for (int c = 0; c < 3; ++c) A.fchk[(size_t)veh * 3 + c] = f[c];
        }
    }
}

}  // namespace ndp

using namespace ndp;

extern "C" {

// allow plant_force_vjp_kernel's dynamic-LDS launch (ndp_create)
hipError_t plant_force_deriv_prepare(void)
{
    return hipFuncSetAttribute((const void *)plant_force_vjp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(VJ_LDS_FLOATS * sizeof(float)));
}

// The reverse launches of both forms and of closed_loop.hip's formation sweep: the refusals (-6, then -2 under `who`) before anything is
// enqueued.  No locking, no sync, K not checked (check_neigh).
int launch_plant_force_vjp(ndp_handle *h, const char *who, const void *d_x, const void *d_index, int K, int gate, double scale,
                           const void *d_gf, void *d_gz, void *d_gw, hipStream_t s)
{
    if (d_index && !h->have_mlp) { h->err = std::string(who) + ": ndp_set_mlp_weights was never called"; return -6; }
    const char *why = nullptr;
    if (!d_gf) why = ": d_gf is required (the upstream gradient of the summed force)";
    else if (!d_gz && !d_gw) why = ": no output asked for (d_gz and d_gw both NULL)";
    if (why) { h->err = std::string(who) + why; return -2; }
    const int B = h->cfg.batch, rows = B * K;
    if (!d_index) {      // nobody has a neighbour: exact zeros, no network pass, no weights needed
        if (d_gz) NDP_HIP(h, hipMemsetAsync(d_gz, 0, (size_t)rows * 6 * 8, s));
        if (d_gw) NDP_HIP(h, hipMemsetAsync(d_gw, 0, (size_t)NDP_MLP_NPARAM * 4, s));
        return 0;
    }
    // the workspace is ndp_downwash_vjp_device's, [mlp_vjp_groups][NDP_MLP_NPARAM]: never more workgroups than it has rows (the grid-stride
    // loop takes the rest)
    const int ngroups = ((rows + 31) / 32 + 3) / 4, cap = mlp_vjp_groups(h), G = ngroups < cap ? ngroups : cap;
    PlantForceVjpArgs a{h->dFrag, h->dFragT, (const double *)d_x, (const int *)d_index, (const double *)d_gf, (double *)d_gz,
                        d_gw ? h->dGwPart : nullptr, B, K, gate ? 1 : 0, h->cfg.r_horiz * h->cfg.r_horiz, scale};
    hipLaunchKernelGGL(plant_force_vjp_kernel, dim3(G), dim3(256), VJ_LDS_FLOATS * sizeof(float), s, a);
    NDP_HIP(h, hipGetLastError());
    if (d_gw) {
        hipLaunchKernelGGL(plant_force_reduce_kernel, dim3((PTOTAL + 255) / 256), dim3(256), 0, s, (const float *)h->dGwPart, G, (float *)d_gw);
        NDP_HIP(h, hipGetLastError());
    }
    return 0;
}

// Both reverse forms; K was checked by the caller.
static int plant_force_vjp(ndp_handle *h, const char *who, Entry &g, const void *d_x, const void *d_index, int K, int gate, double scale,
                           const void *d_gf, void *d_gz, void *d_gw)
{
    return g.noted(launch_plant_force_vjp(h, who, d_x, d_index, K, gate, scale, d_gf, d_gz, d_gw, g.s));
}

static int plant_force_jvp(ndp_handle *h, const char *who, Entry &g, const void *d_x, const void *d_index, int K, int gate, double scale,
                           int n_tan, const void *d_tx, const void *d_tw, void *d_df, void *d_f_check)
{
    if (d_index && !h->have_mlp) { h->err = std::string(who) + ": ndp_set_mlp_weights was never called"; return -6; }
    const char *why = nullptr;
    if (n_tan < 1 || n_tan > NDP_JVP_MAX_TANGENTS) why = ": n_tan must be 1..8 (directions per call)";
    else if (!d_tx && !d_tw) why = ": no tangent given (d_tx and d_tw both NULL)";
    else if (!d_df) why = ": d_df is required (the tangent of the summed force)";
    if (why) { h->err = std::string(who) + why; return -2; }
    const int B = h->cfg.batch;
    if (!d_index) {
        NDP_HIP(h, hipMemsetAsync(d_df, 0, (size_t)B * n_tan * 3 * 8, g.s));
        if (d_f_check) NDP_HIP(h, hipMemsetAsync(d_f_check, 0, (size_t)B * 3 * 8, g.s));
        return g.noted(0);
    }
    const int ntiles = (B + 31) / 32;
    const int nw = ntiles < 4 ? ntiles : 4;          // launch_plant_force's shape
    PlantForceJvpArgs a{h->dFrag, (const double *)d_x, (const int *)d_index, (const double *)d_tx, (const float *)d_tw, (double *)d_df,
                        (double *)d_f_check, B, K, n_tan, gate ? 1 : 0, h->cfg.r_horiz * h->cfg.r_horiz, scale};
    hipLaunchKernelGGL(plant_force_jvp_kernel, dim3((ntiles + nw - 1) / nw), dim3(64 * nw), 0, g.s, a);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

int ndp_plant_force_vjp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int gate, double scale, const void *d_gf,
                               void *d_gz, void *d_gw, void *stream)
{
    Entry g(h, d_x != nullptr, stream);
    if (g.rc) return g.rc;
    return plant_force_vjp(h, "ndp_plant_force_vjp_device", g, d_x, d_other_index, 1, gate, scale, d_gf, d_gz, d_gw);
}

int ndp_plant_force_multi_vjp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int K, int gate, double scale,
                                     const void *d_gf, void *d_gz, void *d_gw, void *stream)
{
    Entry g(h, d_x != nullptr, stream);
    if (g.rc) return g.rc;
    int rc = check_neigh(h, "ndp_plant_force_multi_vjp_device", K);
    if (rc) return rc;
    return plant_force_vjp(h, "ndp_plant_force_multi_vjp_device", g, d_x, d_other_index, K, gate, scale, d_gf, d_gz, d_gw);
}

int ndp_plant_force_jvp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int gate, double scale, int n_tan,
                               const void *d_tx, const void *d_tw, void *d_df, void *d_f_check, void *stream)
{
    Entry g(h, d_x != nullptr, stream);
    if (g.rc) return g.rc;
    return plant_force_jvp(h, "ndp_plant_force_jvp_device", g, d_x, d_other_index, 1, gate, scale, n_tan, d_tx, d_tw, d_df, d_f_check);
}

int ndp_plant_force_multi_jvp_device(ndp_handle *h, const void *d_x, const void *d_other_index, int K, int gate, double scale, int n_tan,
                                     const void *d_tx, const void *d_tw, void *d_df, void *d_f_check, void *stream)
{
    Entry g(h, d_x != nullptr, stream);
    if (g.rc) return g.rc;
    int rc = check_neigh(h, "ndp_plant_force_multi_jvp_device", K);
    if (rc) return rc;
    return plant_force_jvp(h, "ndp_plant_force_multi_jvp_device", g, d_x, d_other_index, K, gate, scale, n_tan, d_tx, d_tw, d_df, d_f_check);
}

}  // extern "C"
