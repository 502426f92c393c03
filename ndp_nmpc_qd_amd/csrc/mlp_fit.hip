// mlp_fit.hip -- the downwash network on sample rows (nn_train.py:99-108,131,142-147: flat x [n,6], y [n,3] in float32, nn.MSELoss,
// loss.backward(); nn_test.py: the network on grid rows): the forward, and the fit's loss and weight gradient in one pass.
//
// Kernels
//   mlp_rows_kernel       : the forward alone, LDS-free, one wave per 32-row tile.
//   mlp_fit_rows_kernel   : mlp_vjp_kernel's geometry and backward pass (mlp_vjp_dev.hpp, mlp_vjp_back.inc, mlp_vjp_part.inc) behind the
//                           forward with its last layer, the residual and the loss term.
//   mlp_fit_reduce_kernel : gradient, loss and row counts out of the workgroups' partials in a fixed order.
// A unit of its own: beside mlp_vjp_kernel in one module the compiler gave that kernel other registers, and its code object is held fixed.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"
#include "mlp_common.hpp"
#include "mlp_vjp_dev.hpp"

namespace ndp {

// ----------------------------------------------------------------------------------------------- the network on sample rows, and its fit
// ndp_mlp_rows_device / ndp_mlp_fit_rows_device: rows [R][6] fp32 as the caller holds them, no window, no gate; output or batch row m uses
// data row index[m] (null: m); an index outside 0..R-1 is an empty slot -- never read, its force exactly 0, nothing added anywhere.
struct MlpFitArgs {
    const float *fr, *frt;
    const float *z, *y, *rw;       // [R][6] | [R][3] | [R] or null (every weight 1)
    const int *index;              // [M] or null
    float *f;                      // [M][3] or null
    float *part;                   // [gridDim.x][NDP_MLP_NPARAM] or null (no weight gradient asked for: none of the backward pass runs)
    double *lpart;                 // [gridDim.x] sum over the workgroup's rows of rw |e|^2
    int *ipart;                    // [gridDim.x][2] rows used | rows skipped
    long long R, M;
    double scale;
};

// the last layer (128 -> 3) behind vjp_forward: mlp_tile's, the same fused multiply-adds in the same order, the weights from global memory
__device__ __forceinline__ void rows_layer4(const float *fr, const f16_t a3[4], int lane, float o[3])
{
    typedef float f4_t __attribute__((ext_vector_type(4)));
    const f4_t *w4 = reinterpret_cast<const f4_t *>(fr + frag::W4);
    const int h = lane >> 5;
    o[0] = o[1] = o[2] = 0.0f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        VJP_FENCE();
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

// this lane's three inputs of data row src (a half-wave holds features 2s + h); *fin: all six of the row are finite -- a row that is not
// runs the network on zeros (its activations meet the weight path with an upstream of 0, and 0 x NaN would poison the sums)
__device__ __forceinline__ void rows_load_z(const float *z, long long src, bool open, int h, float zb[3], bool *fin)
{
    bool ok = true;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        zb[s] = open ? z[(size_t)src * 6 + 2 * s + h] : 0.0f;
        ok = ok && __builtin_isfinite(zb[s]);
    }
    const int half = (int)ok, other = __shfl_xor(half, 32, 64);      // (every lane takes part: no short circuit around the exchange)
    ok = half != 0 && other != 0;
    if (!ok) zb[0] = zb[1] = zb[2] = 0.0f;
    *fin = ok;
}

// The forward alone: one wave per 32-row tile, four per workgroup, no LDS; vjp_forward + rows_layer4 are mlp_tile's arithmetic, so a row is
// bit-equal to what mlp_kernel gives for the same six fp32 inputs.  A tile of empty slots costs its index loads and three stores.
__global__ __launch_bounds__(256) void mlp_rows_kernel(MlpFitArgs A)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const long long row = ((long long)blockIdx.x * 4 + wave) * 32 + j;
    const bool valid = row < A.M;
    long long src = -1;
    if (valid) src = A.index ? (long long)A.index[row] : row;
    const bool open = valid && src >= 0 && src < A.R;
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (__ballot(open) != 0ull) {
        float zb[3];
        bool fin;
        f16_t a2[2], a3[4];
        rows_load_z(A.z, src, open, h, zb, &fin);
        vjp_forward(A.fr, zb, lane, a2, a3);
        rows_layer4(A.fr, a3, lane, o);
        if (!fin) o[0] = o[1] = o[2] = __builtin_nanf("");
    }
    if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A.f[(size_t)row * 3 + c] = open ? o[c] : 0.0f;
    }
}

// Loss and weight gradient of the fit in one pass: mlp_vjp_kernel's geometry (256 threads, a 32-row tile per wave and round, a grid-stride
// loop over groups of four tiles, the weight gradient in registers across it), the forward with its last layer and the residual in front
// of the backward pass of mlp_vjp_back.inc.  Per row: e = f - y in fp32, the loss term rw (e0^2 + e1^2 + e2^2) in fp64 (each square is
// exact there), the upstream d4[c] = fp32(2 scale rw e[c]) formed in fp64.  A row whose z, y, rw, prediction or residual is not finite is
// skipped: counted, upstream 0, no loss term.  The loss terms are summed per lane over the rounds, then over the wave by a butterfly and
// over the four waves in wave order: a fixed order for a given (M, gridDim.x).
__global__ __launch_bounds__(256) void mlp_fit_rows_kernel(MlpFitArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float vsm[];
    lds_f32 buf = (lds_f32)vsm;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (int)((A.M + 31) / 32), ngroups = (ntiles + 3) / 4;
    const bool want_w = A.part != nullptr;
    lds_f32 mine = buf + wave * VJ_WAVE;

    f16_t g4, g3[2], g2[2], g1;          // this wave's share of the weight gradient, as in mlp_vjp_body.inc
#pragma unroll
    for (int r = 0; r < 16; ++r) g4[r] = g3[0][r] = g3[1][r] = g2[0][r] = g2[1][r] = g1[r] = 0.0f;
    float gb4 = 0.0f, gb3 = 0.0f, gb2 = 0.0f;
    double lsum = 0.0;
    int used = 0, skipped = 0;          // (wave-uniform: counted off ballots, in scalar registers)

#pragma unroll 1
    for (int grp = (int)blockIdx.x; grp < ngroups; grp += (int)gridDim.x) {
        const float *fr = A.fr, *frt = A.frt;
        asm volatile("" : "+s"(fr), "+s"(frt));          // (see mlp_vjp_body.inc)
        const long long row = ((long long)grp * 4 + wave) * 32 + j;
        const bool valid = row < A.M;
        long long src = -1;
        if (valid) src = A.index ? (long long)A.index[row] : row;
        const bool open = valid && src >= 0 && src < A.R;
        const int tile_open = __builtin_amdgcn_readfirstlane((int)(__ballot(open) != 0ull));
        float d4[3] = {0.0f, 0.0f, 0.0f}, o[3] = {0.0f, 0.0f, 0.0f};
        f16_t a2[2], a3[4], dl[4];
        float zb[3];
        if (tile_open) {
            bool fin, ok = false;
            rows_load_z(A.z, src, open, h, zb, &fin);
            vjp_forward(fr, zb, lane, a2, a3);
            rows_layer4(fr, a3, lane, o);
            if (open) {
                const float w = A.rw ? A.rw[src] : 1.0f;
                float e[3];
                ok = fin && __builtin_isfinite(w);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    e[c] = o[c] - A.y[(size_t)src * 3 + c];      // (o finite, y finite and no overflow <=> e finite)
                    ok = ok && __builtin_isfinite(e[c]);
                }
                if (ok) {
                    const double s0 = (double)e[0] * (double)e[0], s1 = (double)e[1] * (double)e[1], s2 = (double)e[2] * (double)e[2];
                    if (h == 0) lsum += (double)w * (s0 + s1 + s2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) d4[c] = (float)(2.0 * A.scale * (double)w * (double)e[c]);
                }
                if (!fin) o[0] = o[1] = o[2] = __builtin_nanf("");
            }
            used += __popcll(__ballot(open && ok && h == 0));
            skipped += __popcll(__ballot(open && !ok && h == 0));
        }
        if (A.f && valid && h == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) A.f[(size_t)row * 3 + c] = open ? o[c] : 0.0f;
        }
        if (want_w) {
#include "mlp_vjp_back.inc"
        }
    }
    if (want_w) {
#include "mlp_vjp_part.inc"
    }

    // ---- this workgroup's loss term and row counts
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
    __syncthreads();
    __attribute__((address_space(3))) double *ls = (__attribute__((address_space(3))) double *)buf;
    __attribute__((address_space(3))) int *is = (__attribute__((address_space(3))) int *)(buf + 8);
    if (lane == 0) { ls[wave] = lsum; is[2 * wave] = used; is[2 * wave + 1] = skipped; }
    __syncthreads();
    if (tid == 0) {
        A.lpart[blockIdx.x] = ((ls[0] + ls[1]) + ls[2]) + ls[3];
        A.ipart[2 * blockIdx.x] = is[0] + is[2] + is[4] + is[6];
        A.ipart[2 * blockIdx.x + 1] = is[1] + is[3] + is[5] + is[7];
    }
}

// gw, loss and the row counts out of the partials, in a fixed order
__global__ __launch_bounds__(256) void mlp_fit_reduce_kernel(const float *__restrict__ part, const double *__restrict__ lpart,
                                                             const int *__restrict__ ipart, int groups, double scale, float *__restrict__ gw,
                                                             double *__restrict__ loss, int *__restrict__ info)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (gw && i < PTOTAL) {
        float s = 0.0f;
        for (int g = 0; g < groups; ++g) s += part[(size_t)g * PTOTAL + i];
        gw[i] = s;
    }
    if (i != 0) return;
    if (loss) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s += lpart[g];
        *loss = scale * s;
    }
    if (info) {
        int u = 0, k = 0;
        for (int g = 0; g < groups; ++g) { u += ipart[2 * g]; k += ipart[2 * g + 1]; }
        info[0] = u; info[1] = k;
    }
}

}  // namespace ndp

using namespace ndp;

extern "C" {

// allow mlp_fit_rows_kernel's dynamic-LDS launch (ndp_create)
hipError_t mlp_fit_prepare(void)
{
    return hipFuncSetAttribute((const void *)mlp_fit_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(VJ_LDS_FLOATS * sizeof(float)));
}

// what both row calls refuse alike; null: nothing
static const char *rows_refusal(const char *who, const void *d_index, int64_t R, int64_t M, std::string &buf)
{
    const char *why = nullptr;
    if (R < 1 || M < 1) why = "R and M must be at least 1";
    else if (R > INT32_MAX || M > INT32_MAX) why = "R and M must be below 2^31 (the index list is int32)";
    else if (!d_index && M > R) why = "d_index is NULL (row m uses data row m), so M may not exceed R";
    if (!why) return nullptr;
    buf = std::string(who) + ": " + why;
    return buf.c_str();
}

int ndp_mlp_rows_device(ndp_handle *h, const void *d_z, const void *d_index, int64_t R, int64_t M, void *d_f, void *stream)
{
    Entry g(h, d_z != nullptr, stream);
    if (g.rc) return g.rc;
    if (!h->have_mlp) { h->err = "ndp_mlp_rows_device: ndp_set_mlp_weights was never called"; return -6; }
    std::string buf;
    if (rows_refusal("ndp_mlp_rows_device", d_index, R, M, buf)) { h->err = buf; return -2; }
    if (!d_f) { h->err = "ndp_mlp_rows_device: d_f is required"; return -2; }
    MlpFitArgs a{h->dFrag, h->dFragT, (const float *)d_z, nullptr, nullptr, (const int *)d_index, (float *)d_f, nullptr, nullptr, nullptr,
                 (long long)R, (long long)M, 0.0};
    hipLaunchKernelGGL(mlp_rows_kernel, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, g.s, a);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

int ndp_mlp_fit_rows_device(ndp_handle *h, const void *d_z, const void *d_y, const void *d_rw, const void *d_index, int64_t R, int64_t M,
                            double scale, int groups, void *d_loss, void *d_gw, void *d_f, void *d_info, void *stream)
{
    Entry g(h, d_z && d_y, stream);
    if (g.rc) return g.rc;
    if (!h->have_mlp) { h->err = "ndp_mlp_fit_rows_device: ndp_set_mlp_weights was never called"; return -6; }
    std::string buf;
    if (rows_refusal("ndp_mlp_fit_rows_device", d_index, R, M, buf)) { h->err = buf; return -2; }
    if (groups < 0 || groups > NDP_FIT_MAX_GROUPS) { h->err = "ndp_mlp_fit_rows_device: groups must be 0 (the library's choice) or 1..256 (NDP_FIT_MAX_GROUPS)"; return -2; }
    if (!d_loss && !d_gw && !d_f) { h->err = "ndp_mlp_fit_rows_device: no output asked for (d_loss, d_gw and d_f all NULL)"; return -2; }
    const int64_t want = (M + 127) / 128;
    const int G = groups ? groups : (int)(want < NDP_FIT_MAX_GROUPS ? want : NDP_FIT_MAX_GROUPS);
    // dFitPart: partial gradients [NDP_FIT_MAX_GROUPS][NDP_MLP_NPARAM] fp32 | partial losses [..] fp64 | row counts [..][2] int32
    double *lpart = reinterpret_cast<double *>(h->dFitPart + (size_t)NDP_FIT_MAX_GROUPS * NDP_MLP_NPARAM);
    int *ipart = reinterpret_cast<int *>(lpart + NDP_FIT_MAX_GROUPS);
    MlpFitArgs a{h->dFrag, h->dFragT, (const float *)d_z, (const float *)d_y, (const float *)d_rw, (const int *)d_index, (float *)d_f,
                 d_gw ? h->dFitPart : nullptr, lpart, ipart, (long long)R, (long long)M, scale};
    hipLaunchKernelGGL(mlp_fit_rows_kernel, dim3(G), dim3(256), VJ_LDS_FLOATS * sizeof(float), g.s, a);
    NDP_HIP(h, hipGetLastError());
    if (d_loss || d_gw || d_info) {
        hipLaunchKernelGGL(mlp_fit_reduce_kernel, dim3(d_gw ? (PTOTAL + 255) / 256 : 1), dim3(256), 0, g.s, (const float *)h->dFitPart,
                           (const double *)lpart, (const int *)ipart, G, scale, (float *)d_gw, (double *)d_loss, (int *)d_info);
        NDP_HIP(h, hipGetLastError());
    }
    return g.noted(0);
}

}  // extern "C"
