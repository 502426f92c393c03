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
#include "mlp_vjp_dev.hpp"

namespace ndp {

// The backward pass's device functions and the LDS image of its weight path are mlp_vjp_dev.hpp (mlp_fit.hip's kernels inline them too).
// The image's size, which the launches below ask for, restated from there and held to it by the compiler (tests read these numbers):
//   enum { VJ_PITCH = 33, VJ_WAVE = 192 * VJ_PITCH, VJ_FLAGS = 4 * VJ_WAVE, VJ_LDS_FLOATS = VJ_FLAGS + 4 };
static_assert(VJ_PITCH == 33 && VJ_WAVE == 192 * VJ_PITCH && VJ_FLAGS == 4 * VJ_WAVE && VJ_LDS_FLOATS == VJ_FLAGS + 4,
              "mlp_vjp_dev.hpp: the LDS image's layout changed; restate it in the comment above");

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

// The body of ndp_downwash_vjp_device (multi false: d_other_index optional, K not read) and ndp_downwash_multi_vjp_device (K slots, the index
// required): the refusals under the entry's name `who`, the argument block, the grid, the launch, the reduce launch.  (multi is a flag of
// its own, not "K != 0": the multi form has to refuse K = 0 under its own name, behind the weights.)
static int downwash_vjp(ndp_handle *h, const char *who, bool multi, const void *d_other, int other_stride, const void *d_other_index, int K,
                        const void *d_ego_ref, const void *d_ego_xy, const void *d_gf, void *d_gz, void *d_gw, void *stream)
{
    Entry g(h, d_other && d_ego_ref, stream);
    if (g.rc) return g.rc;
    const char *why = nullptr;
    // (the weights in front of K here; plant_force_deriv.hip's plant_force_vjp checks K first)
    if (!h->have_mlp) { h->err = std::string(who) + ": ndp_set_mlp_weights was never called"; return -6; }
    if (multi && (K < 1 || K > NDP_MAX_NEIGH)) why = ": K must be 1..8 (NDP_MAX_NEIGH neighbours per vehicle)";
    else if (multi && !d_other_index) why = ": d_other_index is required (int32 [B][K])";
    else if (other_stride != 6 && other_stride != NX) why = ": other_stride must be 6 or 10";
    // (the two forms word the force differently)
    else if (!d_gf) why = multi ? ": d_gf is required (the upstream gradient of the summed force)" : ": d_gf is required (the upstream gradient of the force)";
    else if (!d_gz && !d_gw) why = ": no output asked for (d_gz and d_gw both NULL)";
    if (why) { h->err = std::string(who) + why; return -2; }
    const int np1 = h->cfg.N + 1, rows = h->cfg.batch * (multi ? K : 1) * np1;        // K slots: virtual rows
    // the workspace dGwPart has mlp_vjp_groups rows, one per 128 rows of the single form: never more workgroups than that (the grid-stride
    // loop takes the rest); the single form's grid is exactly that, and so is the K = 1 grid, hence its summation order
    const int ngroups = ((rows + 31) / 32 + 3) / 4, cap = mlp_vjp_groups(h), G = ngroups < cap ? ngroups : cap;
    MlpVjpArgs a{h->dFrag, h->dFragT, (const double *)d_other, (const double *)d_ego_ref, (const double *)d_ego_xy, (const double *)d_gf,
                 (double *)d_gz, d_gw ? h->dGwPart : nullptr, rows, np1, h->cfg.r_horiz * h->cfg.r_horiz, other_stride,
                 (const int *)d_other_index, peer_mapped(d_other), (size_t)np1 * other_stride, (size_t)np1 * NX, (size_t)2};
    if (multi) hipLaunchKernelGGL(mlp_vjp_multi_kernel, dim3(G), dim3(256), VJ_LDS_FLOATS * sizeof(float), g.s, a, K);
    else hipLaunchKernelGGL(mlp_vjp_kernel, dim3(G), dim3(256), VJ_LDS_FLOATS * sizeof(float), g.s, a);
    NDP_HIP(h, hipGetLastError());
    if (d_gw) {
        hipLaunchKernelGGL(mlp_vjp_reduce_kernel, dim3((PTOTAL + 255) / 256), dim3(256), 0, g.s, (const float *)h->dGwPart, G, (float *)d_gw);
        NDP_HIP(h, hipGetLastError());
    }
    return g.noted(0);
}

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
    return downwash_vjp(h, "ndp_downwash_vjp_device", false, d_other, other_stride, d_other_index, 0, d_ego_ref, d_ego_xy, d_gf, d_gz, d_gw,
                        stream);
}

int ndp_downwash_multi_vjp_device(ndp_handle *h, const void *d_other, int other_stride, const void *d_other_index, int K,
                                  const void *d_ego_ref, const void *d_ego_xy, const void *d_gf, void *d_gz, void *d_gw, void *stream)
{
    return downwash_vjp(h, "ndp_downwash_multi_vjp_device", true, d_other, other_stride, d_other_index, K, d_ego_ref, d_ego_xy, d_gf, d_gz,
                        d_gw, stream);
}

int ndp_set_mlp_weights_device(ndp_handle *h, const void *d_blob, void *stream)
{
    Entry g(h, d_blob != nullptr, stream);
    if (g.rc) return g.rc;
    hipLaunchKernelGGL(mlp_frag_kernel, dim3((frag::TOTAL + 255) / 256), dim3(256), 0, g.s, (const float *)d_blob, (unsigned *)h->dFrag.get(), h->dFragT);
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
