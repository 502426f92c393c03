// mlp_train.hip -- the optimiser step of the downwash network (nn_train.py:129-157 with --SN): full-batch Adam followed by the spectral-norm
// cap on every weight matrix, and the layers' spectral norms on their own.
//
// Kernel
//   mlp_train_kernel<ADAM> : four workgroups of 256 lanes, one per layer; the layers are independent, nothing synchronises across
//                            workgroups except the step word (below).  Per layer
//                              (a) Adam on the layer's weights and bias (ADAM only): fp64 from the fp32 inputs, m, v, p rounded to fp32 once
//                                  each, p from the STORED m and v.  A non-finite value anywhere in the gradient (every workgroup scans all
//                                  of it: 70 KB out of L2) skips (a) and (c) in all four alike;
//                              (b) sigma of the layer's weight matrix: the Gram matrix on the smaller side with v_mfma_f64_16x16x4_f64
//                                  (wave w: the 16-row band w of up to four 16x16 tiles; products of fp32 values are exact in fp64) into
//                                  LDS; Householder tridiagonalisation there (a zero column is skipped, not divided by); 8 rounds of
//                                  256-way multisection -- one Sturm count per lane, LAPACK's pivmin guard -- from a Gershgorin bound;
//                              (c) if cap > 0 and sigma > cap: w = fp32(w * (cap / sigma)) in fp64, and (b) once more on the result (the
//                                  norm reported is the norm AFTER the call).
//                            Every loop has a compile-time trip count.
//   The step word: int64 in the caller's memory.  Every workgroup reads it at entry; lane 0 of each takes a ticket when it is done (one
//   agent-scope atomic add on a word of the handle's workspace, the layer's `scaled` bit riding on it); the fourth ticket belongs to the
//   workgroup that finished last: it writes info[], step + 1 (unless skipped) and resets the ticket.  No workgroup reads the step word after
//   another has written it.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "../../include/ndp_nmpc.h"
#include "host.hpp"

namespace ndp {

// blob order of ndp_set_mlp_weights: W1[128][6] b1 W2[64][128] b2 W3[128][64] b3 W4[3][128] b4.  A layer's weights and bias are contiguous.
// Its Gram matrix G[i][j] = sum over k < 128 of a(i, k) a(j, k), a(i, k) = w[i * si + k * sk]: W'W for W1 and W3 (the columns are the
// smaller side), WW' for W2 and W4.
struct TrainLayer { int off, n, nw, nb, si, sk; };
__host__ __device__ inline TrainLayer train_layer(int l)
{
    switch (l) {
    case 0: return {0, 6, 128 * 6, 128, 1, 6};
    case 1: return {128 * 6 + 128, 64, 64 * 128, 64, 128, 1};
    case 2: return {128 * 6 + 128 + 64 * 128 + 64, 64, 128 * 64, 128, 1, 64};
    default: return {128 * 6 + 128 + 64 * 128 + 64 + 128 * 64 + 128, 3, 3 * 128, 3, 128, 1};
    }
}
static_assert(128 * 6 + 128 + 64 * 128 + 64 + 128 * 64 + 128 + 3 * 128 + 3 == NDP_MLP_NPARAM, "blob layout");

typedef WaveGfx950::d4_t d4_t;

enum { TR_N = 64, TR_PITCH = TR_N + 1, TR_ROUNDS = 8 };

struct TrainArgs {
    float *w;               // [NDP_MLP_NPARAM]; only read when !ADAM
    const float *g;
    float *m, *v;
    long long *step;
    double lr, b1, b2, eps, cap;
    double *sigma;          // [4] or null
    int *info;              // [4] or null
    unsigned *ticket;
};

struct TrainLds {
    double G[TR_N * TR_PITCH];
    double d[TR_N], e[TR_N], e2[TR_N], v[TR_N], w[TR_N], part[4 * TR_N];
};

// the wave's sum, the same bits in every lane and, on the same data, in every wave (WaveGfx950::wave_sum: four DPP steps, then four lanes
// read out and added in one order)
__device__ __forceinline__ double train_wsum(double a) { return WaveGfx950::wave_sum(a); }

// Largest singular value of the layer at w (its fp32 weight matrix): the same value in every lane of the workgroup.  Ends behind a barrier.
__device__ __forceinline__ double train_sigma(const float *w, const TrainLayer L, TrainLds &S)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = L.n, nt = (n + 15) >> 4;
    // ---- Gram matrix: A lane l = a(16 wave + (l & 15), 4 s + (l >> 4)), B lane l = a(16 tj + (l & 15), 4 s + (l >> 4)), D register r of
    // lane l = G[16 wave + (l >> 4) + 4 r][16 tj + (l & 15)] (wave_gfx950.hpp: the f64 matrix instruction's lane map)
    if (wave < nt) {
        d4_t acc[4];
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[tj] = d4_t{0.0, 0.0, 0.0, 0.0};
        const int ia = 16 * wave + (lane & 15), kq = lane >> 4;
#pragma unroll 2
        for (int s = 0; s < 32; ++s) {
            const int k = 4 * s + kq;
            const double a = ia < n ? (double)w[ia * L.si + k * L.sk] : 0.0;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                if (tj < nt) {
                    const int ib = 16 * tj + (lane & 15);
                    const double b = ib < n ? (double)w[ib * L.si + k * L.sk] : 0.0;
                    acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[tj], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
            if (tj < nt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) S.G[(16 * wave + (lane >> 4) + 4 * r) * TR_PITCH + 16 * tj + (lane & 15)] = acc[tj][r];
            }
    }
    __syncthreads();
    // ---- Householder tridiagonalisation, column k: x = G[k+1.., k] on the lanes of EVERY wave (so that its norm, the reflector v and the
    // scalars are in registers everywhere); G_sub v and the rank-two update split over the waves by 16 columns each.
    for (int k = 0; k < TR_N - 2; ++k) {
        if (k >= n - 2) break;                                           // (the same in every lane)
        const int m = n - k - 1;
        const double x = lane < m ? S.G[(k + 1 + lane) * TR_PITCH + k] : 0.0;
        const double s = train_wsum(x * x);
        if (s == 0.0) {                                                  // nothing below the diagonal: no reflection
            if (tid == 0) { S.d[k] = S.G[k * TR_PITCH + k]; S.e[k] = 0.0; }
            continue;
        }
        const double x0 = __shfl(x, 0, 64), nrm = sqrt(s), alpha = x0 > 0.0 ? -nrm : nrm;
        const double vi = lane == 0 ? x - alpha : x;                     // v = x - alpha e1, v'v = 2 (s + |x0| ||x||): no cancellation
        const double beta = 1.0 / (s + fabs(x0) * nrm);                  // 2 / v'v
        if (wave == 0) {
            S.v[lane] = vi;
            if (lane == 0) { S.d[k] = S.G[k * TR_PITCH + k]; S.e[k] = alpha; }
        }
        __syncthreads();
        double acc = 0.0;
        if (lane < m) {
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const int j = 16 * wave + jj;
                if (j < m) acc += S.G[(k + 1 + lane) * TR_PITCH + k + 1 + j] * S.v[j];
            }
        }
        S.part[wave * TR_N + lane] = acc;
        __syncthreads();
        const double pi = beta * ((S.part[lane] + S.part[TR_N + lane]) + (S.part[2 * TR_N + lane] + S.part[3 * TR_N + lane]));
        const double kk = 0.5 * beta * train_wsum(pi * vi);
        const double wi = pi - kk * vi;
        if (wave == 0) S.w[lane] = wi;
        __syncthreads();
        if (lane < m) {
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const int j = 16 * wave + jj;
                if (j < m) S.G[(k + 1 + lane) * TR_PITCH + k + 1 + j] -= vi * S.w[j] + wi * S.v[j];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        S.d[n - 2] = S.G[(n - 2) * TR_PITCH + n - 2];
        S.e[n - 2] = S.G[(n - 1) * TR_PITCH + n - 2];
        S.d[n - 1] = S.G[(n - 1) * TR_PITCH + n - 1];
    }
    __syncthreads();
    if (tid < n - 1) S.e2[tid] = S.e[tid] * S.e[tid];
    // ---- Gershgorin interval of the tridiagonal matrix (every lane for itself)
    double lo = INFINITY, hi = -INFINITY, emax2 = 0.0;
    for (int i = 0; i < TR_N; ++i) {
        if (i < n) {
            const double el = i > 0 ? fabs(S.e[i - 1]) : 0.0, er = i < n - 1 ? fabs(S.e[i]) : 0.0;
            lo = fmin(lo, S.d[i] - (el + er));
            hi = fmax(hi, S.d[i] + (el + er));
            emax2 = fmax(emax2, er * er);
        }
    }
    __syncthreads();
    if (hi <= 0.0) return 0.0;                                           // a Gram matrix without a positive bound: W = 0
    const double pivmin = DBL_MIN * fmax(1.0, emax2);
    {
        const double widen = 2.0 * n * DBL_EPSILON * fmax(fabs(lo), fabs(hi)) + 2.0 * pivmin;
        lo -= widen;
        hi += widen;
    }
    // ---- multisection: lane t counts the eigenvalues below x_t = lo + (hi - lo) t / 256; lambda_max >= x_t where fewer than n lie below.
    // The number of such lanes (not the index of the last one) picks the next interval: a count that is not monotone costs nothing.
    for (int round = 0; round < TR_ROUNDS; ++round) {
        const double x = lo + (hi - lo) * (tid * (1.0 / 256.0));
        double q = S.d[0] - x;
        if (fabs(q) < pivmin) q = -pivmin;
        int below = q < 0.0;
        for (int i = 1; i < TR_N; ++i) {
            if (i < n) {
                q = S.d[i] - x - S.e2[i - 1] / q;
                if (fabs(q) < pivmin) q = -pivmin;
                below += q < 0.0;
            }
        }
        int c = __syncthreads_count(below < n);
        c = c < 1 ? 1 : c;
        const double nlo = lo + (hi - lo) * ((c - 1) * (1.0 / 256.0)), nhi = c == 256 ? hi : lo + (hi - lo) * (c * (1.0 / 256.0));
        lo = nlo;
        hi = nhi;
    }
    return sqrt(fmax(0.5 * (lo + hi), 0.0));
}

// Adam on parameter j; ss = lr / (1 - beta1^t), bc2 = sqrt(1 - beta2^t).  Every operation is a separately rounded IEEE fp64 one (no fused
// multiply-add): at beta1 = 0.9 a fifth of a percent of the exact values of m lie so close to a float32 tie that a fused rounding decides
// the float32 result (measured against the float64 reference) -- the step is meant to be reproducible from its formula, operation by operation.
__device__ __forceinline__ void train_adam(const TrainArgs &A, int j, double ss, double bc2)
{
#pragma clang fp contract(off)
    const double g = (double)A.g[j];
    const float mf = (float)(A.b1 * (double)A.m[j] + (1.0 - A.b1) * g);
    const float vf = (float)(A.b2 * (double)A.v[j] + (1.0 - A.b2) * (g * g));
    A.m[j] = mf;
    A.v[j] = vf;
    A.w[j] = (float)((double)A.w[j] - ss * ((double)mf / (sqrt((double)vf) / bc2 + A.eps)));
}

template <bool ADAM>
__global__ __launch_bounds__(256) void mlp_train_kernel(TrainArgs A)
{
    __shared__ TrainLds S;
    const int l = (int)blockIdx.x, tid = (int)threadIdx.x;
    const TrainLayer L = train_layer(l);
    bool skipped = false;
    long long step = 0;
    unsigned scaled = 0;
    if (ADAM) {
        step = __hip_atomic_load(A.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int bad = 0;
        for (int i = tid; i < NDP_MLP_NPARAM; i += 256) bad |= (__float_as_uint(A.g[i]) & 0x7f800000u) == 0x7f800000u;   // NaN or infinite
        skipped = __syncthreads_or(bad) != 0;
        if (!skipped) {
            const double t = (double)(step + 1);
            const double bc1 = 1.0 - pow(A.b1, t), bc2 = sqrt(1.0 - pow(A.b2, t)), ss = A.lr / bc1;
            for (int i = tid; i < L.nw + L.nb; i += 256) train_adam(A, L.off + i, ss, bc2);
        }
        __syncthreads();             // the layer's new weights are read back below by other lanes
    }
    float *w = A.w + L.off;
    double sig = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        sig = train_sigma(w, L, S);
        if (!ADAM || pass == 1 || skipped || !(A.cap > 0.0 && sig > A.cap)) break;
        const double f = A.cap / sig;
        for (int i = tid; i < L.nw; i += 256) w[i] = (float)((double)w[i] * f);
        scaled = 1;
        __syncthreads();
    }
    if (tid == 0) {
        if (A.sigma) A.sigma[l] = sig;
        if (ADAM) {
            const unsigned old = atomicAdd(A.ticket, 1u + (scaled << (8 + l)));
            if ((old & 0xffu) == 3u) {                                   // the other three are done: theirs were the reads at entry
                if (A.info) {
                    A.info[0] = skipped ? 1 : 0;
                    A.info[1] = (int)((old >> 8) | (scaled << l));
                    A.info[2] = 0;
                    A.info[3] = 0;
                }
                if (!skipped) *A.step = step + 1;
                __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

}  // namespace ndp

using namespace ndp;

extern "C" {

int ndp_mlp_spectral_norms_device(ndp_handle *h, const void *d_w, void *d_sigma, void *stream)
{
    Entry g(h, d_w && d_sigma, stream);
    if (g.rc) return g.rc;
    TrainArgs a{};
    a.w = (float *)d_w;
    a.sigma = (double *)d_sigma;
    hipLaunchKernelGGL(mlp_train_kernel<false>, dim3(4), dim3(256), 0, g.s, a);
    NDP_HIP(h, hipGetLastError());
    return g.noted(0);
}

int ndp_mlp_spectral_norms(ndp_handle *h, const float *blob, double *sigma4)
{
    Entry g(h, blob && sigma4);
    if (g.rc) return g.rc;
    double *d_sigma = reinterpret_cast<double *>(reinterpret_cast<char *>(h->dTrain.get()) + 64);
    float *d_w = reinterpret_cast<float *>(d_sigma + 4);
    NDP_HIP(h, hipMemcpyAsync(d_w, blob, (size_t)NDP_MLP_NPARAM * 4, hipMemcpyHostToDevice, h->stream));
    TrainArgs a{};
    a.w = d_w;
    a.sigma = d_sigma;
    hipLaunchKernelGGL(mlp_train_kernel<false>, dim3(4), dim3(256), 0, h->stream, a);
    NDP_HIP(h, hipGetLastError());
    NDP_HIP(h, hipMemcpyAsync(sigma4, d_sigma, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return g.synced(0);
}

int ndp_mlp_adam_sn_device(ndp_handle *h, void *d_w, const void *d_g, void *d_m, void *d_v, void *d_step, double lr, double beta1,
                           double beta2, double eps, double sn_cap, void *d_sigma, void *d_info, int install, void *stream)
{
    Entry g(h, d_w && d_g && d_m && d_v && d_step, stream);
    if (g.rc) return g.rc;
    const char *why = nullptr;
    if (!std::isfinite(lr)) why = "ndp_mlp_adam_sn_device: lr must be finite";
    else if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) why = "ndp_mlp_adam_sn_device: beta1 and beta2 must lie in [0, 1)";
    else if (!(eps > 0.0)) why = "ndp_mlp_adam_sn_device: eps must be positive";
    else if (sn_cap != sn_cap) why = "ndp_mlp_adam_sn_device: sn_cap is NaN (<= 0 switches the cap off)";
    if (why) { h->err = why; return -2; }
    TrainArgs a{(float *)d_w, (const float *)d_g, (float *)d_m, (float *)d_v, (long long *)d_step, lr, beta1, beta2, eps, sn_cap,
                (double *)d_sigma, (int *)d_info, reinterpret_cast<unsigned *>(h->dTrain.get())};
    hipLaunchKernelGGL(mlp_train_kernel<true>, dim3(4), dim3(256), 0, g.s, a);
    NDP_HIP(h, hipGetLastError());
    const int rc = g.noted(0);
    if (rc || !install) return rc;
    g.lk.unlock();                   // (ndp_set_mlp_weights_device takes the handle's lock itself)
    return ndp_set_mlp_weights_device(h, d_w, stream);
}

}  // extern "C"
