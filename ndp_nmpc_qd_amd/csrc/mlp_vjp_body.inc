// mlp_vjp_body.inc -- the body of mlp_vjp_kernel and mlp_vjp_multi_kernel (mlp_vjp.hip, which describes it and includes this text into
// both).  Expects the kernel argument `MlpVjpArgs A` and two macros: VJP_EGO, the instance whose ego window and ego xy a row reads, and
// VJP_FROW, the row of A.gf that is its upstream (size_t).  Two spans of it are texts of their own, because mlp_fit_rows_kernel includes
// them too: mlp_vjp_back.inc (a round's backward pass) and mlp_vjp_part.inc (the partial gradient's way out).
    extern __shared__ __attribute__((aligned(16))) float vsm[];
    lds_f32 buf = (lds_f32)vsm;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = (A.rows + 31) / 32, ngroups = (ntiles + 3) / 4;
    const bool want_w = A.part != nullptr;
    lds_f32 mine = buf + wave * VJ_WAVE;

    // this wave's share of the weight gradient: dW4 tile (0, wave) | dW3 tiles (wave, 0..1) | dW2 tiles (wave >> 1, 2 (wave & 1) + 0..1) |
    // dW1 tile (wave, 0) with b1 in its column 6; the bias sums of layers 2..4 per thread (bias_rows)
    f16_t g4, g3[2], g2[2], g1;
#pragma unroll
    for (int r = 0; r < 16; ++r) g4[r] = g3[0][r] = g3[1][r] = g2[0][r] = g2[1][r] = g1[r] = 0.0f;
    float gb4 = 0.0f, gb3 = 0.0f, gb2 = 0.0f;

#pragma unroll 1
    for (int grp = (int)blockIdx.x; grp < ngroups; grp += (int)gridDim.x) {
        // (the weight records are the same in every round: keep the compiler from hoisting 17k loads out of the loop into registers)
        const float *fr = A.fr, *frt = A.frt;
        asm volatile("" : "+s"(fr), "+s"(frt));
        const int tile = grp * 4 + wave;
        const int row = tile * 32 + j;
        const bool valid = row < A.rows;
        const int rowc = valid ? row : A.rows - 1;
        const int inst = rowc / A.np1, k = rowc - inst * A.np1;
        const int orow = A.other_index ? A.other_index[inst] : inst;
        const double *oth = A.other + (size_t)(orow < 0 ? 0 : orow) * A.other_pitch;
        bool open = valid && orow >= 0;
        if (A.ego_xy) {
            const double oxy[2] = {ld_other(oth, A.other_sys), ld_other(oth + 1, A.other_sys)};
            open = open && gate_open(oxy, A.ego_xy + (size_t)VJP_EGO * A.ego_xy_pitch, A.r2);
        }
        const int tile_open = __builtin_amdgcn_readfirstlane((int)(__ballot(open) != 0ull));
        float d4[3] = {0.0f, 0.0f, 0.0f};
        bool finite = true;
        f16_t a2[2], a3[4], dl[4];
        float zb[3];
        if (tile_open) {
            if (open) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    d4[c] = (float)A.gf[VJP_FROW * 3 + c];
                    finite = finite && __builtin_isfinite(d4[c]);
                }
                // a row whose upstream gradient is not finite (a failed step's) adds nothing to the weights and gets NaN itself
                if (!finite) d4[0] = d4[1] = d4[2] = 0.0f;
            }
#pragma unroll
            for (int s = 0; s < 3; ++s)
                zb[s] = (float)(ld_other(oth + (size_t)k * A.other_stride + 2 * s + h, A.other_sys) -
                                A.ego[(size_t)VJP_EGO * A.ego_pitch + (size_t)k * NX + 2 * s + h]);
            vjp_forward(fr, zb, lane, a2, a3);
        }

#include "mlp_vjp_back.inc"
        // g_z = W1' d1
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
