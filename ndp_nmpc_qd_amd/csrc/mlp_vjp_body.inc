// mlp_vjp_body.inc -- the body of mlp_vjp_kernel and mlp_vjp_multi_kernel (mlp_vjp.hip, which describes it and includes this text into
// both).  Expects the kernel argument `MlpVjpArgs A` and two macros: VJP_EGO, the instance whose ego window and ego xy a row reads, and
// VJP_FROW, the row of A.gf that is its upstream (size_t).
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

        // ---- layer 4: dW4 = d4 (x) a3, db4
        __syncthreads();                                   // (the previous round's reads of the image are over)
        if (lane == 0) ((__attribute__((address_space(3))) int *)(buf + VJ_FLAGS))[wave] = tile_open;
        if (tile_open && want_w) {
            if (h == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) mine[c * VJ_PITCH + j] = d4[c];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) park(mine, a3[t], 1 + t, lane);
        }
        __syncthreads();
        int opn[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) opn[w] = __builtin_amdgcn_readfirstlane(((const __attribute__((address_space(3))) int *)(buf + VJ_FLAGS))[w]);
        if (want_w) {
            contract(buf, opn, 0, wave, 32, 3, 32, -1, lane, g4);
            gb4 += bias_rows(buf, opn, 3, tid);
        }
        // d3 = (W4' d4) m3
        if (tile_open) {
            typedef float f4_t __attribute__((ext_vector_type(4)));
            const f4_t *w4 = reinterpret_cast<const f4_t *>(fr + frag::W4);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                VJP_FENCE();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const f4_t q = w4[t * 32 + f0(r) + 4 * h];
                    const float v = fmaf(q[2], d4[2], fmaf(q[1], d4[1], q[0] * d4[0]));
                    dl[t][r] = a3[t][r] > 0.0f ? v : 0.0f;
                }
            }
        }
        // ---- layer 3: dW3 = d3 (x) a2, db3
        __syncthreads();
        if (tile_open && want_w) {
#pragma unroll
            for (int t = 0; t < 4; ++t) park(mine, dl[t], t, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t) park(mine, a2[t], 4 + t, lane);
        }
        __syncthreads();
        if (want_w) {
            contract(buf, opn, wave, 0, 128, 32, 32, -1, lane, g3[0]);
            contract(buf, opn, wave, 1, 128, 32, 32, -1, lane, g3[1]);
            gb3 += bias_rows(buf, opn, 128, tid);
        }
        // d2 = (W3' d3) m2
        f16_t d2[2];
        if (tile_open) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                f16_t acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    VJP_FENCE();
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(frt[FRT_L3 + ((it * 4 + st) * 16 + r) * 64 + lane], dl[st][r], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) d2[it][r] = mask_cap(a2[it][r], acc[r]);
            }
        }
        // ---- layer 2: dW2 = d2 (x) a1, db2
        __syncthreads();
        if (tile_open) {                                   // (a1 also serves d1's mask below: parked whether or not dW is asked for)
#pragma unroll
            for (int t = 0; t < 2; ++t) park(mine, d2[t], t, lane);
#pragma unroll
            for (int t = 0; t < 4; ++t) park(mine, vjp_layer1(fr, zb, lane, t), 2 + t, lane);
        }
        __syncthreads();
        if (want_w) {
            contract(buf, opn, wave >> 1, 2 * (wave & 1), 64, 32, 32, -1, lane, g2[0]);
            contract(buf, opn, wave >> 1, 2 * (wave & 1) + 1, 64, 32, 32, -1, lane, g2[1]);
            gb2 += bias_rows(buf, opn, 64, tid);
        }
        // d1 = (W2' d2) m1
        if (tile_open) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                f16_t acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    VJP_FENCE();
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(frt[FRT_L2 + ((it * 2 + st) * 16 + r) * 64 + lane], d2[st][r], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) dl[it][r] = mask_cap(mine[((2 + it) * 32 + f0(r) + 4 * h) * VJ_PITCH + j], acc[r]);   // a1, this wave's own
            }
        }
        // ---- layer 1: dW1 = d1 (x) z, db1 (the column of ones behind z's six features)
        __syncthreads();
        if (tile_open && want_w) {
#pragma unroll
            for (int t = 0; t < 4; ++t) park(mine, dl[t], t, lane);
#pragma unroll
            for (int s = 0; s < 3; ++s) mine[(128 + 2 * s + h) * VJ_PITCH + j] = zb[s];
        }
        __syncthreads();
        if (want_w) contract(buf, opn, wave, 0, 128, 32, 6, 6, lane, g1);
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

    // ---- this workgroup's partial gradient, every entry written
    float *P = A.part + (size_t)blockIdx.x * PTOTAL;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = f0(r) + 4 * h;
        if (m < 3) P[PW4 + m * 128 + wave * 32 + j] = g4[r];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            P[PW3 + (wave * 32 + m) * 64 + t * 32 + j] = g3[t][r];
            P[PW2 + ((wave >> 1) * 32 + m) * 128 + (2 * (wave & 1) + t) * 32 + j] = g2[t][r];
        }
        if (j < 6) P[PW1 + (wave * 32 + m) * 6 + j] = g1[r];
        if (j == 6) P[PB1 + wave * 32 + m] = g1[r];
    }
    __syncthreads();
    buf[tid] = gb4; buf[256 + tid] = gb3; buf[512 + tid] = gb2;
    __syncthreads();
    if (tid < 3) P[PB4 + tid] = buf[tid] + buf[128 + tid];
    if (tid < 128) P[PB3 + tid] = buf[256 + tid] + buf[256 + 128 + tid];
    if (tid < 64) P[PB2 + tid] = buf[512 + tid] + buf[512 + 128 + tid];
