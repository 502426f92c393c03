// mlp_vjp_back.inc -- one round of the backward pass behind the forward (mlp_vjp_body.inc and mlp_fit_rows_kernel include this text): weight path
// and data path from d4 down to d1 and dW1.  Expects the names of mlp_vjp_body.inc: buf, mine, fr, frt, tile_open, want_w, d4, zb, a2, a3, dl, g*, gb*.
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
