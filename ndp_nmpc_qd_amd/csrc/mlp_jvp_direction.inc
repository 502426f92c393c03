// mlp_jvp_direction.inc -- one direction through the four layers: the inside of the T loop of mlp_jvp_kernel and mlp_jvp_multi_kernel
// (mlp_jvp.hip, which includes this text into both; a function around it changed the registers the compiler gives mlp_jvp_kernel, whose
// code object is held fixed).  Expects fr (the weights' records), tw (the direction of the weights or null), tzb[3] (this lane's share
// of dz), zb[3], a1[4], a2[2], a3[4] (the forward's input and activations), lane, j, h.  Leaves g[3] = df of the lane's row, complete
// on both half-waves; d1, d2, d3 and g are declared here (and acc, q, v, w4 in inner scopes: keep such names out of the including scope).
        // ---- layer 1: da1 = m1 (W1 dz + dW1 z + db1)
        f16_t d1[4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) {
            f16_t acc = jvp_dbias(tw ? tw + PB1 + ot * 32 : nullptr, h);
            JVP_FENCE();
#pragma unroll
            for (int s = 0; s < 3; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[frag::L1 + (ot * 3 + s) * 64 + lane], tzb[s], acc, 0, 0, 0);
            if (tw) {
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tw[PW1 + (ot * 32 + j) * 6 + 2 * s + h], zb[s], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) d1[ot][r] = jvp_mask_cap(a1[ot][r], acc[r]);
        }
        // ---- layer 2: da2 = m2 (W2 da1 + dW2 a1 + db2)
        f16_t d2[2];
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) {
            f16_t acc = jvp_dbias(tw ? tw + PB2 + ot * 32 : nullptr, h);
            jvp_dense(fr, ot * 8, 4, d1, lane, acc);
            if (tw) jvp_dweight(tw + PW2 + (ot * 32 + j) * 128 + 4 * h, 4, a1, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) d2[ot][r] = jvp_mask_cap(a2[ot][r], acc[r]);
        }
        // ---- layer 3: da3 = m3 (W3 da2 + dW3 a2 + db3), plain ReLU
        f16_t d3[4];
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) {
            f16_t acc = jvp_dbias(tw ? tw + PB3 + ot * 32 : nullptr, h);
            jvp_dense(fr, 16 + ot * 4, 2, d2, lane, acc);
            if (tw) jvp_dweight(tw + PW3 + (ot * 32 + j) * 64 + 4 * h, 2, a2, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) d3[ot][r] = a3[ot][r] > 0.0f ? acc[r] : 0.0f;
        }
        // ---- layer 4 on the VALU: df = W4 da3 + dW4 a3 + db4; each half-wave owns 64 of the 128 features of its row
        float g[3] = {0.0f, 0.0f, 0.0f};
        const f4_t *w4 = reinterpret_cast<const f4_t *>(fr + frag::W4);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            JVP_FENCE();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f4_t q = w4[it * 32 + f0(r) + 4 * h];
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = fmaf(q[c], d3[it][r], g[c]);
            }
        }
        if (tw) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                JVP_FENCE();
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f4_t v = ld4(tw + PW4 + c * 128 + it * 32 + 8 * q + 4 * h);
#pragma unroll
                        for (int i = 0; i < 4; ++i) g[c] = fmaf(v[i], a3[it][4 * q + i], g[c]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g[c] += __shfl_xor(g[c], 32, 64);
            if (tw) g[c] += tw[PB4 + c];
        }
