// mlp_vjp_part.inc -- the end of a backward kernel: the workgroup writes its partial gradient, every entry, to row blockIdx.x of A.part.
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
