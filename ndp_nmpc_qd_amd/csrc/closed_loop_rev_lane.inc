// closed_loop_rev_lane.inc -- the lane body of closed_loop.hip's two reverse link kernels, included as text (as mlp_vjp_back.inc is): `a` the
// launch's ClRev, `v` the lane's vehicle (< a.p.B).  Two hooks, macros of the including kernel: CL_REV_INCOMING(v, lam) behind
// lam = gx_p + gx0 (the formation adds gx_f), CL_REV_FORCE(v, g0, g1, g2) behind the plant's force gradient (the formation hands
// gfps[k] + gfp_k to the force's adjoint).  closed_loop_rev_link_kernel defines both empty: its code is what it was before they existed.
    double lam[10], gk[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) lam[i] = 0.0;
    if (a.c_p) {
        plant_ld_row<5>(a.c_p + (size_t)v * 10, lam);
        plant_ld_row<5>(a.c_s + (size_t)v * 10, gk);
#pragma unroll
        for (int i = 0; i < 10; ++i) lam[i] = lam[i] + gk[i];
        CL_REV_INCOMING(v, lam)
    }
    double p15 = 0.0;
    const bool bad = a.st_prev && a.st_prev[v] != 0;
    if (bad && a.gfp_prev) {
        const double nan = __builtin_nan("");
        a.gfp_prev[(size_t)v * 3] = nan; a.gfp_prev[(size_t)v * 3 + 1] = nan; a.gfp_prev[(size_t)v * 3 + 2] = nan;
    }
    if (a.tail) {
        if (a.gx0) plant_st_row<5>(a.gx0 + (size_t)v * 10, lam);
    } else {
        double xin[10], y[10], uv[4], acc[3], guv[4] = {0.0, 0.0, 0.0, 0.0}, gacc[3] = {0.0, 0.0, 0.0};
        plant_ld_row<5>(a.xin + (size_t)v * 10, xin);
        plant_ld_row<2>(a.u + (size_t)v * 4, uv);
        if (a.gxs) {
            plant_ld_row<5>(a.gxs + (size_t)v * 10, gk);
#pragma unroll
            for (int i = 0; i < 10; ++i) lam[i] = gk[i] + lam[i];
        }
        plant_acc(a.fp, (size_t)v * 3, a.p.inv_mass, a.p.g, acc);
#pragma unroll
        for (int i = 0; i < 10; ++i) y[i] = xin[i];
        for (int s = 0; s < a.p.sub; ++s) plant_rk4(y, uv, acc, a.p.h);
        const double n = plant_renorm(y);                    // y[6..9]: the tick's output quaternion
        const double d = y[6] * lam[6] + y[7] * lam[7] + y[8] * lam[8] + y[9] * lam[9];
#pragma unroll
        for (int i = 6; i < 10; ++i) lam[i] = (lam[i] - y[i] * d) / n;
        for (int s = a.p.sub - 1; s >= 0; --s) {
#pragma unroll
            for (int i = 0; i < 10; ++i) y[i] = xin[i];
            for (int j = 0; j < s; ++j) plant_rk4(y, uv, acc, a.p.h);
            plant_rk4_vjp(y, uv, acc, a.p.h, lam, guv, gacc);
        }
        plant_st_row<5>(a.gxp + (size_t)v * 10, lam);
        if (a.gus) {
            double up[4];
            plant_ld_row<2>(a.gus + (size_t)v * 4, up);
#pragma unroll
            for (int i = 0; i < 4; ++i) guv[i] = up[i] + guv[i];
        }
        plant_st_row<2>(a.gu0 + (size_t)v * 4, guv);
        const double g0 = gacc[0] * a.p.inv_mass, g1 = gacc[1] * a.p.inv_mass, g2 = gacc[2] * a.p.inv_mass;
        if (a.gfp) { a.gfp[(size_t)v * 3] = g0; a.gfp[(size_t)v * 3 + 1] = g1; a.gfp[(size_t)v * 3 + 2] = g2; }
        CL_REV_FORCE(v, g0, g1, g2)
        if (a.fp) p15 = -a.p.inv_mass * (g0 * a.fp[(size_t)v * 3] + g1 * a.fp[(size_t)v * 3 + 1] + g2 * a.fp[(size_t)v * 3 + 2]);
    }
    if (a.gm_tot) {
        double tot[16], row[16];
        if (a.gm_row) {
            plant_ld_row<8>(a.gm_tot + (size_t)v * 16, tot);
            plant_ld_row<8>(a.gm_row + (size_t)v * 16, row);
#pragma unroll
            for (int i = 0; i < 15; ++i) tot[i] = tot[i] + row[i];
            tot[15] = bad ? __builtin_nan("") : tot[15] + p15;
        } else {
#pragma unroll
            for (int i = 0; i < 15; ++i) tot[i] = 0.0;
            tot[15] = p15;
        }
        plant_st_row<8>(a.gm_tot + (size_t)v * 16, tot);
    }
