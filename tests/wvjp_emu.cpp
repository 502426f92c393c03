// wvjp_emu.cpp -- vjp_emu.cpp's sibling for the gradient in the cost weights and the mass (RtiWave::run<..., VJP, WVJP>,
// RtiWave::vjp_out<true>) on the host wave emulator, one instance per call.  TEST INFRASTRUCTURE ONLY: compiled by tests/test_model_grad.py
// into a temporary directory.
#include <vector>

#include "emu/wave_emu.hpp"
#include "../ndp_nmpc_qd_amd/csrc/cfg_params.hpp"

template <class Prog>
static void run_wvjp(const ndp::RtiParams &P, ndp::RtiIo &io, double *lds, const ndp::VjpIo &vo, double *gmodel)
{
    typename Prog::InBuf inb;
    emu::vd x0v;
    Prog::issue_first(P, io, inb, x0v);
    Prog::template run<false, false, false, false, true, true>(P, io, lds, inb, x0v, nullptr, nullptr, &vo, gmodel);
}

extern "C" {

// vjp_emu_step's arguments, then gmodel [16] = dL/dQd [10] | dL/dRd [4] | dL/dmass | 0
int wvjp_emu_step(const ndp_cfg *cfg, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                  double *u0, int *status, int *iters, signed char *act, const double *gu0, const double *gX, const double *gU,
                  double *gx0, double *gxr, double *gur, double *gf, double *gmodel)
{
    ndp::RtiParams P = ndp::to_params(*cfg);
    if (P.n_rti != 1 || cfg->qp_precision != 0 || ndp::slots_for(P.N) > 3 || !gmodel) return -1;
    const int n = ndp::lds_doubles(P.N);
    std::vector<double> lds((size_t)n, 0.0 / 0.0);   // NaN-poisoned: any read of unwritten LDS shows up
    emu::Wave::lds_limit() = n;
    double kc[ndp::KC_HOST];
    ndp::fill_kc(P, kc);
    ndp::RtiIo io{x0, xr, ur, f, X, U, u0, status, iters, nullptr, 0, kc};
    std::vector<int> tb(ndp::TB_WORDS);
    ndp::fill_tables(P.N, tb.data(), 0);
    io.tables = tb.data();
    io.act = act;
    const ndp::VjpIo vo{gu0, gX, gU, gx0, gxr, gur, gf};
    // as the device runs them: N = 20 the compile-time horizon with host-built tables, other horizons the run-time form
    if (P.N == 20) run_wvjp<ndp::RtiWave<emu::Wave, 3, 20, true, 1>>(P, io, lds.data(), vo, gmodel);
    else run_wvjp<ndp::RtiWave<emu::Wave, 3, 0, true>>(P, io, lds.data(), vo, gmodel);
    return 0;
}
}
