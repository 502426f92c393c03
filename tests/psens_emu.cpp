// psens_emu.cpp -- the control step with its initial-state and parameter sensitivities (RtiWave::run<..., SENS, PSENS>, RtiWave::psens_out)
// on the host wave emulator, one instance per call.  TEST INFRASTRUCTURE ONLY: compiled by tests/test_param_sensitivity.py into a temporary
// directory (tests/emu/ is left as it is).
#include <vector>

#include "emu/wave_emu.hpp"
#include "../ndp_nmpc_qd_amd/csrc/cfg_params.hpp"

template <class Prog>
static void run_psens(const ndp::RtiParams &P, ndp::RtiIo &io, double *lds, const ndp::SensIo &so, const ndp::PSensIo &po)
{
    typename Prog::InBuf inb;
    emu::vd x0v;
    Prog::issue_first(P, io, inb, x0v);
    Prog::template run<false, false, true, true>(P, io, lds, inb, x0v, &so, &po);
}

extern "C" {

// act: the instance's kept active set (ndp::act_pitch(N) bytes), in and out; du0 [4][10]; dxr [4][N+1][10], dur [4][N][4], df [4][N+1][3]
int psens_emu_step(const ndp_cfg *cfg, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                   double *u0, int *status, int *iters, signed char *act, double *du0, double *dxr, double *dur, double *df)
{
    ndp::RtiParams P = ndp::to_params(*cfg);
    if (P.n_rti != 1 || cfg->qp_precision != 0 || ndp::slots_for(P.N) > 3) return -1;
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
    const ndp::SensIo so{du0, nullptr, nullptr, 1};
    const ndp::PSensIo po{dxr, dur, df};
    // as the device runs them: N = 20 the compile-time horizon with host-built tables, other horizons the run-time form
    if (P.N == 20) run_psens<ndp::RtiWave<emu::Wave, 3, 20, true, 1>>(P, io, lds.data(), so, po);
    else run_psens<ndp::RtiWave<emu::Wave, 3, 0, true>>(P, io, lds.data(), so, po);
    return 0;
}
}
