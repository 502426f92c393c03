// step_model_jvp_emu.cpp -- the control step with its forward mode along directions of the cost weights and the mass on the host wave
// emulator, one instance per call (RtiWave::run<..., JVP, MJVP>, jvp_out<true>; T directions per call), as rti_mjvp_kernel runs it.
// TEST INFRASTRUCTURE ONLY: compiled by tests/step_model_jvp_emu.py into a temporary directory (tests/emu/ is left as it is).
#include <vector>

#include "emu/wave_emu.hpp"
#include "../ndp_nmpc_qd_amd/csrc/cfg_params.hpp"

namespace {

template <class Prog>
void run_prog(const ndp::RtiParams &P, const ndp::RtiIo &io, std::vector<double> &lds, const ndp::JvpIo &jo)
{
    typename Prog::InBuf inb;
    emu::vd x0v;
    Prog::issue_first(P, io, inb, x0v);
    Prog::template run<false, false, false, false, false, false, true, true>(P, io, lds.data(), inb, x0v, nullptr, nullptr, nullptr, nullptr, &jo);
}

}  // namespace

extern "C" {

// X, U, act: the tape (the iterate and kept set before the step), advanced in place as the step does; T directions tx0 [T][10],
// txr [T][N+1][10], tur [T][N][4], tf [T][N+1][3] (any may be null), tmodel [T][16] (required); du0 [T][4], dX [T][N+1][10], dU [T][N][4]
// (any may be null)
int mjvp_emu_step(const ndp_cfg *cfg, int T, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                  double *u0, int *status, int *iters, signed char *act, const double *tx0, const double *txr, const double *tur,
                  const double *tf, const double *tmodel, double *du0, double *dX, double *dU)
{
    const ndp::RtiParams P = ndp::to_params(*cfg);
    if (T < 1 || !tmodel || P.n_rti != 1 || cfg->qp_precision != 0 || ndp::slots_for(P.N) > 3) return -1;
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
    const ndp::JvpIo jo{tx0, txr, tur, tf, du0, dX, dU, T, tmodel};
    // as the device runs them: N = 20 the compile-time horizon with host-built tables, other horizons the run-time form
    if (P.N == 20) run_prog<ndp::RtiWave<emu::Wave, 3, 20, true, 1>>(P, io, lds, jo);
    else run_prog<ndp::RtiWave<emu::Wave, 3, 0, true>>(P, io, lds, jo);
    return 0;
}
}
