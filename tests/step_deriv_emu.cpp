// step_deriv_emu.cpp -- the control step with each of its derivatives on the host wave emulator, one instance per call: the initial-state
// sensitivities (RtiWave::run<..., SENS>, sens_out), the parameter sensitivities (<..., SENS, PSENS>, psens_out), the adjoint of its QP
// (<..., VJP>, vjp_out), the adjoint with the gradient in the cost weights and the mass (<..., VJP, WVJP>, vjp_out<true>) and forward mode
// (<..., JVP>, jvp_out; T directions per call).
// TEST INFRASTRUCTURE ONLY: compiled by tests/step_deriv_emu.py into a temporary directory (tests/emu/ is left as it is).
#include <vector>

#include "emu/wave_emu.hpp"
#include "../ndp_nmpc_qd_amd/csrc/cfg_params.hpp"

namespace {

// what every entry sets up: the parameters, NaN-poisoned LDS, the constants and index tables, the instance's pointers
struct Setup {
    ndp::RtiParams P;
    std::vector<double> lds;
    double kc[ndp::KC_HOST];
    std::vector<int> tb;
    ndp::RtiIo io;
};

// false: a shape the derivative kernels do not serve
bool setup(Setup &s, const ndp_cfg *cfg, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
           double *u0, int *status, int *iters, signed char *act)
{
    s.P = ndp::to_params(*cfg);
    if (s.P.n_rti != 1 || cfg->qp_precision != 0 || ndp::slots_for(s.P.N) > 3) return false;
    const int n = ndp::lds_doubles(s.P.N);
    s.lds.assign((size_t)n, 0.0 / 0.0);   // NaN-poisoned: any read of unwritten LDS shows up
    emu::Wave::lds_limit() = n;
    ndp::fill_kc(s.P, s.kc);
    s.io = ndp::RtiIo{x0, xr, ur, f, X, U, u0, status, iters, nullptr, 0, s.kc};
    s.tb.resize(ndp::TB_WORDS);
    ndp::fill_tables(s.P.N, s.tb.data(), 0);
    s.io.tables = s.tb.data();
    s.io.act = act;
    return true;
}

template <class Prog, bool SENS, bool PSENS, bool VJP, bool WVJP, bool JVP>
void run_prog(Setup &s, const ndp::SensIo *so, const ndp::PSensIo *po, const ndp::VjpIo *vo, double *gmodel, const ndp::JvpIo *jo)
{
    typename Prog::InBuf inb;
    emu::vd x0v;
    Prog::issue_first(s.P, s.io, inb, x0v);
    Prog::template run<false, false, SENS, PSENS, VJP, WVJP, JVP>(s.P, s.io, s.lds.data(), inb, x0v, so, po, vo, gmodel, jo);
}

// as the device runs them: N = 20 the compile-time horizon with host-built tables, other horizons the run-time form
template <bool SENS, bool PSENS, bool VJP, bool WVJP, bool JVP = false>
void run(Setup &s, const ndp::SensIo *so, const ndp::PSensIo *po, const ndp::VjpIo *vo, double *gmodel, const ndp::JvpIo *jo = nullptr)
{
    if (s.P.N == 20) run_prog<ndp::RtiWave<emu::Wave, 3, 20, true, 1>, SENS, PSENS, VJP, WVJP, JVP>(s, so, po, vo, gmodel, jo);
    else run_prog<ndp::RtiWave<emu::Wave, 3, 0, true>, SENS, PSENS, VJP, WVJP, JVP>(s, so, po, vo, gmodel, jo);
}

}  // namespace

extern "C" {

// act: the instance's kept active set (ndp::act_pitch(N) bytes), in and out; du0 [4][10], dU [N][4][10], dX [N+1][10][10] (level 2)
int sens_emu_step(const ndp_cfg *cfg, int level, const double *x0, const double *xr, const double *ur, const float *f,
                  double *X, double *U, double *u0, int *status, int *iters, signed char *act, double *du0, double *dU, double *dX)
{
    Setup s;
    if (!setup(s, cfg, x0, xr, ur, f, X, U, u0, status, iters, act)) return -1;
    const ndp::SensIo so{du0, dU, dX, level};
    run<true, false, false, false>(s, &so, nullptr, nullptr, nullptr);
    return 0;
}

// act as above; du0 [4][10]; dxr [4][N+1][10], dur [4][N][4], df [4][N+1][3]
int psens_emu_step(const ndp_cfg *cfg, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                   double *u0, int *status, int *iters, signed char *act, double *du0, double *dxr, double *dur, double *df)
{
    Setup s;
    if (!setup(s, cfg, x0, xr, ur, f, X, U, u0, status, iters, act)) return -1;
    const ndp::SensIo so{du0, nullptr, nullptr, 1};
    const ndp::PSensIo po{dxr, dur, df};
    run<true, true, false, false>(s, &so, &po, nullptr, nullptr);
    return 0;
}

// X, U, act: the tape (the iterate and kept set before the step), advanced in place as the step does; gu0 [4], gX [N+1][10], gU [N][4]
// (any may be null); gx0 [10], gxr [N+1][10], gur [N][4], gf [N+1][3]
int vjp_emu_step(const ndp_cfg *cfg, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                 double *u0, int *status, int *iters, signed char *act, const double *gu0, const double *gX, const double *gU,
                 double *gx0, double *gxr, double *gur, double *gf)
{
    Setup s;
    if (!setup(s, cfg, x0, xr, ur, f, X, U, u0, status, iters, act)) return -1;
    const ndp::VjpIo vo{gu0, gX, gU, gx0, gxr, gur, gf};
    run<false, false, true, false>(s, nullptr, nullptr, &vo, nullptr);
    return 0;
}

// vjp_emu_step's arguments, then gmodel [16] = dL/dQd [10] | dL/dRd [4] | dL/dmass | 0
int wvjp_emu_step(const ndp_cfg *cfg, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                  double *u0, int *status, int *iters, signed char *act, const double *gu0, const double *gX, const double *gU,
                  double *gx0, double *gxr, double *gur, double *gf, double *gmodel)
{
    Setup s;
    if (!gmodel || !setup(s, cfg, x0, xr, ur, f, X, U, u0, status, iters, act)) return -1;
    const ndp::VjpIo vo{gu0, gX, gU, gx0, gxr, gur, gf};
    run<false, false, true, true>(s, nullptr, nullptr, &vo, gmodel);
    return 0;
}

// X, U, act: the tape, advanced in place as the step does; T directions tx0 [T][10], txr [T][N+1][10], tur [T][N][4], tf [T][N+1][3] (any
// may be null); du0 [T][4], dX [T][N+1][10], dU [T][N][4] (any may be null)
int jvp_emu_step(const ndp_cfg *cfg, int T, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                 double *u0, int *status, int *iters, signed char *act, const double *tx0, const double *txr, const double *tur,
                 const double *tf, double *du0, double *dX, double *dU)
{
    Setup s;
    if (T < 1 || !setup(s, cfg, x0, xr, ur, f, X, U, u0, status, iters, act)) return -1;
    const ndp::JvpIo jo{tx0, txr, tur, tf, du0, dX, dU, T};
    run<false, false, false, false, true>(s, nullptr, nullptr, nullptr, nullptr, &jo);
    return 0;
}
}
