// step_jvp_emu.cpp -- the control step with its forward-mode derivative (RtiWave::run<..., JVP>, jvp_out) on the host wave emulator, one
// instance and T directions per call.  TEST INFRASTRUCTURE ONLY: compiled by tests/step_jvp_emu.py into a temporary directory.
// The set-up (parameters, NaN-poisoned LDS, constants, index tables) is step_deriv_emu.cpp's, taken as it is by including that file: this
// library then holds its entries too (vjp_emu_step: the duality test runs both derivatives from one library).
#include "step_deriv_emu.cpp"

namespace {

template <class Prog>
void run_jvp(Setup &s, const ndp::JvpIo &jo)
{
    typename Prog::InBuf inb;
    emu::vd x0v;
    Prog::issue_first(s.P, s.io, inb, x0v);
    Prog::template run<false, false, false, false, false, false, true>(s.P, s.io, s.lds.data(), inb, x0v, nullptr, nullptr, nullptr, nullptr, &jo);
}

}  // namespace

extern "C" {

// X, U, act: the tape, advanced in place as the step does; T directions tx0 [T][10], txr [T][N+1][10], tur [T][N][4], tf [T][N+1][3] (any
// may be null); du0 [T][4], dX [T][N+1][10], dU [T][N][4] (any may be null)
int jvp_emu_step(const ndp_cfg *cfg, int T, const double *x0, const double *xr, const double *ur, const float *f, double *X, double *U,
                 double *u0, int *status, int *iters, signed char *act, const double *tx0, const double *txr, const double *tur,
                 const double *tf, double *du0, double *dX, double *dU)
{
    Setup s;
    if (T < 1 || !setup(s, cfg, x0, xr, ur, f, X, U, u0, status, iters, act)) return -1;
    const ndp::JvpIo jo{tx0, txr, tur, tf, du0, dX, dU, T};
    if (s.P.N == 20) run_jvp<ndp::RtiWave<emu::Wave, 3, 20, true, 1>>(s, jo);     // as the device runs them (step_deriv_emu.cpp: run)
    else run_jvp<ndp::RtiWave<emu::Wave, 3, 0, true>>(s, jo);
    return 0;
}
}
