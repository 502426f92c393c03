"""Builds the gfx950 shared library in-tree (hipcc cross-compiles without a GPU): one object per translation unit, then one link.

    python -m ndp_nmpc_qd_amd.build [-o LIB] [extra hipcc flags]      (always rebuilds every unit)
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libndp_nmpc_hip.so")
# the translation units (csrc/host.hpp: which one owns what); rti_kernels.hip first, it is by far the longest compile
UNITS = ["rti_kernels.hip", "ndp_hip.hip", "downwash.hip", "rows.hip", "tick.hip", "exchange.hip", "mlp_vjp.hip", "mlp_jvp.hip", "mlp_train.hip",
         "mlp_fit.hip", "plant_deriv.hip", "plant_force_deriv.hip", "closed_loop.hip"]
HOST_ONLY = {"tick.hip"}      # units without a kernel: compiled for the host only, so that no empty code object goes into the library
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))) + [os.path.join("..", "..", "include", "ndp_nmpc.h")]   # every header a unit can include
# -amdgpu-mfma-vgpr-form: MFMA results go straight to VGPRs.  With the default AGPR form every accumulator that is
# live across a basic block or feeds VALU/LDS is copied through v_accvgpr_read/write behind full-latency s_nops,
# which serialised the matrix pipe against the VALU in the Riccati sweep.
# -amdgpu-schedule-relaxed-occupancy: the scheduler does not trade instruction order for an occupancy target these kernels cannot
# reach anyway (one wave per SIMD by LDS): MLP tile 8.45 k -> 8.30 k cycles, headline +0.6 % (round 5, A/B on one box).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-mllvm", "-amdgpu-schedule-relaxed-occupancy=true", "-fPIC"]


def _mtime(p):
    return os.path.getmtime(p) if os.path.exists(p) else -1.0


def build(force=False, verbose=False, out=LIB, extra=()):
    """hipcc --offload-arch=gfx950 -> `out` (default ndp_nmpc_qd_amd/libndp_nmpc_hip.so).  The objects go to the git-ignored
    ndp_nmpc_qd_amd/build/<name of out>/; a unit is recompiled when its source or any header is newer than its object, or when the
    flags (NDP_EXTRA_HIPCC_FLAGS, `extra`) differ from the last build's.  At most 16 compiles run at once (fewer if MAX_JOBS says so)."""
    flags = FLAGS + os.environ.get("NDP_EXTRA_HIPCC_FLAGS", "").split() + list(extra)
    odir = os.path.join(HERE, "build", os.path.splitext(os.path.basename(out))[0])
    os.makedirs(odir, exist_ok=True)
    stamp = os.path.join(odir, "flags")
    if not os.path.exists(stamp) or open(stamp).read() != " ".join(flags):
        force = True
    t_hdr = max(_mtime(os.path.join(CSRC, f)) for f in HEADERS)
    objs = [os.path.join(odir, os.path.splitext(u)[0] + ".o") for u in UNITS]
    todo = [(u, o) for u, o in zip(UNITS, objs) if force or _mtime(o) < max(t_hdr, _mtime(os.path.join(CSRC, u)))]

    def compile_unit(job):
        u, o = job
        cmd = ["hipcc"] + flags + (["--cuda-host-only"] if u in HOST_ONLY else []) + ["-c", "-o", o, os.path.join(CSRC, u)]
        if verbose:
            print(" ".join(cmd), flush=True)
        return subprocess.run(cmd, cwd=CSRC).returncode

    if todo:
        if os.path.exists(stamp):
            os.remove(stamp)         # (a failed or interrupted build leaves no stamp: the next one recompiles everything)
        jobs = max(1, min(16, len(todo), int(os.environ.get("MAX_JOBS") or 16)))
        with ThreadPoolExecutor(jobs) as ex:
            failed = [u for (u, _), rc in zip(todo, ex.map(compile_unit, todo)) if rc != 0]
        if failed:
            raise subprocess.CalledProcessError(1, "hipcc " + " ".join(failed))
        with open(stamp, "w") as fh:
            fh.write(" ".join(flags))
    if todo or _mtime(out) < max(_mtime(o) for o in objs):
        cmd = ["hipcc", "-shared", "-o", out] + objs       # (the objects carry their device code: the link takes no compile flags)
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out = LIB
    if args[:1] == ["-o"]:
        out, args = os.path.abspath(args[1]), args[2:]
    print(build(force=True, verbose=True, out=out, extra=args))
