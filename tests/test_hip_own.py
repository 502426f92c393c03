"""csrc/hip_own.hpp, the owners of the handle's device buffers, page-locked blocks, events and streams, on the CPU: tests/hip_own_check.cpp
(stand-ins for the HIP calls, its own main) is compiled with the ROCm clang under AddressSanitizer (leak check included) and
UndefinedBehaviorSanitizer and run as a child process.  No HIP runtime is linked and nothing is loaded into this interpreter: exit status 0
and a silent sanitizer are the assertion."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_owners_release_everything_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "hip_own_check")
    cmd = [os.path.join(ROCM, "llvm", "bin", "clang++"), "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
           "-I" + os.path.join(ROOT, "ndp_nmpc_qd_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tests", "hip_own_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert "live counter 0" in run.stdout
