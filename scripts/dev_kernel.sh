#!/bin/bash
# Kernel-development build: only the reference configuration's two rti_kernel instantiations (N = 20, 1 RTI iteration, fused /
# unfused), ~25 s instead of ~3 min.  Output ndp_nmpc_qd_amd/libndp_nmpc_hip_dev.so (git-ignored, travels with gpurun); use it
# with NDP_NMPC_LIB=$PWD/ndp_nmpc_qd_amd/libndp_nmpc_hip_dev.so.  Extra hipcc flags: "$@".  Every unit is built with the same
# flags (objects under ndp_nmpc_qd_amd/build/libndp_nmpc_hip_dev/); the collapse itself is in csrc/rti_kernels.hip (RTI_K).
set -e
cd "$(dirname "$0")/.."
python3 -m ndp_nmpc_qd_amd.build -o ndp_nmpc_qd_amd/libndp_nmpc_hip_dev.so -DNDP_DEV_HEADLINE_ONLY "$@"
