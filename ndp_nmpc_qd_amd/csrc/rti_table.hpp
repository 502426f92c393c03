// rti_table.hpp -- the rows of the control-step kernel table (rti_kernels.hip: k_rti, one kernel per row, in this order).  Host code
// outside that unit names a control-step kernel by its row only (ndp_hip.hip: rti_pick -> launch_kern); bit RtiId of
// ndp_debug_rti_launched's mask is the row, and _lib.rti_kernel_names reads the names from here.
#pragma once

enum RtiId {
    K3_4, K3_2, K3_1, K5_4, K5_2, K5_1, K3F_4, K3F_2, K3F_1,         // any horizon: 3 / 5 slots, fused downwash; 4, 2, 1 instances per group
    K20, K20F, K20_W2, K20F_W2,                                       // the reference shape (N = 20, one RTI iteration)
    K20_PROD, K20F_PROD, K20_CONS, K20_LATE,                          // ... work-list producer / consumer, late-force step
    K20F_TICK, K20_TICK, K20F_PROD_TICK, K20_PROD_TICK,               // ... one-launch ticks
    KPREC1, KPREC2, KPREC3, KPREC4, KPREC5, KPREC6,                   // precision studies, any horizon, one wave per group
    K40_F32, K40_BF16, K40, K40_PROD, K40_CONS,                       // BASELINE config 5's shape (N = 40, two RTI iterations)
    S20F_PROD, S20_PROD, S20_CONS, S20F, S20, SF_4, S_4, SF_2, S_2,   // sensitivities (three slots)
    P20F_PROD, P20_PROD, P20_CONS, P20F, P20, PF_4, PF_2,              // ... with parameter sensitivities (no unfused run-time horizon)
    RTI_KERNELS
};
