// rti_kernel_body.inc -- the statements of the control-step kernels rti_kernel, rti_sens_kernel and rti_psens_kernel (rti_kernels.hip), included INSIDE
// their function bodies.  A device function both kernels call, however much inlined, reorders the kernels' code a little; the text
// itself, compiled in each kernel's own body, gives rti_kernel exactly the code it had before rti_sens_kernel existed.
// In scope where it is included: the template parameters NSLOT, WAVES, FUSED, NC, PREC, NRC, QMODE, TICK, the constants SENS and PSENS,
// the kernel argument `ka`, the sensitivity arguments `sa` (SensArgs; used only when SENS) and `pa` (PSensArgs; used only when PSENS), the
// dynamic LDS `smem` and the word `wg_done`.
    static_assert(!(FUSED && QMODE == 2), "the consumer reads the force the producer left in global memory");
    static_assert(!TICK || (QMODE <= 1 && NC > 0 && PREC == 0), "the one-launch tick exists for the compile-time horizon's in-place and producer forms");
#ifndef NDP_NO_KERNARG_WARM
    {   // The argument block is ~1.2 KB = 19 scalar-cache lines, and the compiler fetches each field next to its first use, waiting for it
        // there: every first touch of a line is a memory round trip of its own, one behind the other through the whole prologue.
        // One dword of every line, requested together at the very top: one round trip, the later fetches hit the scalar cache.
        typedef const __attribute__((address_space(4))) unsigned *kptr;
        kptr kp = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
        unsigned acc = 0;
#pragma unroll
        for (unsigned o = 0; o < (unsigned)sizeof(KernArgs); o += 64) acc |= kp[o / 4];
        asm volatile("" : : "s"(acc));
    }
#endif
    const RtiParams &P = ka.P;
    const BatchPtrs &bp = ka.bp;
    const MlpArgs &ma = ka.ma;
    const QueueArgs &qa = ka.qa;
    const int B = ka.B;
    const int wave = (int)(threadIdx.x >> 6);
    if (!FUSED && (QMODE == 0 || QMODE == 3) && ka.la.proto) {
        if (threadIdx.x == 0) wg_done = 0;
        __syncthreads();             // (before any wave of a ragged last workgroup leaves)
    }
    int inst_raw = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WAVES + wave);
    if (QMODE == 2) {         // list entry -> instance; past the end of the list: nothing to do
        const int n = (int)*qa.count;
        if (inst_raw >= n) return;
        inst_raw = __builtin_amdgcn_readfirstlane(qa.ids[inst_raw]);
    }
    const bool active = inst_raw < B;
    if (!FUSED && !active) return;
    const int inst = active ? inst_raw : B - 1;   // fused: idle waves of the last workgroup still take part in the barriers
    const int N = NC ? NC : P.N;
    const size_t nf = (size_t)(N + 1) * 3;
    RtiIo io;
    bind_instance(io, bp, inst, N);
    if (NSLOT <= 3 && (QMODE == 0 || QMODE == 3)) io.ipm_ctr = qa.ipm_total;
    if (NSLOT <= 3 && QMODE != 2 && blockIdx.x == 0 && threadIdx.x == 0 && qa.ipm_total)
        __hip_atomic_fetch_add(qa.ipm_total + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!FUSED && (QMODE == 0 || QMODE == 3) && ka.la.proto) {
        // this launch is control step number t; its force was written into slot t & 1 by downwash launch t
        const LateArgs &la = ka.la;
        const unsigned long long t = la.proto[PF_RTI_C2] / la.groups_rti + 1;       // (plain load: see LateArgs)
        const unsigned g = blockIdx.x % la.groups_rti;
        const unsigned np1 = (unsigned)N + 1, row0 = (unsigned)inst * np1;
        io.f_late = la.F[t & 1] + (size_t)inst * nf;
        io.late_flag = la.proto + PF_EPOCH + (t & 1) * la.ntiles + row0 / 32;
        io.late_flag2 = la.proto + PF_EPOCH + (t & 1) * la.ntiles + (row0 + np1 - 1) / 32;
        io.late_want = t;
        io.late_ready = la.proto[PF_MLP_DONE] >= t ? 1 : 0;                         // (plain load)
        io.late_timeout_us = la.timeout_us;
        io.late_missed = reinterpret_cast<int *>(la.proto + PF_MISSED);
        io.late_slow = reinterpret_cast<int *>(la.proto + PF_SLOW);
        io.late_cnt = reinterpret_cast<unsigned *>(la.proto + PF_RTI_C1 + PF_STRIDE * g);
        io.late_done_word = la.proto + PF_RTI_C2;
        io.late_gsize = pf_group_size(gridDim.x, la.groups_rti, g);
        // (LDS offset + 1: the word may well sit at offset 0, and null means "no workgroup-level counter")
        io.late_group = (void *)((size_t)(unsigned)(size_t)(__attribute__((address_space(3))) unsigned *)&wg_done + 1);
        const int left = B - (int)blockIdx.x * WAVES;
        io.late_group_size = (unsigned)(left < WAVES ? left : WAVES);
    }
    const int lpw = NC ? ((lds_doubles(NC) + 1) & ~1) : ka.lds_per_wave;
    WaveGfx950::lds_ptr lds = (WaveGfx950::lds_ptr)(smem + (size_t)wave * lpw);
    // PREC 0: the product path (f64 matrix instruction); 1 / 2: operand-rounding studies on it; 3 / 4: the sweeps on the real
    // fp32 / bf16-input matrix instructions (BASELINE config 5)
    using WB = std::conditional_t<PREC == 3, WaveGfx950F32, std::conditional_t<PREC == 4, WaveGfx950BF16, WaveGfx950>>;
    // PREC 5 / 6: config 5's CONDENSED study (cond_qp.hpp) -- the f64 program with every QP's first solve in condensed form on the fp32 / bf16 instructions
    using Prog = RtiWave<WB, NSLOT, NC, true, NRC, (PREC >= 3 ? 0 : PREC), QMODE == 3, (PREC == 5 ? 1 : (PREC == 6 ? 2 : 0))>;   // compile-time horizon and iteration count (NC = 0: both at run time)
    if (NDP_RARELY(io.stamps && (threadIdx.x & 63u) == 0)) {    // profiling hook: real time (100 MHz) and shader clock at entry -> the clock the launch ran at
        io.stamps[12] = (double)__builtin_amdgcn_s_memrealtime();
        io.stamps[14] = (double)__builtin_amdgcn_s_memtime();
    }
    // fused, neighbour rows picked through other_index: the row number is the head of a dependent load chain (index -> window
    // address -> window loads).  Fetch it before anything else is in the wave's in-order load queue and consume it here, so
    // that the one unavoidable wait covers one load, not the seventeen input loads requested next.
    // wg_nb: does ANY instance of this workgroup have a neighbour?  (Four scalar loads of the workgroup's own index entries, the
    // same in every wave: no barrier.)  A workgroup of plain NMPC followers -- a rank's local order puts them behind its leaders,
    // dist.config4_gids -- then skips the 70 KB weight transfer, both barriers and the network's input loads altogether.
    int orow = inst;
    bool wg_nb = true;
    if (FUSED && ma.other_index) {
        int any = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int iw = (int)blockIdx.x * WAVES + w;
            any |= (ma.other_index[iw < B ? iw : B - 1] >= 0) ? 1 : 0;
        }
        orow = __builtin_amdgcn_readfirstlane(ma.other_index[inst]);
        asm volatile("" : : "s"(orow));
        wg_nb = __builtin_amdgcn_readfirstlane(any) != 0;
    }
    const bool advance = TICK && ka.ta.advance != 0;
    TickEarly te;                            // (left as it is without `advance`: nothing looks at it then)
    if (TICK && NDP_RARELY(io.stamps && (threadIdx.x & 63u) == 0)) io.stamps[16] = (double)__builtin_amdgcn_s_memtime();   // neighbour index known
    if (TICK && advance) {
        te = tick_early(ka.ta, inst, FUSED && wg_nb ? orow : -1, (int)(threadIdx.x & 63u));
        __builtin_amdgcn_sched_barrier(0);   // (these two loads lead the wave's in-order load queue)
    }
    if (TICK && NDP_RARELY(io.stamps && (threadIdx.x & 63u) == 0)) io.stamps[22] = (double)__builtin_amdgcn_s_memtime();   // cache loads issued
    typename Prog::InBuf inb;
    double x0v;
    Prog::issue_first(P, io, inb, x0v);      // every global input of the RTI step is now in flight (hidden under the MLP when fused)
    __builtin_amdgcn_sched_barrier(0);       // do not let the scheduler sink those loads behind the MLP
    if (TICK && NDP_RARELY(io.stamps && (threadIdx.x & 63u) == 0)) io.stamps[23] = (double)__builtin_amdgcn_s_memtime();   // input loads issued
    // TICK: the newest list entry of this vehicle (x_new / u_new) and the position / velocity part of the neighbour's (nb_new).  Row N of
    // both windows is NOT read from the list in this launch (the neighbour's wave writes its entry while this one runs): the ego's goes
    // into the staged window through RtiIo::xrN, the pair into the network's input below.
    double x_new[10], u_new[4], nb_new[6], seg_fill = 0.0, seg_cfill = 0.0;
    int seg_refill = 0;
    if (TICK && !(FUSED && wg_nb) && advance) {      // (fused with neighbours: made below, under the weight transfer)
        tick_arrived(te);
        seg_fill = tick_new_point(ka.ta, te, inst, (int)(threadIdx.x & 63u), active, x_new, u_new, nb_new, seg_refill, seg_cfill, io.stamps);
#pragma unroll
        for (int i = 0; i < 10; ++i) io.xrN[i] = x_new[i];
        io.have_xrN = 1;
    }
    if (FUSED && !wg_nb) {          // no instance of the workgroup has a neighbour: zero force, nothing of the network runs
        if (!active) return;
        const int lane = (int)(threadIdx.x & 63u);
        const LdsMap m = make_map(N);
        if (lane < 3 * (N + 1)) {
            lds[m.TF + lane] = 0.0;
            ma.force_out[inst * nf + lane] = 0.0f;
        }
        if (3 * (N + 1) > 64 && lane + 64 < 3 * (N + 1)) {
            lds[m.TF + lane + 64] = 0.0;
            ma.force_out[inst * nf + lane + 64] = 0.0f;
        }
        WaveGfx950::sync();
        io.f = nullptr;
        io.f_in_lds = 1;
    } else if (FUSED) {
        const int lane = (int)(threadIdx.x & 63u), j = lane & 31, h = lane >> 5;
        const int np1 = N + 1;
        const int st = ma.other_stride;
        const double *oth = ma.other + (size_t)(orow < 0 ? 0 : orow) * ma.other_pitch;
        // the gate's four numbers are only REQUESTED here; the comparison comes after the barrier (consuming them here would
        // park the wave on the whole in-order load queue -- s_waitcnt vmcnt(0) -- before the weight transfer is even issued)
        const double *exy = ma.ego_xy ? ma.ego_xy + (size_t)inst * ma.ego_pitch : oth;
        const int osys = ma.other_sys;
        const double g_ox = ld_other(oth, osys), g_oy = ld_other(oth + 1, osys), g_ex = exy[0], g_ey = exy[1];
        const int jr = j < np1 ? j : np1 - 1;
        float zb[3], o[3];
        // Network input (downwash_nn.py:22-23): columns 0..5 of (other - ego reference), rows 0..N, subtracted in fp64.  Lane
        // (j, h) of the tile wants row j, columns 2s + h -- read that way it is an 8-byte load at an 80-byte lane stride (ten
        // cache lines per quarter wave, six instructions).  Instead ONE 16-byte load per array covers a row's six columns with
        // three adjacent lanes (lane l: row l / 3, columns 2 (l % 3), 2 (l % 3) + 1: 63 lanes for N = 20), and the tile's
        // layout is made by a cross-lane gather of the fp32 differences (ds_bpermute: the LDS crossbar, no LDS storage).
        typedef double d2_t __attribute__((ext_vector_type(2)));
        constexpr int ZR = NC ? (3 * (NC + 1) + 63) / 64 : 2;      // load rounds: 3 (N+1) lanes, N + 1 <= 32
        d2_t dv[ZR], ev[ZR];
#pragma unroll
        for (int t = 0; t < ZR; ++t) {
            const int l3 = lane + 64 * t, r3 = l3 / 3, c3 = l3 - 3 * r3, rc = r3 < np1 ? r3 : np1 - 1;
            dv[t] = ld_other2(oth + (size_t)rc * st + 2 * c3, osys);
            ev[t] = *(const d2_t *)(io.xr + (size_t)rc * NX + 2 * c3);
        }
        const LdsMap m = make_map(N);
        if (NDP_RARELY(io.dbg && lane == 0)) io.dbg[m.total + 9] = (double)__builtin_amdgcn_s_memtime();
        if (NDP_RARELY(io.stamps && lane == 0)) io.stamps[9] = (double)__builtin_amdgcn_s_memtime();
        // the whole workgroup's LDS is still unused: park the weight fragments there for the MLP phase
        lds_f32 wl = (lds_f32)smem;
        if (TICK) tick_arrived(te);               // (see there: the one wait of the prologue, in FRONT of the weight transfer; not under
                                                  // `advance`: a path around it leaves the values pending in the compiler's books)
        stage_fragments(ma.frag, wl, (int)threadIdx.x, 64 * WAVES);
        if (TICK && advance) {                    // the polynomial work runs while the weights stream into LDS
            seg_fill = tick_new_point(ka.ta, te, inst, lane, active, x_new, u_new, nb_new, seg_refill, seg_cfill, io.stamps);
#pragma unroll
            for (int i = 0; i < 10; ++i) io.xrN[i] = x_new[i];
            io.have_xrN = 1;
#pragma unroll
            for (int t = 0; t < ZR; ++t) {        // row N of the network's input: the two new entries (downwash_nn.py:22: columns 0..5)
                const int l3 = lane + 64 * t, r3 = l3 / 3, c3 = l3 - 3 * r3;
                if (r3 == N) {
                    dv[t][0] = c3 == 0 ? nb_new[0] : (c3 == 1 ? nb_new[2] : nb_new[4]);
                    dv[t][1] = c3 == 0 ? nb_new[1] : (c3 == 1 ? nb_new[3] : nb_new[5]);
                    ev[t][0] = c3 == 0 ? x_new[0] : (c3 == 1 ? x_new[2] : x_new[4]);
                    ev[t][1] = c3 == 0 ? x_new[1] : (c3 == 1 ? x_new[3] : x_new[5]);
                }
            }
        }
        __syncthreads();
        const double g_o[2] = {g_ox, g_oy}, g_e[2] = {g_ex, g_ey};
        const bool open = orow >= 0 && (ma.ego_xy ? gate_open(g_o, g_e, ma.r2) : true);
        {
            float fx[ZR], fy[ZR];
#pragma unroll
            for (int t = 0; t < ZR; ++t) { fx[t] = (float)(dv[t][0] - ev[t][0]); fy[t] = (float)(dv[t][1] - ev[t][1]); }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int src = 3 * jr + s, sl = (src & 63) << 2;
                float vx = __int_as_float(__builtin_amdgcn_ds_bpermute(sl, __float_as_int(fx[0])));
                float vy = __int_as_float(__builtin_amdgcn_ds_bpermute(sl, __float_as_int(fy[0])));
                if (ZR > 1) {
                    const float wx = __int_as_float(__builtin_amdgcn_ds_bpermute(sl, __float_as_int(fx[ZR - 1])));
                    const float wy = __int_as_float(__builtin_amdgcn_ds_bpermute(sl, __float_as_int(fy[ZR - 1])));
                    if (src >= 64) { vx = wx; vy = wy; }
                }
                zb[s] = h ? vy : vx;
            }
        }
        if (NDP_RARELY(io.stamps && lane == 0)) io.stamps[11] = (double)__builtin_amdgcn_s_memtime();
        // gate closed (or no neighbour): the force is zero and the reference does not evaluate the network either
        // (ndp_nmpc_leader_node.py:66-76).  The test is the same in every lane: a wave-uniform branch around the tile.
        o[0] = o[1] = o[2] = 0.0f;
        if (__builtin_amdgcn_readfirstlane((int)open)) mlp_tile(wl, zb, lane, o);
        __syncthreads();                              // every wave is done with the weights before LDS becomes RTI state
        if (!active) return;
        if (NDP_RARELY(io.dbg && lane == 0)) io.dbg[m.total + 10] = (double)__builtin_amdgcn_s_memtime();
        if (NDP_RARELY(io.stamps && lane == 0)) io.stamps[10] = (double)__builtin_amdgcn_s_memtime();
        if (j < np1 && h == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = open ? o[c] : 0.0f;      // ndp_nmpc_leader_node.py:75-76
                lds[m.TF + j * 3 + c] = (double)v;       // fp32 value promoted to fp64 (SURVEY B11)
                ma.force_out[inst * nf + j * 3 + c] = v; // also what the consumer launch of the work list reads
            }
        }
        WaveGfx950::sync();
        io.f = nullptr;
        io.f_in_lds = 1;
    }
    if (TICK && advance && active) tick_cache_store(ka.ta, te, inst, (int)(threadIdx.x & 63u), seg_refill, seg_fill, seg_cfill);   // (requested in the prologue: long there)
    if (TICK && ka.ta.est && active) io.kthr = tick_estimator(ka.ta, inst, B, (int)(threadIdx.x & 63u));
    bool deferred;
    if constexpr (SENS) {
        // the instance's views of the sensitivity outputs (QMODE 2: the listed instance this wave solves)
        const SensIo so{sa.du0 + (size_t)inst * sens_u0_pitch(), sa.dU ? sa.dU + (size_t)inst * sens_u_pitch(N) : nullptr,
                        sa.dX ? sa.dX + (size_t)inst * sens_x_pitch(N) : nullptr, sa.level};
        if constexpr (PSENS) {
            // ... and of its parameter outputs (rti_psens_kernel)
            const PSensIo po{pa.dxr + (size_t)inst * psens_xr_pitch(N), pa.dur + (size_t)inst * psens_ur_pitch(N), pa.df + (size_t)inst * psens_f_pitch(N)};
            deferred = Prog::template run<QMODE == 1, QMODE == 0 || QMODE == 3, true, true>(P, io, lds, inb, x0v, &so, &po);
        } else {
            deferred = Prog::template run<QMODE == 1, QMODE == 0 || QMODE == 3, true>(P, io, lds, inb, x0v, &so);
        }
    } else {
        deferred = Prog::template run<QMODE == 1, QMODE == 0 || QMODE == 3>(P, io, lds, inb, x0v);
    }
    if (NDP_RARELY(io.stamps && (threadIdx.x & 63u) == 0)) {
        io.stamps[13] = (double)__builtin_amdgcn_s_memrealtime();
        io.stamps[15] = (double)__builtin_amdgcn_s_memtime();
    }
    if (QMODE == 1 && deferred && (threadIdx.x & 63u) == 0) {
        const unsigned s = __hip_atomic_fetch_add(qa.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        qa.ids[s] = inst;
    }
