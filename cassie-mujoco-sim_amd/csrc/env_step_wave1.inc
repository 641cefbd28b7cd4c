/* env_step, fragment: wave 1's program of the two-wave form (mass-matrix group, drive-level pass, factorisations, bias stage, sensor stage, the stages behind the solve).
 * Included by physics_kernel.h INSIDE the body of ck::env_step (one function, so that the register allocator sees one region): not a header of its own. */
    /* ---------------- two-wave form: wave 1's program ---------------- */
    if constexpr (NW == 2) {
        if (wid == 1) {
            for (int sub1 = sub_start;;) {
                /* this substep's constants are requested ahead of the barrier, where their trip through memory costs nothing */
                const int pb = isbody ? b : 0;
                const double mass = P->body_mass[pb];
                double iner[3], imat[9];
                for (int i = 0; i < 3; ++i) iner[i] = P->body_inertia[pb][i];
                for (int i = 0; i < 9; ++i) imat[i] = m->body_imat[pb][i];
                CK_STAMP(35);
                wv::block_barrier(); /* F: wave 0 has the poses, the inertial origins and the joint anchors / axes in LDS */
                if (wv::opaque(S.cmd[0])) return -1;
                wv::set_priority<(FEAT & FEAT_HFIELD) != 0 ? CK_PRIO_W1_FJ_HFIELD : CK_PRIO_W1_FJ>(); /* (F .. J: wave 0 needs what this wave makes about when it gets there -- later with a height-field pre-pass on its way) */
                CK_STAMP(36);
                double ximat[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
                if (isbody && b > 0) {
                    double xm[9];
                    for (int i = 0; i < 9; ++i) xm[i] = S.x.s.xmat[b][i];
                    for (int i = 0; i < 3; ++i)
                        for (int c = 0; c < 3; ++c) ximat[3 * i + c] = xm[3 * i] * imat[c] + xm[3 * i + 1] * imat[3 + c] + xm[3 * i + 2] * imat[6 + c];
                }
                double col[NVP], colh[NVP];
                mass_matrix_columns<NVP, TOPO, FEAT, NW>(io, S, m, env, ids, mass, iner, ximat, col, colh);
                /* X as two one-directional flags: com, cinert and cdof are in LDS and the buf tile is free again (wave 0's velocity
                 * stage waits for that); the factorisations -- which touch nothing wave 0's collision stage does -- do not wait for
                 * wave 0's collision verdict, only the drive-level pass (it changes the drive state) does */
                wv::publish(&S.cmd[3], sub1 + 1);
                CK_STAMP(38);
                factor_pair_by_height<NVP, TOPO, 0>(m, P, h, S, col, colh, lane); /* (that of M + hB: behind the barrier J) */
                /* The columns of M + hB wait for their factorisation behind J.  With 40 dofs and 256 registers they cannot wait in
                 * registers (80 of them, across the drive-level pass, the bias stage and the sensor stage: the model constants those
                 * stages request went to scratch one by one): they wait in LDS, in the slots their factor will take -- entry (i, j)
                 * of the lower triangle in the factor's slot (i, j), the diagonal in dinvH -- and come back behind J. */
                constexpr bool park_colh = NVP > 32;
                if constexpr (park_colh) {
                    if (isdof) {
#pragma unroll
                        for (int i = 0; i < NVP; ++i) {
                            if (i >= TOPO::nv) continue;
                            if (i == k_) S.dinvH[k_] = colh[i];
                            else if (i > k_ && LP::col_has(i, k_)) S.LHp[LP::col_idx(i, k_)] = colh[i]; /* (entries outside the slots are zero) */
                        }
                    }
                    wv::sync();
                }
                wv::wait_for(&S.cmd[4], sub1 + 1);
                if (wv::opaque(S.cmd[0])) return -1; /* (the row-capped instantiation hands this substep over) */
                if (io.drive_mode) {
                    if (integrates<FEAT>(io)) drive_level_io(io, S, m, env, lane, sub1 == nsub - 1);
                    wv::sync();
                }
                CK_STAMP(4);
                {
                    const int kd = isdof ? k_ : 0;
                    const double kdamp = P->dof_damping[kd], kstiff = PS->dof_stiffness[kd], kref = PS->dof_springref[kd];
                    const double kgear = m->dof_gear[kd], klo = m->dof_ctrl_lo[kd], khi = m->dof_ctrl_hi[kd];
                    const int kq = m->dof_qadr[kd], ka = m->dof_act[kd];
                    wv::wait_for(&S.cmd[1], sub1 + 1); /* wave 0's velocity stage has the body forces (cfrc) in LDS */
                    bias_forces_and_qfrc_smooth<NVP, FEAT, (NVP > 32)>(io, S, m, env, ids, kdamp, kstiff, kref, kgear, klo, khi, kq, ka);
                }
                /* (the sensor stage's constants: requested ahead of the barrier) */
                const bool lastsub1 = sub1 == nsub - 1 || !integrates<FEAT>(io);
                const bool need_imu1 = lastsub1 || io.all_outputs_every_substep || (io.drive_mode && sub1 + 2 == nsub);
                const bool issens1 = lane < m->nsensor && (lastsub1 || io.drive_mode || io.all_outputs_every_substep);
                const int ls1 = issens1 ? lane : 0;
                SensorConsts sens_c1;
                int aslot1;
                if constexpr (!sensors_behind_j) {
                    sens_c1 = request_sensor_consts(m, ls1);
                    /* the sensor stage, in the time this wave used to wait at J for wave 0's Jacobian rows: everything it reads is in LDS
                     * (poses since F, body velocities and bias accelerations since cmd[1]) and its own drive-level pass has read the
                     * previous substep's sensor words */
                    aslot1 = sensors_before_solve(io, S, m, env, issens1, ls1, sens_c1, need_imu1, lastsub1);
                }
                CK_STAMP(47);
                wv::block_barrier(); /* J: the factor of M and qfrc_smooth are in LDS (and, where the sensor stage runs in front: it is done with the body tiles) */
                if constexpr (!sensors_behind_j) wv::set_priority<CK_PRIO_W1_JP>(); /* (J .. P: this wave has the length of wave 0's solve for the factor of M + hB and its staging) */
                CK_STAMP(39);
                if constexpr (sensors_behind_j) {
                    /* the sensor stage BEHIND J, beside wave 0's half solve: whichever wave reaches J last, the other one waits for it, and
                     * in front of J the sensor stage made this wave the late one that much more often -- a wait on wave 0's critical path,
                     * while this wave has the length of wave 0's solve to spare behind J.  Everything the stage reads is still in LDS:
                     * wave 0's half solve works in registers and first writes into the body tiles' region with its staging store, in front
                     * of which it waits for cmd[6].  Wave 0 is waiting for this stage soon, so it runs at this wave's F .. J priority. */
                    sens_c1 = request_sensor_consts(m, ls1);
                    aslot1 = sensors_before_solve(io, S, m, env, issens1, ls1, sens_c1, need_imu1, lastsub1);
                    wv::publish(&S.cmd[6], sub1 + 1); /* the body tiles are wave 0's: the staged matrix may overwrite them */
                    wv::set_priority<CK_PRIO_W1_JP>();
                    /* (the profiled forms: the stage's length from the stamp behind J, in the upper half of slot 15 -- pk_types.h) */
                    if constexpr (feat_prof(FEAT)) { if (io.prof && lane == 0) ((int *)&io.prof[(size_t)env * NSTAMP + 15])[1] = (int)(wv::clock() - io.prof[(size_t)env * NSTAMP + 39]); }
                }
                if constexpr (WIDE) {
                    /* the 127-row instantiation: this wave's rows 64 .. 126 and the qfrc_smooth column (wide_solve); its row forces
                     * go to LDS for the barrier P like wave 0's */
                    int it1 = 0, ng1 = 0;
                    const double f1 = wide_solve<NVP, TOPO>(S, m, P, 1, wv::opaque(S.x.turn[0]), sub1, it1, ng1);
                    (&S.c_solimp[0][0])[NROW + lane] = f1;
                }
                /* the factorisation of M + hB, which only this wave's Euler step reads: here, in the time this wave would otherwise
                 * wait for wave 0's solve, instead of on the way to the barrier J, where wave 0 waited for it (+4.6 %) */
                if constexpr (park_colh) {
#pragma unroll
                    for (int i = 0; i < NVP; ++i) {
                        double v = 0.0;
                        if (i < TOPO::nv && isdof) {
                            if (i == k_) v = S.dinvH[k_];
                            else if (i > k_ && LP::col_has(i, k_)) v = S.LHp[LP::col_idx(i, k_)];
                        }
                        colh[i] = v;
                    }
                    wv::sync();
                }
                factor_pair_by_height<NVP, TOPO, 1>(m, P, h, S, col, colh, lane);
                /* ---- the stages behind wave 0's constraint solve: operands staged now, while wave 0 assembles and solves ---- */
                {
                    const bool lastsub = lastsub1, need_imu = need_imu1;
                    const int sb = sens_c1.sb, aslot = aslot1;
                    const int pf_u = lane < nu ? lane : 0, pf_ej = lane < njnt ? lane : 0;
                    const double pf_agear = m->act_gear[pf_u], pf_kdamp = P->dof_damping[isdof ? k_ : 0];
                    const int pf_adof = m->act_dofid[pf_u], pf_ejt = m->jnt_type[pf_ej], pf_eqa = m->jnt_qposadr[pf_ej], pf_eda = m->jnt_dofadr[pf_ej];
                    const double *const fbuf = &S.c_solimp[0][0];
                    double lrow[NVP];
                    constexpr bool stage_h_early = NVP <= 32;
                    if constexpr (stage_h_early) stage_factor_row<NVP, TOPO>(S, k_, isdof, lrow);
                    /* ... and its column of the factor of M + hB (this wave formed it right behind J): the Euler step's first
                     * substitution then starts without the column's 32 address computations and reads in front of it */
                    double lcol[NVP], lrowh[NVP];
                    /* (the 40-dof instantiation at 256 registers cannot hold its row of L, this column and -- from the qacc stage on -- the row of
                     * the factor of M + hB at once: 240 registers, which went to scratch and came back on the tail; there every operand
                     * is fetched right in front of its use, 120 LDS reads on the tail instead) */
                    if constexpr (stage_h_early) stage_factor_h<NVP, TOPO, 0>(S, k_, isdof, nv, lcol, lrowh);
                    const double rsdk = isdof ? S.rsd[k_] : 0.0;
                    const int kk = isdof ? k_ : 0;
                    /* this lane's column of the staged matrix (row MAXR = the qfrc_smooth column), once wave 0 has put it in LDS: the
                     * row-capped instantiation keeps it in registers across wave 0's solve, the full one reads it at its use */
                    constexpr bool stage_y = MAXR <= 31;
                    double ycolk[stage_y ? MAXR + 1 : 1];
                    if constexpr (stage_y) {
                        wv::wait_for(&S.cmd[2], sub1 + 1);
#pragma unroll
                        for (int r = 0; r <= MAXR; ++r) ycolk[r] = S.x.Yr[r][kk];
                    }
                    wv::block_barrier(); /* P: wave 0's row forces and solver statistics are in LDS */
                    wv::set_priority<CK_PRIO_W1_PE>(); /* (P .. E: wave 0 waits for this wave) */
                    const double f = fbuf[lane], f_hi = WIDE ? fbuf[NROW + lane] : 0.0; /* (rows 64 .. 126 of the 127-row instantiation) */
                    constexpr int FB = WIDE ? 2 * NROW : NROW;
                    const int ncon = (int)fbuf[FB], nefc = (int)fbuf[FB + 1], iters = (int)fbuf[FB + 2], nguarded = (int)fbuf[FB + 3];
                    /* ================= qacc = L^-1 D^-1/2 (y63 + Y f)  (lane = dof) ================= */
                    double z, z1 = 0, z2 = 0, z3 = 0;
                    if constexpr (stage_y) {
                        /* (the summation order of the one-wave form's loop: rows four to a group into four partial sums, the rows of
                         * the last, partial group into the first) */
                        z = isdof ? ycolk[MAXR] : 0.0;
#pragma unroll
                        for (int r = 0; r < MAXR; r += 4) {
                            if (r + 4 <= nefc) {
                                z += ycolk[r] * wv::readlane(f, r); z1 += ycolk[r + 1 < MAXR ? r + 1 : r] * wv::readlane(f, r + 1);
                                z2 += ycolk[r + 2 < MAXR ? r + 2 : r] * wv::readlane(f, r + 2); z3 += ycolk[r + 3 < MAXR ? r + 3 : r] * wv::readlane(f, r + 3);
                            } else {
#pragma unroll
                                for (int j = 0; j < 4; ++j) if (r + j < nefc && r + j < MAXR) z += ycolk[r + j < MAXR ? r + j : r] * wv::readlane(f, r + j);
                            }
                        }
                    } else {
                        z = isdof ? S.x.Yr[MAXR][k_] : 0.0;
                        /* (row r's force: lane r of f, or -- rows 64 .. 126 of the 127-row instantiation -- lane r - 64 of f_hi) */
                        auto frow = [&](int r) { if constexpr (WIDE) return r < NROW ? wv::readlane(f, r) : wv::readlane(f_hi, r - NROW); else return wv::readlane(f, r); };
                        int r = 0;
                        for (; r + 4 <= nefc; r += 4) {
                            const double y0 = S.x.Yr[r][kk], y1 = S.x.Yr[r + 1][kk], y2 = S.x.Yr[r + 2][kk], y3 = S.x.Yr[r + 3][kk];
                            z += y0 * frow(r); z1 += y1 * frow(r + 1);
                            z2 += y2 * frow(r + 2); z3 += y3 * frow(r + 3);
                        }
                        for (; r < nefc; ++r) z += S.x.Yr[r][kk] * frow(r);
                    }
                    z = (z + z1) + (z2 + z3);
                    if (!isdof) z = 0.0;
                    if (isdof) z *= rsdk;
                    /* (the Euler step's operands are requested here: their LDS latency runs under the substitution below) */
                    if constexpr (stage_h_early) stage_factor_h<NVP, TOPO, 1>(S, k_, isdof, nv, lcol, lrowh); /* (the row: its registers were the staged column of Y until here) */
                    const double dih = isdof ? S.dinvH[k_] : 0.0;
                    if constexpr (!stage_h_early) stage_factor_row<NVP, TOPO>(S, k_, isdof, lrow);
                    wv::sched_fence();
                    const double qacc = solve_forward<NVP, TOPO>(z, lrow, lane, nv);
                    {
                        const bool badv = isdof && (!(qacc == qacc) || fabs(qacc) > 1e10);
                        if (wv::ballot(badv) != 0ull) { /* diverged: the state stays as it is, wave 0 raises the flag */
                            if (lane == 0) S.cmd[0] = 2;
                            wv::block_barrier(); /* E */
                            return -1;
                        }
                    }
                    if (isdof) S.qacc[k_] = qacc;
                    const double av = pf_agear * S.qvel[pf_adof]; /* (the actuator velocity of the state the substep started from) */
                    wv::sync();
                    CK_STAMP(12);
                    /* Euler first: wave 0's next substep waits for qpos / qvel / the warm start only, so the barrier E sits right
                     * behind them and the substep's outputs -- the accelerometers (they read qacc, the partials parked in S.accel and
                     * cdof, none of which wave 0 touches before the next barrier F), the actuator velocities, the last substep's
                     * stores -- run beside wave 0's guard and kinematics stage instead of in front of them */
                    if (integrates<FEAT>(io)) {
                        if constexpr (!stage_h_early) stage_factor_h<NVP, TOPO>(S, k_, isdof, nv, lcol, lrowh);
                        euler_step<NVP, TOPO>(S, m, lane, isdof, k_, nv, njnt, h, qacc, lcol, lrowh, dih, pf_kdamp, pf_ejt, pf_eqa, pf_eda);
                    }
                    CK_STAMP(13);
                    wv::block_barrier(); /* E: the state of the next substep is in LDS (qpos / qvel / warm start) */
                    wv::set_priority<CK_PRIO_W1_EF>(); /* (the outputs, then the wait at F) */
                    outputs_after_qacc(io, S, m, env, lane, isdof, k_, nu, qacc, aslot, sb, need_imu, lastsub, av, ncon, nefc, iters, nguarded);
                    CK_STAMP(14);
                }
                if (!integrates<FEAT>(io) || ++sub1 >= nsub) return -1;
            }
        }
    }

