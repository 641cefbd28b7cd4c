/* env_step, fragment: P5 constraint rows -- descriptors, geometry, impedance, Jacobian rows (in two passes in the 127-row instantiation), barrier J, read-outs.
 * Included by physics_kernel.h INSIDE the body of ck::env_step (one function, so that the register allocator sees one region): not a header of its own. */
        /* ================= P5 constraint rows: lane = row ================= */
        /* row descriptor assignment is wave-uniform bookkeeping; every lane keeps its own row */
        /* (The 127-row instantiation forms its rows in TWO PASSES of this wave -- rows 0 .. 63, then, if the substep has them, rows
         * 64 .. 126 -- and parks every row's raw Jacobian row and solver parameters in LDS (x.Yr, x.rowt); behind the barrier J each
         * wave picks up its 64 rows from there: wide_solve.  Every other instantiation runs the loop below once.) */
        int r_ = lane;
        int rtype = -1, rid = 0, rsub = 0;
        int nefc = 0, nefc_before_contacts = 0;
        double rpos = 0, rmargin = 0, rR = 1.0, rK = 0, rB = 0, rimp = 1.0;
        const bool need_imu = lastsub || io.all_outputs_every_substep || (io.drive_mode && sub + 2 == nsub);
        const bool need_pos = lastsub || io.drive_mode || io.all_outputs_every_substep;
        const bool issens = lane < m->nsensor && need_pos;
        const int ls = issens ? lane : 0;
        SensorConsts sens_c;
        double ycol[NVP]; /* this lane's Jacobian row, one dof at a time, straight into registers; lane 63 carries qfrc_smooth */
        double jvel = 0, jws = 0;
        const bool lastcol = !WIDE && lane == NROW - 1;
        for (int pass = 0; pass < (WIDE ? 2 : 1); ++pass) {
        if constexpr (WIDE) {
            if (pass == 1 && nefc <= NROW) break; /* (wave-uniform: no second pass) */
            r_ = NROW * pass + lane; rtype = -1; rid = 0; rsub = 0; nefc = 0; jvel = 0; jws = 0;
            rpos = 0; rmargin = 0; rR = 1.0; rK = 0; rB = 0; rimp = 1.0;
        }
        {
            /* all equalities active and within the cap (the usual case): three rows each, in order, in closed form */
            const int neq = m->neq;
            const bool eact = lane < neq && m->eq_active[lane < neq ? lane : 0] != 0;
            const unsigned long long eall = neq >= 64 ? ~0ull : (1ull << neq) - 1;
            if (wv::ballot(eact) == eall && 3 * neq <= capr) {
                if (r_ < 3 * neq) { rtype = CM_CNSTR_EQUALITY; rid = r_ / 3; rsub = r_ - 3 * rid; }
                nefc = 3 * neq;
            } else
            for (int e = 0; e < neq; ++e) {
                if (!m->eq_active[e]) continue;
                if (nefc + 3 > capr) { warn |= WARN_CONSTRAINT_FULL; continue; }
                if (r_ >= nefc && r_ < nefc + 3) { rtype = CM_CNSTR_EQUALITY; rid = e; rsub = r_ - nefc; }
                nefc += 3;
            }
        }
        {
            /* joint-limit rows in joint order, lower side before upper side (lob / hib: evaluated after the collision stage) */
            for (unsigned long long any = lob | hib; any; any &= any - 1) {
                const int j = wv::popc64((any & (0ull - any)) - 1);
                for (int side = 0; side < 2; ++side) {
                    if (!(((side == 0 ? lob : hib) >> j) & 1ull)) continue;
                    if (nefc >= capr) { warn |= WARN_CONSTRAINT_FULL; continue; }
                    if (r_ == nefc) { rtype = CM_CNSTR_LIMIT_JOINT; rid = j; rsub = side; }
                    ++nefc;
                }
            }
        }
        nefc_before_contacts = nefc;
        /* every contact a friction pyramid of four rows and all of them within the cap (the usual case): closed form */
        const bool cpyr = lane < ncon && S.c_dim[lane < ncon ? lane : 0] == 3;
        if (wv::ballot(cpyr) == (ncon >= 64 ? ~0ull : (1ull << ncon) - 1) && nefc + 4 * ncon <= capr) {
            if (r_ >= nefc && r_ < nefc + 4 * ncon) { rtype = CM_CNSTR_CONTACT_PYRAMIDAL; rid = (r_ - nefc) >> 2; rsub = (r_ - nefc) & 3; }
            nefc += 4 * ncon;
        } else
        for (int c = 0; c < ncon; ++c) {
            const int dim = S.c_dim[c];
            if (dim != 1 && dim != 3) { warn |= WARN_UNSUPPORTED_PAIR; continue; }
            const int nrow = dim == 1 ? 1 : 2 * (dim - 1);
            if (nefc + nrow > capr) { warn |= WARN_CONSTRAINT_FULL; continue; }
            if (r_ >= nefc && r_ < nefc + nrow) {
                rtype = dim == 1 ? CM_CNSTR_CONTACT_FRICTIONLESS : CM_CNSTR_CONTACT_PYRAMIDAL;
                rid = c; rsub = r_ - nefc;
            }
            nefc += nrow;
        }

        CK_STAMP(25);
        /* per-row geometry: J_rk = plus_k (u.lin_k + wp.ang_k) - minus_k (u.lin_k + wm.ang_k) (+ sgn at one dof) */
        double u3[3] = {0, 0, 0}, wp[3] = {0, 0, 0}, wm[3] = {0, 0, 0};
        unsigned long long maskp = 0, maskm = 0;
        int limdof = -1;
        double limsgn = 0, rdiag = 0, imp_pos = 0, rRscale = 1.0;
        double solref0 = 0.02, solref1 = 1, solimp[5] = {0.9, 0.95, 0.001, 0.5, 2};
        if (rtype == CM_CNSTR_EQUALITY) {
            if (rid != pf_eq) { /* (an inactive equality ahead of this one: the constants requested in advance are another row's) */
                pf_eb1 = m->eq_body1[rid]; pf_eb2 = m->eq_body2[rid]; pf_er1 = m->eq_root[rid][0]; pf_er2 = m->eq_root[rid][1];
            }
            maskp = m->eq_dofmask[rid][0]; maskm = m->eq_dofmask[rid][1];
            rdiag = P->eq_invweight[rid];
            solref0 = m->eq_solref[rid][0]; solref1 = m->eq_solref[rid][1];
            for (int i = 0; i < 5; ++i) solimp[i] = m->eq_solimp[rid][i];
            const int b1 = pf_eb1, b2 = pf_eb2;
            double l1[3] = {m->eq_data[rid][0], m->eq_data[rid][1], m->eq_data[rid][2]};
            double l2[3] = {m->eq_data[rid][3], m->eq_data[rid][4], m->eq_data[rid][5]};
            double a1[3], a2[3];
            mulmatvec3(a1, S.x.s.xmat[b1], l1);
            mulmatvec3(a2, S.x.s.xmat[b2], l2);
            for (int i = 0; i < 3; ++i) { a1[i] += S.x.s.xpos[b1][i]; a2[i] += S.x.s.xpos[b2][i]; }
            u3[0] = rsub == 0 ? 1.0 : 0.0; u3[1] = rsub == 1 ? 1.0 : 0.0; u3[2] = rsub == 2 ? 1.0 : 0.0;
            const double *c1 = S.com[pf_er1], *c2 = S.com[pf_er2];
            double o1[3] = {a1[0] - c1[0], a1[1] - c1[1], a1[2] - c1[2]};
            double o2[3] = {a2[0] - c2[0], a2[1] - c2[1], a2[2] - c2[2]};
            cross3(wp, o1, u3);
            cross3(wm, o2, u3);

            double res[3] = {a1[0] - a2[0], a1[1] - a2[1], a1[2] - a2[2]};
            rpos = rsub == 0 ? res[0] : (rsub == 1 ? res[1] : res[2]); rmargin = 0;
            imp_pos = sqrt(dot3(res, res));

        } else if (rtype == CM_CNSTR_LIMIT_JOINT) {
            const double q = S.qpos[m->jnt_qposadr[rid]];
            rpos = rsub == 0 ? q - m->jnt_range[rid][0] : m->jnt_range[rid][1] - q;
            rmargin = m->jnt_margin[rid];
            imp_pos = rpos;
            limdof = m->jnt_dofadr[rid];
            limsgn = rsub == 0 ? 1.0 : -1.0;
            rdiag = P->jnt_liminvweight[rid];
            solref0 = m->jnt_solref[rid][0]; solref1 = m->jnt_solref[rid][1];
            for (int i = 0; i < 5; ++i) solimp[i] = m->jnt_solimp[rid][i];
        } else if (rtype >= 0) {
            const int c = rid;
            const double *fr = S.c_frame[c];
            if (rtype == CM_CNSTR_CONTACT_PYRAMIDAL) {
                const int a = 1 + rsub / 2;
                const double mu = a <= 2 ? S.c_fri[c][0] : (a == 3 ? S.c_fri[c][1] : S.c_fri[c][2]);
                const double sg = (rsub & 1) ? -mu : mu;
                for (int i = 0; i < 3; ++i) u3[i] = fr[i] + sg * fr[3 * a + i];
                const double mu0 = S.c_fri[c][0];
                rRscale = 2 * mu0 * mu0; /* all pyramid rows use R of the first row, times 2 mu^2 */
            } else {
                for (int i = 0; i < 3; ++i) u3[i] = fr[i];
            }
            const double *c1 = S.com[S.c_root[c][0]], *c2 = S.com[S.c_root[c][1]];
            double o1[3] = {S.c_pos[c][0] - c1[0], S.c_pos[c][1] - c1[1], S.c_pos[c][2] - c1[2]};
            double o2[3] = {S.c_pos[c][0] - c2[0], S.c_pos[c][1] - c2[1], S.c_pos[c][2] - c2[2]};
            cross3(wp, o2, u3);
            cross3(wm, o1, u3);
            maskp = S.c_dofmask[c][1];
            maskm = S.c_dofmask[c][0];
            rpos = S.c_dist[c]; rmargin = S.c_margin[c]; imp_pos = rpos;
            const double tran = S.c_tran[c];
            const double mu_first = S.c_fri[c][0];
            rdiag = rtype == CM_CNSTR_CONTACT_PYRAMIDAL ? tran + mu_first * mu_first * tran : tran;
            solref0 = S.c_solref[c][0]; solref1 = S.c_solref[c][1];
            for (int i = 0; i < 5; ++i) solimp[i] = S.c_solimp[c][i];
        }
        CK_STAMP(26);
        if (rtype >= 0) {
            rimp = impedance(solimp, imp_pos, rmargin);
            rR = fmax(CM_MINVAL, (1 - rimp) * rdiag / rimp);
            if (rtype == CM_CNSTR_CONTACT_PYRAMIDAL) rR = fmax(CM_MINVAL, rRscale * rR);
            const double dmax = solimp[1];
            if (solref0 > 0) {
                double tc = solref0;
                if ((m->flags & CM_FLAG_REFSAFE) && tc < 2 * h) tc = 2 * h;
                rK = 1.0 / fmax(CM_MINVAL, dmax * dmax * tc * tc * solref1 * solref1);
                rB = 2.0 / fmax(CM_MINVAL, dmax * tc);
            } else {
                rK = -solref0 / fmax(CM_MINVAL, dmax * dmax);
                rB = -solref1 / fmax(CM_MINVAL, dmax);
            }
        }
        CK_STAMP(27);
        /* The constants of the sensor stage behind the Jacobian loop are requested here, every one of them in one level of
         * unconditional reads (lane = sensor): their round trip through the memory system runs under the loop instead of
         * in front of the sensors. */
        if constexpr (NW == 1) sens_c = request_sensor_consts(m, ls);
#pragma unroll
        for (int k0 = 0; k0 < NVP; k0 += 4) {
            /* stage four motion axes and the matching qvel / qacc_warmstart / qfrc_smooth entries, then compute */
            double cc[4][6], qv[4], qw[4], qs[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                for (int t = 0; t < 6; ++t) cc[kk][t] = S.cdof[k0 + kk][t];
                qv[kk] = S.qvel[k0 + kk]; qw[kk] = S.qacc_ws[k0 + kk];
                if constexpr (NW == 1) qs[kk] = S.qfrc_smooth[k0 + kk]; else qs[kk] = 0.0; /* (two-wave form: behind the barrier J) */
            }
            wv::sched_fence();
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = k0 + kk;
                double v = 0;
                if (TOPO::is_static ? k < TOPO::nv : k < nv) {
                    if (rtype >= 0) {
                        const double ul = u3[0] * cc[kk][3] + u3[1] * cc[kk][4] + u3[2] * cc[kk][5];
                        /* the two body-chain predicates applied by multiplication (exact: the factors are 0.0 / 1.0) */
                        const double sp = bitf(maskp, k), sm = bitf(maskm, k);
                        v = sp * (ul + wp[0] * cc[kk][0] + wp[1] * cc[kk][1] + wp[2] * cc[kk][2]) -
                            sm * (ul + wm[0] * cc[kk][0] + wm[1] * cc[kk][1] + wm[2] * cc[kk][2]);
                        if (k == limdof) v = limsgn;
                        jvel += v * qv[kk];
                        jws += v * qw[kk];
                    } else if (lastcol) {
                        v = qs[kk];
                    }
                }
                ycol[k] = v;
            }
        }
        if constexpr (WIDE) {
            /* the row goes to LDS: its raw Jacobian row (the half solve behind the barrier J takes it from there) and what the solve
             * needs of it -- R, the reference acceleration, J . qacc_warmstart, and 1 / 0 / -1 for clamped row / equality row / no row */
            if (r_ < MAXR) {
#pragma unroll
                for (int k = 0; k < NVP; ++k) S.x.Yr[r_][k] = ycol[k];
                double *rt = S.x.rowt[r_];
                rt[0] = rR; rt[1] = rtype >= 0 ? -rB * jvel - rK * rimp * (rpos - rmargin) : 0.0; rt[2] = jws;
                rt[3] = rtype < 0 ? -1.0 : (rtype == CM_CNSTR_EQUALITY ? 0.0 : 1.0);
            }
            if (readout_ext<FEAT>(io) && pass == 0 && rtype == CM_CNSTR_EQUALITY && r_ < CM_MAXEQROW) {
                cm_ext_t *ex = readout_ext<FEAT>(io) + env;
                ex->eq_pos[r_] = rpos; ex->eq_id[r_] = rid;
#pragma unroll
                for (int k = 0; k < NVP; ++k) if (k < nv) ex->eq_J[r_][k] = ycol[k];
            }
        }
        } /* (pass) */
        const int sb = NW == 1 ? sens_c.sb : 0;
        CK_STAMP(28);
        if constexpr (NW == 2) {
            /* J: wave 1 is done with this substep -- the factors of M and M + hB and qfrc_smooth are in LDS, and its drive-level pass
             * has read the previous substep's sensor words, which the sensor stage below replaces */
            if constexpr (WIDE) { if (lane == 0) S.x.turn[0] = nefc; } /* (wave 1 takes its rows by it) */
            CK_STAMP(34); wv::block_barrier();
            /* lane 63's column of the staged matrix is qfrc_smooth */
            if (lastcol) {
#pragma unroll
                for (int k = 0; k < NVP; ++k) ycol[k] = (TOPO::is_static ? k < TOPO::nv : k < nv) ? S.qfrc_smooth[k] : 0.0;
            }
        }
        const double raref = rtype >= 0 ? -rB * jvel - rK * rimp * (rpos - rmargin) : 0.0;

        /* ---- sensors, part 1 (sensors_before_solve; two-wave form: wave 1 runs it, in front of the barrier J or behind it -- env_step:
         *      sensors_behind_j) ---- */
        int aslot = -1;
        if constexpr (NW == 1) aslot = sensors_before_solve(io, S, m, env, issens, ls, sens_c, need_imu, lastsub);
        CK_STAMP(29);
        if (io.xpos_out && isbody && lastsub) {
            for (int i = 0; i < 3; ++i) io.xpos_out[((size_t)env * io.sb + b) * 3 + i] = S.x.s.xpos[b][i];
            if (io.xquat_out) for (int i = 0; i < 4; ++i) io.xquat_out[((size_t)env * io.sb + b) * 4 + i] = S.x.s.xquat[b][i];
        }
        if (readout_ext<FEAT>(io)) {
            cm_ext_t *ex = readout_ext<FEAT>(io) + env;
            if (isbody) for (int i = 0; i < 6; ++i) ex->cvel[b][i] = S.x.s.cvel[b][i];
            if (isbody) for (int i = 0; i < 3; ++i) { ex->subtree_com[b][i] = S.com[broot > 0 ? broot : 0][i]; ex->xipos[b][i] = S.x.s.xipos[b][i]; }
            if (lane < m->nsite) {
                const int sb = m->site_bodyid[lane];
                double sp[3] = {m->site_pos[lane][0], m->site_pos[lane][1], m->site_pos[lane][2]};
                double sq[4] = {m->site_quat[lane][0], m->site_quat[lane][1], m->site_quat[lane][2], m->site_quat[lane][3]};
                double t[3], q[4], mm[9];
                mulmatvec3(t, S.x.s.xmat[sb], sp);
                for (int i = 0; i < 3; ++i) ex->site_xpos[lane][i] = t[i] + S.x.s.xpos[sb][i];
                mulquat(q, S.x.s.xquat[sb], sq);
                quat2mat(mm, q);
                for (int i = 0; i < 9; ++i) ex->site_xmat[lane][i] = mm[i];
            }
            if (isdof) for (int i = 0; i < 6; ++i) { ex->cdof[k_][i] = S.cdof[k_][i]; ex->cdof_dot[k_][i] = S.x.s.cdof_dot[k_][i]; }
            if (!WIDE && rtype == CM_CNSTR_EQUALITY && r_ < CM_MAXEQROW) {
                ex->eq_pos[r_] = rpos; ex->eq_id[r_] = rid;
#pragma unroll
                for (int k = 0; k < NVP; ++k) if (k < nv) ex->eq_J[r_][k] = ycol[k];
            }
            if (lane == 0) { int ne = 0; for (int e = 0; e < m->neq; ++e) if (m->eq_active[e] && ne + 3 <= capr) ne += 3; ex->ne = ne; }
            if (lane < ncon) {
                ex->con_geom1[lane] = m->geom_fullid[S.c_g1[lane]]; ex->con_geom2[lane] = m->geom_fullid[S.c_g2[lane]];
                ex->con_body1[lane] = m->geom_bodyid[S.c_g1[lane]]; ex->con_body2[lane] = m->geom_bodyid[S.c_g2[lane]];
                ex->con_dim[lane] = S.c_dim[lane]; ex->con_dist[lane] = S.c_dist[lane];
                for (int i = 0; i < 3; ++i) ex->con_pos[lane][i] = S.c_pos[lane][i];
                for (int i = 0; i < 9; ++i) ex->con_frame[lane][i] = S.c_frame[lane][i];
            }
        }
        /* first constraint row of every contact (lane = contact), for the contact-force read-out */
        int caddr = -1;
        const bool want_cfrc = io.body_cfrc && (sub == nsub - 1 || !integrates<FEAT>(io)); /* read out by the last substep only */
        if (readout_ext<FEAT>(io) || want_cfrc || sums) { /* (the step sums take every substep's contact forces) */
            int acc = nefc_before_contacts;
            for (int c = 0; c < ncon; ++c) {
                const int dim = S.c_dim[c];
                if (dim != 1 && dim != 3) continue;
                const int nrow = dim == 1 ? 1 : 2 * (dim - 1);
                if (acc + nrow > capr) continue;
                if (c == lane) caddr = acc;
                acc += nrow;
            }
        }
        wv::sync(); /* every reader of the body-stage tiles ON THIS WAVE is done: region x becomes the Y staging tile (once wave 1's sensor
                     * stage, where it runs behind J, is done with them too: the wait for cmd[6] in front of the staging store) */
        CK_STAMP(8);

