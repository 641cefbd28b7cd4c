/* env_step, fragment: half solve, A = Y Y^T + R, warm start and PGS, the stages behind the solve (one-wave form) / the hand-over to wave 1 (two-wave form).
 * Included by physics_kernel.h INSIDE the body of ck::env_step (one function, so that the register allocator sees one region): not a header of its own. */
        if constexpr (WIDE) {
            /* the 127-row instantiation: half solve, A and the sweeps for this wave's rows 0 .. 63 (wide_solve; wave 1 is in the same
             * function for rows 64 .. 126 and the qfrc_smooth column), the row forces of both waves through LDS at the barrier P,
             * the read-outs from there */
            int iters = 0, nguarded = 0;
            const double f = wide_solve<NVP, TOPO>(S, m, P, 0, nefc, sub, iters, nguarded);
            CK_STAMP(11);

            /* (the step sums' actuator terms: ahead of the barrier P, behind which wave 1's Euler step changes qvel) */
            if constexpr (feat_sums(FEAT)) { if (sums && lane < nu) step_sums_add_actuator(sums, S, m, lane); }
            static_assert(sizeof(S.c_solimp) >= (2 * NROW + 4) * sizeof(double), "the row forces are handed over through the contacts' solimp slots");
            double *const fbuf = &S.c_solimp[0][0];
            fbuf[lane] = f;
            if (lane == 0) { fbuf[2 * NROW] = (double)ncon; fbuf[2 * NROW + 1] = (double)nefc; fbuf[2 * NROW + 2] = (double)iters; fbuf[2 * NROW + 3] = (double)nguarded; }
            wv::block_barrier(); /* P */
#ifdef CK_WIDE_PROFILE
            if constexpr (feat_prof(FEAT)) if (io.prof && lane < 12) io.prof[(size_t)env * NSTAMP + (lane < 6 ? 16 + lane : 22 + lane)] = (long long)S.x.stepv[lane / 6][lane % 6];   /* slots 16..21: wave 0, 28..33: wave 1 */
#endif
            if (readout_ext<FEAT>(io) || want_cfrc || sums) {
                /* decode the pyramid: normal = sum of the edge forces, tangents = mu (f+ - f-); the rows' forces from LDS */
                const int a0 = caddr >= 0 ? caddr : 0;
                double fn = 0, ft1 = 0, ft2 = 0;
                if (lane < ncon && caddr >= 0) {
                    const double f0 = fbuf[a0];
                    if (S.c_dim[lane] == 1) fn = f0;
                    else { const double f1 = fbuf[a0 + 1], f2 = fbuf[a0 + 2], f3 = fbuf[a0 + 3], mu = S.c_fri[lane][0]; fn = f0 + f1 + f2 + f3; ft1 = mu * (f0 - f1); ft2 = mu * (f2 - f3); }
                }
                if (readout_ext<FEAT>(io)) {
                    cm_ext_t *ex = readout_ext<FEAT>(io) + env;
                    if (lane < ncon) { ex->con_force[lane][0] = fn; ex->con_force[lane][1] = ft1; ex->con_force[lane][2] = ft2; }
                    if (lane == 0) { ex->ncon = ncon; ex->nefc = nefc; ex->solver_iter = iters; }
                }
                if (want_cfrc || sums) {
                    if (lane < ncon) {
                        const double *fr = S.c_frame[lane];
                        double fw[3];
                        for (int j = 0; j < 3; ++j) fw[j] = fr[j] * fn + fr[3 + j] * ft1 + fr[6 + j] * ft2;
                        for (int j = 0; j < 3; ++j) S.c_pos[lane][j] = fw[j];
                    }
                    wv::sync();
                    if (isbody) {
                        double acc[3] = {0, 0, 0};
                        bool touched = false;
                        for (int c = 0; c < ncon; ++c) {
                            const int b1 = m->geom_bodyid[S.c_g1[c]], b2 = m->geom_bodyid[S.c_g2[c]];
                            const double sg = (b2 == b ? 1.0 : 0.0) - (b1 == b ? 1.0 : 0.0);
                            if constexpr (feat_sums(FEAT)) touched |= b1 == b || b2 == b;
                            for (int j = 0; j < 3; ++j) acc[j] += sg * S.c_pos[c][j];
                        }
                        if (want_cfrc) for (int j = 0; j < 3; ++j) io.body_cfrc[((size_t)env * io.sb + b) * 3 + j] = acc[j];
                        if constexpr (feat_sums(FEAT)) { if (sums) step_sums_add_body(sums, b, acc, touched); }
                    }
                    wv::sync();
                }
            }
            wv::block_barrier(); /* E */
            CK_STAMP(37);
            if (wv::opaque(S.cmd[0])) { warn |= WARN_DIVERGED; break; }
            if (!integrates<FEAT>(io)) break;
            time += h;
            continue;
        }
        /* ================= half solve in registers: Y = D^-1/2 L^-T [J^T | qfrc_smooth], lane = column ================= */
        if constexpr (TOPO::is_static) {
            /* The multipliers do not depend on the solve, so dof k - 1's row of L is fetched (LDS broadcast reads) while
             * dof k's updates run; the fences keep the scheduler from re-pairing every read with its own wait. */
            double ta[NVP], tb[NVP], ra = 0, rb = 0;
            auto fetch = [&](int k, double (&t)[NVP], double &rs) {
#pragma unroll
                for (int i = k - 1; i >= 0; --i) if ((TOPO::table[k] >> i) & 1ull) t[i] = S.Lp[LPack<TOPO, NVP>::idx(k, i)];
                rs = S.rsd[k];
            };
            fetch(TOPO::nv - 1, ((TOPO::nv - 1) & 1) ? ta : tb, ((TOPO::nv - 1) & 1) ? ra : rb);
#pragma unroll
            for (int k = NVP - 1; k >= 0; --k) {
                if (k >= TOPO::nv) continue;
                if (k > 0) fetch(k - 1, ((k - 1) & 1) ? ta : tb, ((k - 1) & 1) ? ra : rb);
                wv::sched_fence();
                const double (&t)[NVP] = (k & 1) ? ta : tb;
                const double xk = ycol[k];
#pragma unroll
                for (int i = k - 1; i >= 0; --i) if ((TOPO::table[k] >> i) & 1ull) ycol[i] -= t[i] * xk;
                ycol[k] = xk * ((k & 1) ? ra : rb);
                wv::sched_fence();
            }
        } else {
#pragma unroll
            for (int k = NVP - 1; k >= 0; --k) {
                if (k >= nv) continue;
                const unsigned long long anc = m->dof_ancmask[k];
                const double xk = ycol[k];
#pragma unroll
                for (int i = k - 1; i >= 0; --i) {
                    if (!((anc >> i) & 1ull)) continue;
                    ycol[i] -= S.Lp[CK_TRI(k, i)] * xk;
                }
                ycol[k] = xk * S.rsd[k];
            }
        }
        long long t_wait = 0;
        if constexpr (sensors_behind_j) {
            /* this wave's first store into the body tiles' region since J (the matrix-core forms' Gram matrix overlays the same region,
             * behind this store): wave 1's sensor stage, which ran beside the half solve above, is done reading the tiles.  (The
             * profiled forms record how long the wait took, in clocks: the lower half of slot 15, stored behind the staging store -- a branch here
             * costs the stage its register allocation, see wave.h) */
            if constexpr (feat_prof(FEAT)) t_wait = wv::clock();
            wv::wait_for_straight(&S.cmd[6], sub + 1); /* (no loop the compiler sees: wave.h) */
            if constexpr (feat_prof(FEAT)) t_wait = wv::clock() - t_wait;
        }
        if (r_ < MAXR || lastcol) { /* (lanes MAXR .. 62 of a row-capped instantiation hold no row) */
            const int yrow = lastcol ? MAXR : r_;
#pragma unroll
            for (int k = 0; k < NVP; ++k) S.x.Yr[yrow][k] = ycol[k];
        }
        wv::sync();
        if constexpr (NW == 2) wv::publish(&S.cmd[2], sub + 1); /* wave 1 stages its column of Y for the qacc stage while this wave solves */
        CK_STAMP(9);
        if constexpr (sensors_behind_j && feat_prof(FEAT)) { if (io.prof && lane == 0) ((int *)&io.prof[(size_t)env * NSTAMP + 15])[0] = (int)t_wait; }

        /* ================= P9: this lane's row of A = Y^T Y + diag(R), b = Y^T y63 - aref ================= */
        double arow[MAXR];
        double diag_yy = 0; /* this lane's row of Y with itself */
        double rb = 0;
        /* Every product of two staged rows is ONE fused multiply-add chain over the dofs in index order, started from zero --
         * in both instantiations, so that their results agree bit for bit:
         *   - the row-capped instantiation (at most 31 rows + the qfrc_smooth row = a 32 x 32 Gram matrix of the staged tile)
         *     forms it on the matrix core: v_mfma_f64_16x16x4_f64 is exactly that chain per element (wave.h),
         *     three 16 x 16 tiles (the matrix is symmetric) x NVP / 4 blocks of dofs, operands straight from the staged
         *     tile, 64 clocks each with nothing else on the wave's critical path; the tiles go through LDS (the part of the
         *     body-stage region behind the staged tile) so that every lane ends up with its own row in registers;
         *   - the full instantiation forms the same chains on the vector unit, two rows at a time. */
        constexpr bool gram_on_matrix_core = MAXR == 31 && NVP % 4 == 0;
        constexpr bool gram_in_place = MAXR == 47 && NVP == 40; /* (the same on the matrix core, through the staged tile's own LDS: see there) */
        if constexpr (gram_on_matrix_core) {
            constexpr int YP = EnvShared<NVP, LPack<TOPO, NVP>::count, MAXR>::YP;
            static_assert(2 * (MAXR + 1) * YP * sizeof(double) <= sizeof(S.x), "the Gram matrix is parked behind the staged tile");
            double (*Am)[YP] = (double (*)[YP])(&S.x.Yr[0][0] + (MAXR + 1) * YP);
            const int mi = lane & 15, mk = lane >> 4;
            double y0[NVP / 4], y1[NVP / 4];
#pragma unroll
            for (int kb = 0; kb < NVP / 4; ++kb) { y0[kb] = S.x.Yr[mi][4 * kb + mk]; y1[kb] = S.x.Yr[16 + mi][4 * kb + mk]; }
            wv::mfma_acc t00 = {{0, 0, 0, 0}}, t01 = {{0, 0, 0, 0}}, t11 = {{0, 0, 0, 0}};
#pragma unroll
            for (int kb = 0; kb < NVP / 4; ++kb) wv::mfma_f64_16x16x4_x3(y0[kb], y0[kb], t00, y0[kb], y1[kb], t01, y1[kb], y1[kb], t11);
            wv::mfma_f64_drain(t00, t01, t11);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = mk + 4 * v;
                Am[row][mi] = t00.c[v];
                Am[row][16 + mi] = t01.c[v];
                Am[16 + mi][row] = t01.c[v];
                Am[16 + row][16 + mi] = t11.c[v];
            }
            wv::sync();
            const int myrow = lane & 31; /* (lanes 32 .. 63 hold no row: they read a row's values and never use them) */
#pragma unroll
            for (int t = 0; t < MAXR; ++t) arow[t] = Am[myrow][t];
            rb = Am[myrow][MAXR] - raref;
            /* (the register allocator's plan for the whole kernel depends on this lane's column of Y staying in registers up to
             * here -- it did when the vector unit formed the products; released at the staging store, 600 values go to
             * scratch all over the kernel.  No instruction is emitted.) */
#pragma unroll
            for (int k = 0; k < NVP; ++k) wv::touch(ycol[k]);
            diag_yy = Am[myrow][myrow];
        } else if constexpr (gram_in_place) {
            /* The 40-dof model's row-capped instantiation, one wave per env (512 registers): the 48 x 48 Gram matrix of the staged
             * tile (47 rows + the qfrc_smooth row) on the matrix core -- six 16 x 16 tiles x NVP / 4 blocks of dofs, the three
             * tiles of rows 32 .. 47 only when the substep has that many rows.  There is no LDS behind the staged tile to turn the
             * tiles into one row per lane, so it happens IN the region of the staged tile: every staged value is an operand of the
             * products and sits in a register by then (row 16 I + (lane & 15), dofs 4 kb + (lane >> 4)), the tiles overwrite the
             * staged tile, every lane takes its row of A, and the lanes store their rows of the tile once more (they still
             * hold them). */
            constexpr int AP = 49, AR = MAXR + 1; /* A at a leading dimension that keeps rows and columns off each other's banks */
            static_assert(AR == 48, "three blocks of sixteen staged rows");
            static_assert(AR * AP * sizeof(double) <= sizeof(S.x), "the matrix fits the region of the staged tile");
            double (*Am)[AP] = (double (*)[AP])&S.x.Yr[0][0];
            const int mi = lane & 15, mk = lane >> 4;
            double y0[NVP / 4], y1[NVP / 4], y2[NVP / 4];
#pragma unroll
            for (int kb = 0; kb < NVP / 4; ++kb) { y0[kb] = S.x.Yr[mi][4 * kb + mk]; y1[kb] = S.x.Yr[16 + mi][4 * kb + mk]; y2[kb] = S.x.Yr[32 + mi][4 * kb + mk]; }
            wv::mfma_acc t00 = {{0, 0, 0, 0}}, t01 = {{0, 0, 0, 0}}, t11 = {{0, 0, 0, 0}}, t02 = {{0, 0, 0, 0}}, t12 = {{0, 0, 0, 0}}, t22 = {{0, 0, 0, 0}};
#pragma unroll
            for (int kb = 0; kb < NVP / 4; ++kb) wv::mfma_f64_16x16x4_x3(y0[kb], y2[kb], t02, y1[kb], y2[kb], t12, y2[kb], y2[kb], t22); /* (row 47: always) */
#pragma unroll
            for (int kb = 0; kb < NVP / 4; ++kb) wv::mfma_f64_16x16x4_x3(y0[kb], y0[kb], t00, y0[kb], y1[kb], t01, y1[kb], y1[kb], t11);
            wv::mfma_f64_drain(t00, t01, t11);
            wv::mfma_f64_drain(t02, t12, t22);
            wv::sync(); /* every operand is in registers: the tile's rows may go */
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = mk + 4 * v; /* (a lane's four values of a tile: rows mk + 4 v of column mi, as wave.h lays the result out) */
                Am[row][mi] = t00.c[v];
                Am[row][16 + mi] = t01.c[v]; Am[16 + mi][row] = t01.c[v];
                Am[16 + row][16 + mi] = t11.c[v];
                Am[row][32 + mi] = t02.c[v]; Am[32 + mi][row] = t02.c[v];
                Am[16 + row][32 + mi] = t12.c[v]; Am[32 + mi][16 + row] = t12.c[v];
                Am[32 + row][32 + mi] = t22.c[v];
            }
            wv::sync();
            const int myrow = lane < AR ? lane : AR - 1; /* (lanes past the staged rows hold no row: they take one and never use it) */
            rb = Am[myrow][MAXR] - raref;
            diag_yy = Am[myrow][myrow];
            /* every lane takes its row of A, and the lanes store their rows of the tile once more (they still hold them).  (Leaving A
             * in LDS through the sweeps instead -- one ds_read_b64 per row of the chain, requested eight rows ahead -- frees the 94
             * registers of the row, but the chain is slower by more than the spills cost: round 5, 15.8 against 17.8 M in the two-wave
             * form, 13.7 against 15.6 M with one wave.) */
#pragma unroll
            for (int t = 0; t < MAXR; ++t) arow[t] = Am[myrow][t];
            wv::sync();
            if (r_ < MAXR || lastcol) {
                const int yrow = lastcol ? MAXR : r_;
#pragma unroll
                for (int k = 0; k < NVP; ++k) S.x.Yr[yrow][k] = ycol[k];
            }
            wv::sync();
        }
        else if constexpr (NW == 2 && NVP > 32) {
            /* the 40-dof instantiation at the 256 registers of the two-wave form: one staged row at a time, half a row in flight
             * (the row-pair loop below keeps two staged rows beside this lane's column and its row of A: 330 registers); the same
             * chain per product */
#pragma unroll
            for (int r = 0; r < MAXR; ++r) {
                double acc = 0;
                if (r < nefc) {
#pragma unroll
                    for (int k0 = 0; k0 < NVP; k0 += NVP / 2) {
                        double ya[NVP / 2];
#pragma unroll
                        for (int k = 0; k < NVP / 2; ++k) ya[k] = S.x.Yr[r][k0 + k];
#pragma unroll
                        for (int k = 0; k < NVP / 2; ++k) acc = fma(ya[k], ycol[k0 + k], acc);
                    }
                }
                arow[r] = acc;
            }
            {
                double acc = 0;
#pragma unroll
                for (int k = 0; k < NVP; ++k) acc = fma(S.x.Yr[MAXR][k], ycol[k], acc);
                rb = acc - raref;
            }
        } else {
#pragma unroll
        for (int r = 0; r < MAXR; r += 2) {
            /* rows in pairs: both broadcast rows are requested before the first product, so the second row's LDS latency
             * hides behind the first row's FMAs (rows past the last constraint hold zeros and cost one wasted row at most) */
            double acc0 = 0, acc1 = 0;
            if (r < nefc) {
                /* the 40-dof instantiation requests only the first half of the second row up front (its registers are what
                 * the allocator otherwise spills in this stage) and the rest once the first row's products are under way */
                constexpr int YB1 = NVP > 32 ? NVP / 2 : NVP;
                double ya[NVP], yb[NVP];
#pragma unroll
                for (int k = 0; k < NVP; ++k) ya[k] = S.x.Yr[r][k];
#pragma unroll
                for (int k = 0; k < YB1; ++k) yb[k] = S.x.Yr[r + 1 < MAXR ? r + 1 : r][k];
                wv::sched_fence();
                if constexpr (NVP == 32) {
                    /* (the instantiation with a row-capped twin: the chain of the matrix core, see above) */
#pragma unroll
                    for (int k = 0; k < NVP; ++k) { acc0 = fma(ya[k], ycol[k], acc0); if (r + 1 < MAXR) acc1 = fma(yb[k], ycol[k], acc1); }
                } else if constexpr (NVP == 40) {
                    /* (likewise: its substeps of at most 47 rows go through the matrix core, the in-place form above; the second
                     * row's late half arrives while the chains run over the early halves) */
#pragma unroll
                    for (int k = 0; k < YB1; ++k) { acc0 = fma(ya[k], ycol[k], acc0); if (r + 1 < MAXR) acc1 = fma(yb[k], ycol[k], acc1); }
                    wv::sched_fence();
#pragma unroll
                    for (int k = YB1; k < NVP; ++k) yb[k] = S.x.Yr[r + 1 < MAXR ? r + 1 : r][k];
#pragma unroll
                    for (int k = YB1; k < NVP; ++k) { acc0 = fma(ya[k], ycol[k], acc0); if (r + 1 < MAXR) acc1 = fma(yb[k], ycol[k], acc1); }
                } else {
                double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
                for (int k = 0; k < NVP; k += 4) {
                    a0 += ya[k] * ycol[k]; a1 += ya[k + 1] * ycol[k + 1];
                    a2 += ya[k + 2] * ycol[k + 2]; a3 += ya[k + 3] * ycol[k + 3];
                }
                acc0 = (a0 + a1) + (a2 + a3);
                if constexpr (YB1 < NVP) {
                    wv::sched_fence();
#pragma unroll
                    for (int k = YB1; k < NVP; ++k) yb[k] = S.x.Yr[r + 1 < MAXR ? r + 1 : r][k];
                }
                if (r + 1 < MAXR) {
                    double b0 = 0, b1 = 0, b2 = 0, b3 = 0;
#pragma unroll
                    for (int k = 0; k < NVP; k += 4) {
                        b0 += yb[k] * ycol[k]; b1 += yb[k + 1] * ycol[k + 1];
                        b2 += yb[k + 2] * ycol[k + 2]; b3 += yb[k + 3] * ycol[k + 3];
                    }
                    acc1 = (b0 + b1) + (b2 + b3);
                }
                }
            }
            arow[r] = acc0;
            if (r + 1 < MAXR) arow[r + 1] = acc1;
        }
        {
            double acc = 0;
#pragma unroll
            for (int k = 0; k < NVP; ++k) acc = fma(S.x.Yr[MAXR][k], ycol[k], acc);
            rb = acc - raref;
        }
        }
        CK_STAMP(10);

        /* ================= P10: warm start + projected Gauss-Seidel, one row per lane ================= */
        const bool isrow = rtype >= 0;
        const bool clampf = isrow && rtype != CM_CNSTR_EQUALITY;
        /* The diagonal of A: the lane's own row of Y with itself, plus the regulariser.  arow holds Y Y^T only -- selecting
         * R into the one lane-dependent entry of every row would cost a compare and four selects per row; instead the
         * R part of a row's action on its own residual is applied once per sweep (cdiag below): a row's residual is not
         * read again between its own turn and the end of the sweep. */
        double Aii = 1.0;
        if constexpr (gram_on_matrix_core || gram_in_place) { if (isrow) Aii = diag_yy + rR; }
        else if (isrow) {
            if constexpr (NVP == 32 || NVP == 40) { /* (the instantiations with a matrix-core form: its chain) */
                double d = 0;
#pragma unroll
                for (int k = 0; k < NVP; ++k) d = fma(ycol[k], ycol[k], d);
                Aii = d + rR;
            } else {
                double d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
                for (int k = 0; k < NVP; k += 4) {
                    d0 += ycol[k] * ycol[k]; d1 += ycol[k + 1] * ycol[k + 1];
                    d2 += ycol[k + 2] * ycol[k + 2]; d3 += ycol[k + 3] * ycol[k + 3];
                }
                Aii = ((d0 + d1) + (d2 + d3)) + rR;
            }
        }
        const double invAii = 1.0 / Aii;
        double f = 0, res = isrow ? rb : 0.0;
        int iters = 0, nguarded = 0; /* sweeps taken, and how many of them through the guarded fallback */
        if (nefc > 0) {
            if (m->flags & CM_FLAG_WARMSTART) {
                if (isrow) {
                    f = -(jws - raref) / rR;
                    if (clampf && f < 0) f = 0;
                }
                /* A f, rows four to a wave-uniform branch and four partial sums (rows past the last one contribute
                 * nothing: their column of A is zero and f is zero in lanes that are not rows) */
                double af0 = 0, af1 = 0, af2 = 0, af3 = 0;
#pragma unroll
                for (int t = 0; t < MAXR; t += 4) {
                    if (t < nefc) {
                        af0 += arow[t] * wv::readlane(f, t);
                        if (t + 1 < MAXR) af1 += arow[t + 1] * wv::readlane(f, t + 1);
                        if (t + 2 < MAXR) af2 += arow[t + 2] * wv::readlane(f, t + 2);
                        if (t + 3 < MAXR) af3 += arow[t + 3] * wv::readlane(f, t + 3);
                    }
                }
                const double af = ((af0 + af1) + (af2 + af3)) + (isrow ? rR * f : 0.0); /* + the diagonal's R */
                double cost = wv::wave_sum(isrow ? f * (rb + 0.5 * af) : 0.0);
                if (cost > 0) f = 0;
                else if (isrow) res = rb + af;
            }
        CK_STAMP(30);
            const double scale = 1.0 / (P->meaninertia * (nv > 1 ? nv : 1));
            const double halfAii = 0.5 * Aii;
            const double flo = clampf ? 0.0 : -1e300; /* lower bound of this row's force */
            /* to the scaled domain (see pgs_rows): arow becomes B in place */
            const double ninvAii = -invAii;
            double sres = res * ninvAii;
#pragma unroll
            for (int t = 0; t < MAXR; ++t) arow[t] *= ninvAii;
            const double cdiag = isrow ? rR * ninvAii : 0.0; /* the R part of B_jj = -(Y Y^T + R)_jj / A_jj, see above */
            const int maxiter = m->iterations;
            const double tolerance = m->tolerance;
            /* (the one-row shortcut below rests on the other rows raising the cost sum by at most 1e-10 each: that must stay inside
             * the half tolerance between its 2.5 x threshold and the 2 x band -- true of any tolerance a model is likely to ask for,
             * checked because the tolerance is the model's to set) */
            const bool shortcut_ok = 0.5 * tolerance > (double)MAXR * 1e-10 * scale;
            if constexpr (NW == 2 && CK_PRIO_W0_PGS != CK_PRIO_W0) wv::set_priority<CK_PRIO_W0_PGS>();
            while (iters < maxiter) {
                const int nrows = wv::opaque(nefc); /* keeps the row-bound tests out of loop-invariant hoisting */
                bool converged;
                {
                    const double f0 = f, s0 = sres;
                    double mys = 0;
                    const double lo_f = flo - f;
                    pgs_rows_fast<0, MAXR>(arow, nrows, r_, lo_f, sres, mys);
                    const double mydelta = wv::max_raw(mys, lo_f); /* (the very instruction the row chain took its step with) */
                    const double change = (r_ < nrows) ? mydelta * (halfAii * mydelta - Aii * mys) : 0.0;
                    /* The guarded sweep adds the rows' cost changes in row order, and the sum only feeds the convergence test.
                     * A single-precision tree sum decides it
                     * unless it lands within a factor two of the tolerance -- far outside what precision or the order of
                     * summation can move -- and only then is the ordered double-precision sum formed. */
                    /* One row whose own cost decrease is past 2.5 x the tolerance settles "not converged" without the sum: the other
                     * rows' changes are decreases too (or at most +1e-10 each, else the guard fires), so the sum is past the 2 x band
                     * below whatever they are.  Most sweeps before the last two or three end here: a compare and a ballot instead
                     * of the six-step tree sum on the sweep's dependent chain. */
                    const float tol = (float)tolerance;
                    const bool one_row_decides = shortcut_ok && wv::ballot(-(float)change * (float)scale > 2.5f * tol) != 0ull;
                    const float est = one_row_decides ? 4.0f * tol : -wv::wave_sum_f32((float)change) * (float)scale;
                    if (wv::ballot(change > 1e-10) != 0ull || wv::debug_force_guarded()) { /* some row would have raised the cost: redo guarded */
                        double improvement = 0;
                        f = f0; sres = s0; ++nguarded;
                        pgs_rows<0, MAXR>(arow, nrows, r_, Aii, halfAii, flo, f, sres, improvement);
                        sres = fma(cdiag, f - f0, sres);
                        converged = improvement * scale < tolerance;
                    } else {
                        if (r_ < nrows) { f += mydelta; sres = fma(cdiag, mydelta, sres); }
                        if (est < 0.5f * tol) converged = true;
                        else if (est > 2.0f * tol) converged = false;
                        else {
                            /* inside the band a double-precision tree sum decides: the rows' changes are cost decreases (at
                             * most +1e-10 each, or the guard had fired), so it differs from the ordered sum by rounding only,
                             * and the ordered sum is formed just when the tree sum lands within 1e-9 of the tolerance */
                            const double tree = -wv::wave_sum(change) * scale, tolv = tolerance;
                            if (fabs(tree - tolv) > 1e-9 * tolv) converged = tree < tolv;
                            else
                            {
                                double improvement = 0;
                                for (int t = 0; t < nrows; ++t) improvement -= wv::readlane(change, t);
                                converged = improvement * scale < tolerance;
                            }
                        }
                    }
                }
                ++iters;
                if (converged) break;
            }
        }
        if constexpr (NW == 2 && CK_PRIO_W0_PGS != CK_PRIO_W0) wv::set_priority<CK_PRIO_W0>();
        CK_STAMP(11);
        if (readout_ext<FEAT>(io) || want_cfrc || sums) {
            /* decode the pyramid: normal = sum of the edge forces, tangents = mu (f+ - f-) */
            const int a0 = caddr >= 0 ? caddr : 0;
            const double f0 = wv::shfl(f, a0), f1 = wv::shfl(f, (a0 + 1) & 63), f2 = wv::shfl(f, (a0 + 2) & 63), f3 = wv::shfl(f, (a0 + 3) & 63);
            double fn = 0, ft1 = 0, ft2 = 0;
            if (lane < ncon && caddr >= 0) {
                if (S.c_dim[lane] == 1) fn = f0;
                else { const double mu = S.c_fri[lane][0]; fn = f0 + f1 + f2 + f3; ft1 = mu * (f0 - f1); ft2 = mu * (f2 - f3); }
            }
            if (readout_ext<FEAT>(io)) {
                cm_ext_t *ex = readout_ext<FEAT>(io) + env;
                if (lane < ncon) { ex->con_force[lane][0] = fn; ex->con_force[lane][1] = ft1; ex->con_force[lane][2] = ft2; }
                if (lane == 0) { ex->ncon = ncon; ex->nefc = nefc; ex->solver_iter = iters; }
            }
            if (want_cfrc || sums) {
                /* world-frame force of every contact parked over its (no longer needed) position, then lane = body adds
                 * up the contacts it takes part in: + on geom2's body, - on geom1's */
                if (lane < ncon) {
                    const double *fr = S.c_frame[lane];
                    double fw[3];
                    for (int j = 0; j < 3; ++j) fw[j] = fr[j] * fn + fr[3 + j] * ft1 + fr[6 + j] * ft2;
                    for (int j = 0; j < 3; ++j) S.c_pos[lane][j] = fw[j];
                }
                wv::sync();
                if (isbody) {
                    double acc[3] = {0, 0, 0};
                    bool touched = false;
                    for (int c = 0; c < ncon; ++c) {
                        const int b1 = m->geom_bodyid[S.c_g1[c]], b2 = m->geom_bodyid[S.c_g2[c]];
                        const double sg = (b2 == b ? 1.0 : 0.0) - (b1 == b ? 1.0 : 0.0);
                        if constexpr (feat_sums(FEAT)) touched |= b1 == b || b2 == b;
                        for (int j = 0; j < 3; ++j) acc[j] += sg * S.c_pos[c][j];
                    }
                    if (want_cfrc) for (int j = 0; j < 3; ++j) io.body_cfrc[((size_t)env * io.sb + b) * 3 + j] = acc[j];
                    if constexpr (feat_sums(FEAT)) { if (sums) step_sums_add_body(sums, b, acc, touched); }
                }
                wv::sync();
            }
        }
        /* (the step sums' actuator terms: qvel is still the state the substep started from -- the Euler step is below, or wave 1's behind P) */
        if constexpr (feat_sums(FEAT)) { if (sums && lane < nu) step_sums_add_actuator(sums, S, m, lane); }

        if constexpr (NW == 2) {
            /* Two-wave form: the stages behind the solve -- qacc, the accelerometers, the substep's outputs, the Euler step -- are
             * wave 1's, which has staged their operands (its row of L, its column of Y, its row and column of the factor of
             * M + hB) while this wave was in its PGS sweeps.  The row forces and the solver statistics go through LDS -- the contacts'
             * solimp slots, which nothing reads behind the rows' impedances -- at barrier P; barrier E ends the substep. */
            static_assert(sizeof(S.c_solimp) >= 68 * sizeof(double), "the row forces are handed over through the contacts' solimp slots");
            double *const fbuf = &S.c_solimp[0][0];
            fbuf[lane] = f;
            if (lane == 0) { fbuf[64] = (double)ncon; fbuf[65] = (double)nefc; fbuf[66] = (double)iters; fbuf[67] = (double)nguarded; }
            wv::block_barrier(); /* P */
            wv::block_barrier(); /* E */
            CK_STAMP(37);
            if (wv::opaque(S.cmd[0])) { warn |= WARN_DIVERGED; break; }
            if (!integrates<FEAT>(io)) break;
            time += h;
            continue;
        }
        /* ================= qacc = L^-1 D^-1/2 (y63 + Y f)  (lane = dof) ================= */
        /* (constants of the stages behind the solves, requested ahead of them: actuator velocities, the Euler step) */
        const int pf_u = lane < nu ? lane : 0, pf_ej = lane < njnt ? lane : 0;
        const double pf_agear = m->act_gear[pf_u], pf_kdamp = P->dof_damping[isdof ? k_ : 0];
        const int pf_adof = m->act_dofid[pf_u], pf_ejt = m->jnt_type[pf_ej], pf_eqa = m->jnt_qposadr[pf_ej], pf_eda = m->jnt_dofadr[pf_ej];
        double qacc;
        {
            double z = isdof ? S.x.Yr[MAXR][k_] : 0.0;
            {
                /* z += Y f : rows in groups of four so LDS reads and broadcasts overlap; rolled (row count is dynamic) */
                double z1 = 0, z2 = 0, z3 = 0;
                const int kk = isdof ? k_ : 0;
                int r = 0;
                for (; r + 4 <= nefc; r += 4) {
                    const double y0 = S.x.Yr[r][kk], y1 = S.x.Yr[r + 1][kk], y2 = S.x.Yr[r + 2][kk], y3 = S.x.Yr[r + 3][kk];
                    z += y0 * wv::readlane(f, r); z1 += y1 * wv::readlane(f, r + 1);
                    z2 += y2 * wv::readlane(f, r + 2); z3 += y3 * wv::readlane(f, r + 3);
                }
                for (; r < nefc; ++r) z += S.x.Yr[r][kk] * wv::readlane(f, r);
                z = (z + z1) + (z2 + z3);
                if (!isdof) z = 0.0;
            }
            if (isdof) z *= S.rsd[k_];
            /* forward substitution with this lane's row of L staged first (all LDS reads in flight together) */
            double lrow[NVP];
            stage_factor_row<NVP, TOPO>(S, k_, isdof, lrow);
            qacc = solve_forward<NVP, TOPO>(z, lrow, lane, nv);
        }
        {
            const bool badv = isdof && (!(qacc == qacc) || fabs(qacc) > 1e10);
            if (wv::ballot(badv) != 0ull) { warn |= WARN_DIVERGED; break; }
        }
        if (isdof) S.qacc[k_] = qacc;
        wv::sync();
        CK_STAMP(12);

        /* ---- sensors, part 2 (the accelerometer needs qacc), actuator velocities, the last substep's outputs ---- */
        outputs_after_qacc(io, S, m, env, lane, isdof, k_, nu, qacc, aslot, sb, need_imu, lastsub, pf_agear * S.qvel[pf_adof], ncon, nefc, iters, nguarded);
        if (!integrates<FEAT>(io)) break;
        CK_STAMP(13);

        /* ================= P12 semi-implicit Euler with implicit joint damping ================= */
        {
            double lcol[NVP], lrowh[NVP]; /* this lane's column and row of the factor of M + hB, staged before the chains */
            stage_factor_h<NVP, TOPO>(S, k_, isdof, nv, lcol, lrowh);
            const double dih = isdof ? S.dinvH[k_] : 0.0;
            euler_step<NVP, TOPO>(S, m, lane, isdof, k_, nv, njnt, h, qacc, lcol, lrowh, dih, pf_kdamp, pf_ejt, pf_eqa, pf_eda);
        }
        time += h;
        CK_STAMP(14);
    }

