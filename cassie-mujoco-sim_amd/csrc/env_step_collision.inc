/* env_step, fragment: P4 collision -- pair loop, height-field pre-pass / prism pass, whole-wave box pairs, joint limits, the hand-over verdict.
 * Included by physics_kernel.h INSIDE the body of ck::env_step (one function, so that the register allocator sees one region): not a header of its own. */
        /* ================= P4 collision ================= */
        /* Requested here, read behind the collision passes (joint limits; the dof-chain indices of the velocity stage): the
         * constants' trip through the memory system runs under the pair loop. */
        /* (unconditional reads at clamped indices; the lane predicates are applied where the values are used, behind
         * wv::keep -- a predicate folded into the read would make the compiler wait for the value on the spot) */
        /* rounds of radix-4 pointer jumping along the dof chains (velocity stage, cm_model_t::dof_anc4): after round r a dof
         * holds the sum over itself and its 4^(r+1) - 1 nearest ancestors; a compile-time topology knows how long its longest
         * chain is (Cassie: 14 dofs -> two rounds) */
        constexpr int chain_rounds = [] {
            if constexpr (TOPO::is_static) { int r = 0, n = 1; while (n < DofLevels<TOPO>::depth() + 1) { n *= 4; ++r; } return r < 3 ? r : 3; }
            else return 3;
        }();
        int pf_jlim, pf_jtype, pf_jqadr, danc[9], blast, kvin;
        double pf_jmargin, pf_jlo, pf_jhi;
        auto request_behind_collision = [&](int lane_now) {
            const int pf_lj = lane_now < njnt ? lane_now : 0, pf_kd = lane_now < nv ? lane_now : 0, pf_bb = lane_now < nbody ? lane_now : 0;
            pf_jlim = m->jnt_limited[pf_lj]; pf_jtype = m->jnt_type[pf_lj]; pf_jqadr = m->jnt_qposadr[pf_lj];
            pf_jmargin = m->jnt_margin[pf_lj]; pf_jlo = m->jnt_range[pf_lj][0]; pf_jhi = m->jnt_range[pf_lj][1];
#pragma unroll
            for (int r = 0; r < 3 * chain_rounds; ++r) danc[r] = m->dof_anc4[pf_kd][r];
            blast = m->body_lastdof[pf_bb]; kvin = m->dof_vinsrc[pf_kd];
        };
        /* (the instantiations with the height-field pre-pass have no registers to spare across it and the pair loop: they ask
         * behind the loop) */
        constexpr bool request_early = (FEAT & FEAT_HFIELD) == 0;
        if constexpr (request_early) request_behind_collision(lane);
        /* A pair's constants (one level of lane-coalesced reads of the denormalised pair_* arrays) are requested ahead of
         * their pass: the first 64 pairs' here, the next 64 pairs' between a pass's narrow phase and its contact compaction
         * (into the same registers, which the narrow phase has finished with), so that their trip through the memory system
         * runs under the compaction. */
        const int pair_bound = m->npair_simple;
        struct PairConst { int g1, g2, tt; double margin, rb1, rb2, s10, s11, s20, s21, s22; };
        auto request_pair = [&](int pp, PairConst &c) {
            const int ps = pp < pair_bound ? pp : 0;
            c.g1 = m->pair_geom1[ps]; c.g2 = m->pair_geom2[ps]; c.tt = m->pair_type[ps];
            c.margin = m->pair_margin[ps]; c.rb1 = m->pair_rbound[ps][0]; c.rb2 = m->pair_rbound[ps][1];
            c.s10 = m->pair_size[ps][0]; c.s11 = m->pair_size[ps][1];
            c.s20 = m->pair_size[ps][3]; c.s21 = m->pair_size[ps][4]; c.s22 = m->pair_size[ps][5];
        };
        PairConst pc;
        if constexpr (request_early) request_pair(lane, pc);
        /* pass 1, lane = candidate pair (pair types that give at most two contacts) */
        int ncon = 0;
        /* (env_hfield, the env's grid: shared, its own, or the bank's terrain the env's index names -- resolved once per call ahead of the
         * substep loop, physics_kernel.h) */
        /* block cull: pairs against static non-plane geoms (stairs ...) are visited only if one of those geoms is
         * within reach of a kinematic tree (lane = collision geom) */
        int npass = m->npair_always;
        if (m->npair_simple > m->npair_always) {
            bool nearby = false;
            if (lane < m->ngeom && m->geom_farstatic[lane]) {
                const double rb = m->geom_rbound[lane] + m->geom_margin[lane];
                for (int ri = 0; ri < m->nroot; ++ri) {
                    const int r = m->root_body[ri];
                    double dv[3] = {S.x.s.geom_xpos[lane][0] - S.x.s.xpos[r][0], S.x.s.geom_xpos[lane][1] - S.x.s.xpos[r][1],
                                    S.x.s.geom_xpos[lane][2] - S.x.s.xpos[r][2]};
                    const double bound = PG->body_reach[r] + rb + 0.01;
                    if (dot3(dv, dv) < bound * bound) nearby = true;
                }
            }
            if (wv::ballot(nearby) != 0ull) npass = m->npair_simple;
        }
        CK_STAMP(21);
        /* Height-field pairs ahead of the pair loop: their sample spheres -- the sphere itself, or a capsule's two ends and
         * up to four interior samples -- go one to a lane (CM_HF_SLOTS lanes per pair, CM_HF_PASS pairs per pass), so the
         * walks over the grid cells under the samples run side by side instead of one after the other in the pair's lane;
         * the lanes of a pair then apply the capsule rule (oracle hfield_capsule) to the samples' results and the pair's
         * first lane parks the outcome -- contact count and up to two contacts -- in an LDS table laid over the velocity
         * tiles (unused until the velocity stage), where the pair loop below picks it up.  (Round 2 carried the outcome in
         * registers and fetched it with 40 cross-lane moves per pair-loop pass, and kept a second copy of the terrain walk
         * inside the pair loop for models with more pairs than one pass holds: both were what this instantiation spilled.) */
        constexpr int HF_REC = 1 + 10 * CM_HF_MAXC; /* doubles per pair: count, then up to CM_HF_MAXC x (dist, pos[3], normal[3], tangent[3]) */
        static_assert(CM_MAXHFPAIR * HF_REC <= NB * 12 + NVP * 12, "the height-field result table must fit the cvel + cfrc + cdof_dot + buf tiles");
        static_assert(offsetof(decltype(S.x.s), buf) - offsetof(decltype(S.x.s), cvel) == sizeof(double) * (NB * 12 + NVP * 6), "those four tiles are contiguous");
        static_assert(CM_HF_PASS * CM_HF_SLOTS <= WV_WAVE && CM_HF_SLOTS_DENSE <= WV_WAVE, "a pass of the height-field pre-pass is one wave");
        double *const hfres = &S.x.s.cvel[0][0];
        const bool hf_on = (FEAT & FEAT_HFIELD) != 0 && env_hfield != nullptr && m->nhfpair > 0;
        const bool hf_prism = (FEAT & FEAT_HFIELD) != 0 && hf_on && (m->flags & CM_FLAG_HFPRISM) != 0;
        int ncon_prism = 0;
        if constexpr ((FEAT & FEAT_HFIELD) != 0) if (hf_prism) {
            /* CM_FLAG_HFPRISM: one contact per penetrated grid triangle, straight into the contact list ahead of the other pairs' */
            static_assert(CM_MAXHFPAIR * HP_REC + 64 * 2 * CM_HP_MAXS / 8 <= NB * 12 + NVP * 12, "the per-pair records of the prism pass and its task table (a byte per task) fit the idle velocity tiles");
            CK_STAMP(44);
            ncon_prism = hfield_prism_wave(S, m, env_hfield, lane, hfres, MAXC);
            CK_STAMP(46);
        }
        if constexpr ((FEAT & FEAT_HFIELD) != 0) if (hf_on && !hf_prism) {
            /* CM_FLAG_HFDENSE: ten sample slots per pair (six pairs per pass) instead of six (ten pairs per pass) */
            const bool dense = (m->flags & CM_FLAG_HFDENSE) != 0;
            const int slots = dense ? CM_HF_SLOTS_DENSE : CM_HF_SLOTS, per_pass = dense ? WV_WAVE / CM_HF_SLOTS_DENSE : CM_HF_PASS;
            for (int h0 = 0; h0 < m->nhfpair; h0 += per_pass) {
                const int hl = dense ? lane / CM_HF_SLOTS_DENSE : lane / CM_HF_SLOTS;
                const int h = h0 + hl, k = lane - hl * slots;
                const bool act = hl < per_pass && h < m->nhfpair;
                const int p = m->hfpair[act ? h : 0];
                const int g1 = m->pair_geom1[p], g2 = m->pair_geom2[p], t2 = m->pair_type[p] >> 8;
                const double margin = m->pair_margin[p], s20 = m->pair_size[p][3], s21 = m->pair_size[p][4];
                const double *p1 = S.x.s.geom_xpos[g1], *m1 = S.x.s.geom_xmat[g1], *p2 = S.x.s.geom_xpos[g2], *m2 = S.x.s.geom_xmat[g2];
                const double axis[3] = {m2[2], m2[5], m2[8]};
                const double cell = 2 * m->hfield_size[0] / (m->hfield_ncol > 1 ? m->hfield_ncol - 1 : 1);
                int ni = 0;
                bool mine = act && k == 0;
                double t = 0;
                if (t2 == CM_GEOM_CAPSULE) {
                    ni = (int)ceil(2 * s21 / cell) - 1;
                    if (ni < 0) ni = 0;
                    if (ni > slots - 2) ni = slots - 2;
                    mine = act && k < 2 + ni;
                    t = k == 0 ? s21 : (k == 1 ? -s21 : s21 * (1.0 - 2.0 * (k - 1) / (ni + 1)));
                }
                RawContact rcs;
                rcs.dist = 1e300;
                bool has = false;
                {
                    /* (all lanes: the wave shares the cells under the pass's samples; the contact tables are scratch until the
                     * pair loop below fills them) */
                    double e[3] = {p2[0] + t * axis[0], p2[1] + t * axis[1], p2[2] + t * axis[2]};
                    static_assert(offsetof(SH_T, c_tran) + sizeof(S.c_tran) - offsetof(SH_T, c_dist) >= (size_t)HF_WORK_BYTES,
                                  "the contact tables hold the work area of hfield_spheres_wave");
                    CK_STAMP(44);
                    has = hfield_spheres_wave(rcs, m, env_hfield, p1, m1, mine, e, s20, margin, lane, &S.c_dist[0]) != 0;
                    CK_STAMP(45);
                }
                /* the samples of this lane's pair: distances (1e300 = no contact) */
                const int lead = lane - k;
                double dk[CM_HF_SLOTS_DENSE];
                const double mydist = has ? rcs.dist : 1e300;
#pragma unroll
                for (int q = 0; q < CM_HF_SLOTS_DENSE; ++q) {
                    if (q >= CM_HF_SLOTS && !dense) { dk[q] = 1e300; continue; } /* (wave-uniform) */
                    const double v = wv::shfl(mydist, (lead + q) & 63);
                    dk[q] = q < slots ? v : 1e300;
                }
                int src0 = 0, src1 = 1;
                bool have0 = dk[0] < 1e299, have1 = dk[1] < 1e299;
                if (t2 == CM_GEOM_CAPSULE) {
                    int kmid = -1;
                    double dmid = 1e300;
#pragma unroll
                    for (int q = 2; q < CM_HF_SLOTS_DENSE; ++q) if (dk[q] < 1e299 && (kmid < 0 || dk[q] < dmid)) { kmid = q; dmid = dk[q]; }
                    if (kmid >= 0 && (!have0 || dmid < dk[0]) && (!have1 || dmid < dk[1])) {
                        const bool drop1 = !have0 ? false : (!have1 ? true : dk[0] <= dk[1]);
                        if (drop1) { src1 = kmid; have1 = true; } else { src0 = kmid; have0 = true; }
                    }
                } else {
                    have1 = false;
                }
                /* the lanes holding the chosen samples write them: first kept contact to record slot 0, second to slot 1 */
                int nkeep = (have0 ? 1 : 0) + (have1 ? 1 : 0);
                double *rec = hfres + (size_t)(act ? h : 0) * HF_REC;
                int slot_of_me = (have0 && k == src0) ? 0 : ((have1 && k == src1) ? (have0 ? 1 : 0) : -1);
                if ((m->flags & CM_FLAG_HFMULTI) && t2 == CM_GEOM_CAPSULE) {
                    /* CM_FLAG_HFMULTI: up to CM_HF_MAXC contacts, the deepest samples first (ties: lower sample index): a
                     * sample's record slot is its rank among the pair's samples */
                    int rank = 0, cnt = 0;
#pragma unroll
                    for (int q = 0; q < CM_HF_SLOTS_DENSE; ++q) {
                        const bool valid = dk[q] < 1e299;
                        cnt += valid ? 1 : 0;
                        rank += (valid && (dk[q] < mydist || (dk[q] == mydist && q < k))) ? 1 : 0;
                    }
                    nkeep = cnt < CM_HF_MAXC ? cnt : CM_HF_MAXC;
                    slot_of_me = (has && rank < CM_HF_MAXC) ? rank : -1;
                }
                if (act && k == 0) rec[0] = (double)nkeep;
                if (act && slot_of_me >= 0) {
                    double *c = rec + 1 + 10 * slot_of_me;
                    c[0] = rcs.dist;
                    for (int i = 0; i < 3; ++i) { c[1 + i] = rcs.pos[i]; c[4 + i] = rcs.normal[i]; c[7 + i] = t2 == CM_GEOM_CAPSULE ? axis[i] : 0.0; }
                }
            }
            wv::sync();
            CK_STAMP(46);
        }
        if constexpr (!request_early) request_pair(lane, pc);
        if constexpr ((FEAT & FEAT_HFIELD) != 0) ncon = ncon_prism; /* (the prism pass's contacts come first) */
        for (int p0 = 0; p0 < npass; p0 += WV_WAVE) {
            const int p = p0 + lane;
            int n = 0;
            RawContact rc0, rc1;
            bool from_spread = false;
            int hfs = -1;
            if constexpr ((FEAT & FEAT_HFIELD) != 0) {
                /* height-field pairs take their result from the table the pre-pass filled (no terrain bound: no contact) */
                const int slot = p < npass ? m->pair_hfslot[p] : -1;
                if (slot >= 0) {
                    from_spread = true;
                    if (hf_on && !hf_prism) {
                        const double *rec = hfres + (size_t)slot * HF_REC;
                        n = (int)rec[0];
                        hfs = slot;     /* (contacts 3 and 4 of a CM_FLAG_HFMULTI pair go from the table straight to the contact list) */
                        rc0.dist = rec[1]; rc1.dist = rec[11];
                        for (int i = 0; i < 3; ++i) {
                            rc0.pos[i] = rec[2 + i]; rc0.normal[i] = rec[5 + i]; rc0.tangent[i] = rec[8 + i];
                            rc1.pos[i] = rec[12 + i]; rc1.normal[i] = rec[15 + i]; rc1.tangent[i] = rec[18 + i];
                        }
                    }
                }
            }
            if (p < npass && !from_spread) {
                const int g1 = pc.g1, g2 = pc.g2, tt = pc.tt;
                const int t1 = tt & 255, t2 = tt >> 8;
                const double margin = pc.margin;
                const double *p1 = S.x.s.geom_xpos[g1], *p2 = S.x.s.geom_xpos[g2];
                const double *m1 = S.x.s.geom_xmat[g1], *m2 = S.x.s.geom_xmat[g2];
                const double rb1 = pc.rb1, rb2 = pc.rb2;
                /* (the sizes come with the pair's other constants, not behind the cull: a second trip to memory for the pairs
                 * that survive it costs the whole wave more than five reads that most lanes do not use) */
                const double s10 = pc.s10, s11 = pc.s11, s20 = pc.s20, s21 = pc.s21, s22 = pc.s22;
                double dif[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
                CK_STAMP(31);
                bool cull = false;
                if (rb1 > 0 && rb2 > 0) {
                    double bound = rb1 + rb2 + margin;
                    cull = dot3(dif, dif) > bound * bound;
                } else if (t1 == CM_GEOM_PLANE && rb2 > 0) {
                    double nn[3] = {m1[2], m1[5], m1[8]};
                    cull = dot3(dif, nn) > margin + rb2;
                }
                if (!cull) {
                    if (t1 == CM_GEOM_PLANE && t2 == CM_GEOM_SPHERE) {
                        n = plane_sphere(rc0, p1, m1, p2, s20, margin);
                    } else if (t1 == CM_GEOM_PLANE && t2 == CM_GEOM_CAPSULE) {
                        double axis[3] = {m2[2], m2[5], m2[8]};
                        RawContact tmp;
                        double e0[3] = {p2[0] + s21 * axis[0], p2[1] + s21 * axis[1], p2[2] + s21 * axis[2]};
                        if (plane_sphere(tmp, p1, m1, e0, s20, margin)) { rc0 = tmp; n = 1; }
                        double e1[3] = {p2[0] - s21 * axis[0], p2[1] - s21 * axis[1], p2[2] - s21 * axis[2]};
                        if (plane_sphere(tmp, p1, m1, e1, s20, margin)) { if (n == 0) rc0 = tmp; else rc1 = tmp; ++n; }
                        for (int i = 0; i < 3; ++i) { rc0.tangent[i] = axis[i]; rc1.tangent[i] = axis[i]; }
                    } else if (t1 == CM_GEOM_SPHERE && t2 == CM_GEOM_SPHERE) {
                        n = sphere_sphere(rc0, p1, s10, p2, s20, margin);
                    } else if (t1 == CM_GEOM_SPHERE && t2 == CM_GEOM_CAPSULE) {
                        double a2[3] = {m2[2], m2[5], m2[8]};
                        double d12[3] = {-dif[0], -dif[1], -dif[2]};
                        double x = clampd(dot3(a2, d12), -s21, s21);
                        double q2[3] = {p2[0] + a2[0] * x, p2[1] + a2[1] * x, p2[2] + a2[2] * x};
                        n = sphere_sphere(rc0, p1, s10, q2, s20, margin);
                    } else if (t1 == CM_GEOM_CAPSULE && t2 == CM_GEOM_CAPSULE) {
                        double a1[3] = {m1[2], m1[5], m1[8]}, a2[3] = {m2[2], m2[5], m2[8]};
                        double x1, x2;
                        segment_closest(p1, a1, s11, p2, a2, s21, x1, x2);
                        double q1[3] = {p1[0] + a1[0] * x1, p1[1] + a1[1] * x1, p1[2] + a1[2] * x1};
                        double q2[3] = {p2[0] + a2[0] * x2, p2[1] + a2[1] * x2, p2[2] + a2[2] * x2};
                        n = sphere_sphere(rc0, q1, s10, q2, s20, margin);
                    } else if (t1 == CM_GEOM_SPHERE && t2 == CM_GEOM_BOX) {
                        double sb[3] = {s20, s21, s22};
                        n = sphere_box(rc0, p1, s10, p2, m2, sb, margin);
                    } else if (t1 == CM_GEOM_CAPSULE && t2 == CM_GEOM_BOX) {
                        double sb[3] = {s20, s21, s22};
                        n = capsule_box(rc0, rc1, p1, m1, s10, s11, p2, m2, sb, margin);
                    } else {
                        warn |= WARN_UNSUPPORTED_PAIR;
                    }
                }
            }
            CK_STAMP(32);
            if (p0 + WV_WAVE < npass) request_pair(p + WV_WAVE, pc);
            /* ballot-compact in pair order */
            const unsigned long long m1b = wv::ballot(n >= 1), m2b = wv::ballot(n >= 2);
            const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
            int slot = ncon + wv::popc64(m1b & below) + wv::popc64(m2b & below);
            int more = 0;
            if constexpr ((FEAT & FEAT_HFIELD) != 0) {
                /* height-field pairs with CM_FLAG_HFMULTI can hold a third and a fourth contact */
                const unsigned long long m3b = wv::ballot(n >= 3), m4b = wv::ballot(n >= 4);
                slot += wv::popc64(m3b & below) + wv::popc64(m4b & below);
                more = wv::popc64(m3b) + wv::popc64(m4b);
                for (int extra = 2; extra < CM_HF_MAXC; ++extra)
                    if (n > extra && slot + extra < MAXC) {
                        const double *c = hfres + (size_t)hfs * HF_REC + 1 + 10 * extra;
                        RawContact rx;
                        rx.dist = c[0];
                        for (int i = 0; i < 3; ++i) { rx.pos[i] = c[1 + i]; rx.normal[i] = c[4 + i]; rx.tangent[i] = c[7 + i]; }
                        write_raw_contact(S, slot + extra, p, rx);
                    }
            }
            if (n >= 1 && slot < MAXC) write_raw_contact(S, slot, p, rc0);
            if (n >= 2 && slot + 1 < MAXC) write_raw_contact(S, slot + 1, p, rc1);
            ncon += wv::popc64(m1b) + wv::popc64(m2b) + more;
        }
        CK_STAMP(22);
        if constexpr (!request_early) request_behind_collision(lane);
        /* pass 2, one pair at a time with the whole wave: lane = feature (box corner / vertex), first four hits kept */
        if constexpr ((FEAT & FEAT_WAVEPAIRS) != 0) for (int p = m->npair_simple; p < m->npair; ++p) {
            const int g1 = m->pair_geom1[p], g2 = m->pair_geom2[p], tt = m->pair_type[p];
            const int t1 = tt & 255, t2 = tt >> 8;
            const double margin = m->pair_margin[p];
            const double *p1 = S.x.s.geom_xpos[g1], *p2 = S.x.s.geom_xpos[g2];
            const double *m1 = S.x.s.geom_xmat[g1], *m2 = S.x.s.geom_xmat[g2];
            const double rb1 = m->pair_rbound[p][0], rb2 = m->pair_rbound[p][1];
            {
                double dif[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
                bool cull = false;
                if (rb1 > 0 && rb2 > 0) { const double bound = rb1 + rb2 + margin; cull = dot3(dif, dif) > bound * bound; }
                else if (t1 == CM_GEOM_PLANE && rb2 > 0) { double nn[3] = {m1[2], m1[5], m1[8]}; cull = dot3(dif, nn) > margin + rb2; }
                if (cull) continue; /* wave-uniform: poses come from LDS broadcasts */
            }
            bool hit = false;
            int pairmax = 4;                 /* contacts a whole-wave pair keeps */
            RawContact rc;
            if (t1 == CM_GEOM_PLANE && t2 == CM_GEOM_BOX) {
                if (lane < 8) {
                    const double sb0 = m->pair_size[p][3], sb1 = m->pair_size[p][4], sb2 = m->pair_size[p][5];
                    double nrm[3] = {m1[2], m1[5], m1[8]}, dif[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
                    const double dist = dot3(dif, nrm);
                    double v[3] = {(lane & 1) ? sb0 : -sb0, (lane & 2) ? sb1 : -sb1, (lane & 4) ? sb2 : -sb2}, corner[3];
                    mulmatvec3(corner, m2, v);
                    const double ld = dot3(nrm, corner);
                    if (!(dist + ld > margin || ld > 0)) {
                        hit = true;
                        rc.dist = dist + ld;
                        for (int k = 0; k < 3; ++k) { rc.normal[k] = nrm[k]; rc.tangent[k] = 0; rc.pos[k] = corner[k] + p2[k] - nrm[k] * 0.5 * rc.dist; }
                    }
                }
            } else if (t1 == CM_GEOM_BOX && t2 == CM_GEOM_BOX) {
                double s1[3] = {m->pair_size[p][0], m->pair_size[p][1], m->pair_size[p][2]};
                double s2[3] = {m->pair_size[p][3], m->pair_size[p][4], m->pair_size[p][5]};
                pairmax = (m->flags & CM_FLAG_BOX8) ? 8 : 4;
                hit = box_box_lane(rc, lane, p1, m1, s1, p2, m2, s2, margin, pairmax);
            } else {
                warn |= WARN_UNSUPPORTED_PAIR;
            }
            const unsigned long long hb = wv::ballot(hit);
            const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
            const int rank = wv::popc64(hb & below);
            if (hit && rank < pairmax && ncon + rank < MAXC) write_raw_contact(S, ncon + rank, p, rc);
            const int nh = wv::popc64(hb);
            ncon += nh < pairmax ? nh : pairmax;
        }
        const int ncon_found = ncon;
        if (ncon > capc) ncon = capc; /* (the warning bit: below, unless the substep is handed over) */
        wv::sync();
        finish_contacts(S, m, P, lane, ncon);
        /* joint limits: lane = joint evaluates its own violation (the ballots give the row slots in joint order below) */
        unsigned long long lob, hib;
        {
            bool lo = false, hi = false;
            wv::keep(pf_jlim); wv::keep(pf_jtype);
            if (lane < njnt && pf_jlim && (pf_jtype == CM_JNT_HINGE || pf_jtype == CM_JNT_SLIDE)) {
                const double q = S.qpos[pf_jqadr];
                lo = q - pf_jlo < pf_jmargin;
                hi = pf_jhi - q < pf_jmargin;
            }
            lob = wv::ballot(lo); hib = wv::ballot(hi);
        }
        if constexpr (MAXR < WIDE_ROWS) {
            /* an upper bound of the rows this substep needs (the caps of the row assignment can only lower it): past this
             * instantiation's capacity -- rows or contacts -- the env is handed to the next instantiation, from the start of this substep */
            const bool may_go_down = io.down_rows > 0 && sub > sub_start;     /* (the substep this call was entered for needed the rows) */
            if (can_hand_over || may_go_down) {
                const int neq = m->neq;
                const bool eact = lane < neq && m->eq_active[lane < neq ? lane : 0] != 0;
                /* (a frictionless contact -- condim 1: Cassie's leg against leg -- is one row, a pyramidal one four: counting every
                 * contact as four handed substeps over that fit) */
                wv::sync();
                const int nfrictionless = wv::popc64(wv::ballot(lane < ncon && S.c_dim[lane < MAXC ? lane : 0] == 1));
                const int need = 3 * wv::popc64(wv::ballot(eact)) + wv::popc64(lob) + wv::popc64(hib) + 4 * ncon - 3 * nfrictionless;
                /* (more contacts than this instantiation's list holds are a reason only if the next one's list is longer: the 63-row
                 * pass behind a 31-row kernel has the same 16 slots and could only cap the list the same way) */
                const bool up = can_hand_over && (need > capr || (ncon_found > capc && MAXC < m->maxcon));
                /* (round 6, the 63-row code inside the fast kernel: the substep fits the fast code again -- leave, the way a hand-over leaves) */
                const bool down = !up && may_go_down && need <= io.down_rows;
                if (up || down) {
                    bailed = true; bailed_down = down;
                    if constexpr (NW == 2) { if (lane == 0) S.cmd[0] = 1; wv::publish(&S.cmd[4], sub + 1); } /* (the verdict: handed over) */
                    break;
                }
            }
        }
        if (ncon_found > capc) warn |= WARN_CONTACT_FULL;
        if constexpr (NW == 1) if (io.drive_mode) {
            if (integrates<FEAT>(io)) drive_level_io(io, S, m, env, lane, lastsub); /* mj_forward leaves the drive-level state alone */
            wv::sync();
        }
        if constexpr (NW == 2) { CK_STAMP(33); wv::publish(&S.cmd[4], sub + 1); wv::wait_for(&S.cmd[3], sub + 1); } /* the verdict for wave 1; wave 1's com / cinert / cdof for the stage below */
        CK_STAMP(5);

