/*
 * depth_jobs.inc -- the body of the two depth-image kernels (depth_kernel.h), included once per kernel with `SCENE` a constant in
 * scope: false for cassie_depth_kernel (static planes, boxes and the height field: every `if (SCENE)` below drops out and the text
 * that is left is the static kernel's own), true for cassie_depth_scene_kernel (the geoms of DepthIO::geoms, moving bodies included).
 * A shared function would do for the text, but not for the code: inlined into a kernel, the compiler fetches the launch arguments
 * in other portions and the static kernel spills six more scalar registers.
 */
    const int lane = wv::lane();
    const int W = io.width, H = io.height;
    const int tiles_x = (W + DEPTH_TILE - 1) / DEPTH_TILE, tiles = tiles_x * ((H + DEPTH_TILE - 1) / DEPTH_TILE);
    const long long njobs = (long long)io.n * tiles;
    for (long long job = wv::env_id(); job < njobs; job += wv::grid_size()) {
        const int env = io.env0 + (int)(job / tiles), tile = (int)(job % tiles);
        const ModelPtr m = env_model(io.models, io.model_stride, env);
        const ParamPtr PG = env_geometry(io.envparams, m, (size_t)env);
        /* the camera's world pose (wave-uniform) */
        double bp[3], bq[4], Rb[9], cp[3], cq[4], wq[4], Rc[9], off[3];
        static_body_pose(m, io.body, io.qpos + (size_t)env * io.sq, bp, bq);
        const double *own = io.pose ? io.pose + (size_t)env * 7 : nullptr;
        for (int k = 0; k < 3; ++k) cp[k] = own ? own[k] : io.cam_pos[k];
        for (int k = 0; k < 4; ++k) cq[k] = own ? own[3 + k] : io.cam_quat[k];
        normalize4(cq);
        quat2mat(Rb, bq);
        mulmatvec3(off, Rb, cp);
        mulquat(wq, bq, cq);
        quat2mat(Rc, wq);
        const double o[3] = {bp[0] + off[0], bp[1] + off[1], bp[2] + off[2]};
        /* this lane's pixel and its ray */
        const int r = (tile / tiles_x) * DEPTH_TILE + (lane >> 3), c = (tile % tiles_x) * DEPTH_TILE + (lane & 7);
        const bool mine = r < H && c < W;
        const double aspect = (double)W / (double)H;
        const double dc[3] = {aspect * io.tan_half * (2.0 * (c + 0.5) / W - 1.0), io.tan_half * (1.0 - 2.0 * (r + 0.5) / H), -1.0};
        double D[3];
        mulmatvec3(D, Rc, dc);
        bool clamped;
        const float *grid = terrain_grid(io.hfield, io.hfield_stride, io.hfield_index, io.hfield_nterrain, env, &clamped);
        double best = io.zfar;
        int best_id = -1;
        /* (scene) lane g's own geom: its world position and rotation, where it is rendered */
        double fp[3] = {0.0, 0.0, 0.0}, fR[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (SCENE) {
            if (lane < m->ngeom && ((io.geoms >> lane) & 1u)) {
                const int B = m->geom_bodyid[lane];
                if (m->body_weldid[B] == 0) static_geom_pose(m, PG, lane, fp, fR);
                else if (io.xpos && io.xquat) {
                    const double *xp = io.xpos + (size_t)env * io.sxp + 3 * B, *xq = io.xquat + (size_t)env * io.sxq + 4 * B;
                    const double q[4] = {xq[0], xq[1], xq[2], xq[3]}, lp[3] = {PG->geom_pos[lane][0], PG->geom_pos[lane][1], PG->geom_pos[lane][2]};
                    double RB[9], w[3];
                    quat2mat(RB, q);
                    mulmatvec3(w, RB, lp);
                    for (int k = 0; k < 3; ++k) fp[k] = xp[k] + w[k];
                    for (int r_ = 0; r_ < 3; ++r_)
                        for (int c_ = 0; c_ < 3; ++c_)
                            fR[3 * r_ + c_] = RB[3 * r_] * PG->geom_mat[lane][c_] + RB[3 * r_ + 1] * PG->geom_mat[lane][3 + c_] + RB[3 * r_ + 2] * PG->geom_mat[lane][6 + c_];
                }
            }
        }
        const double DD = SCENE ? dot3(D, D) : 0.0;
        for (int g = 0; g < m->ngeom; ++g) {              /* (the same trip for every lane: the geom's pose is the wave's, not the lane's) */
            const int gt = m->geom_type[g];
            const bool solid = gt == CM_GEOM_SPHERE || gt == CM_GEOM_CAPSULE || gt == CM_GEOM_BOX;
            double gp[3], R[9], og[3], dg[3];
            if (!SCENE) {
                if (m->body_weldid[m->geom_bodyid[g]] != 0 || (gt != CM_GEOM_PLANE && gt != CM_GEOM_BOX && gt != CM_GEOM_HFIELD)) continue;
                static_geom_pose(m, PG, g, gp, R);
            } else {
                if (!((io.geoms >> g) & 1u)) continue;
                const bool moving = m->body_weldid[m->geom_bodyid[g]] != 0;
                if (moving ? !(solid && io.xpos && io.xquat) : !(solid || gt == CM_GEOM_PLANE || gt == CM_GEOM_HFIELD)) continue;
                for (int k = 0; k < 3; ++k) gp[k] = wv::readlane(fp[k], g);
                for (int k = 0; k < 9; ++k) R[k] = wv::readlane(fR[k], g);
            }
            const double rel[3] = {o[0] - gp[0], o[1] - gp[1], o[2] - gp[2]};
            double t = io.zfar + 1.0;
            bool live = mine;                               /* (a lane past the image's edge has no ray) */
            if (SCENE && solid) {
                /* the bounding sphere (the sphere itself): who meets it at all, in range and in front of the best so far */
                const double rb = gt == CM_GEOM_SPHERE ? m->geom_size[g][0] : m->geom_rbound[g] + DEPTH_CULL_PAD;
                double e0 = 0.0, e1 = 0.0;
                const bool meets = mine && depth_ray_round(rel, D, DD, rb * rb, &e0, &e1) && e1 >= io.znear && e0 < best;
                if (wv::ballot(meets) == 0ull) continue;
                if (gt == CM_GEOM_SPHERE) {
                    if (meets) t = depth_convex(e0, e1, io.znear, t);
                    if (t >= io.znear && t < best) { best = t; best_id = g; }
                    continue;
                }
                live = meets;
            }
            mulmatTvec3(og, R, rel);
            mulmatTvec3(dg, R, D);
            if (!live) {
            } else if (gt == CM_GEOM_PLANE) {
                if (dg[2] != 0.0) t = -og[2] / dg[2];
            } else if (gt == CM_GEOM_BOX) {
                double t0 = -1e300, t1 = 1e300;
                bool inside = true;
                for (int k = 0; k < 3; ++k) {
                    const double s = m->geom_size[g][k];
                    if (dg[k] != 0.0) {
                        const double ta = (-s - og[k]) / dg[k], tb = (s - og[k]) / dg[k];
                        const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
                        t0 = lo > t0 ? lo : t0; t1 = hi < t1 ? hi : t1;
                    } else if (fabs(og[k]) > s) inside = false;
                }
                if (inside && t0 <= t1) t = t0 >= io.znear ? t0 : (t1 >= io.znear ? io.znear : t);
            } else if (SCENE && gt == CM_GEOM_CAPSULE) {
                double t0, t1;
                if (depth_ray_capsule(og, dg, m->geom_size[g][0], m->geom_size[g][1], &t0, &t1)) t = depth_convex(t0, t1, io.znear, t);
            } else if (grid && m->hfield_nrow >= 2 && m->hfield_ncol >= 2) {
                t = depth_ray_hfield(grid, m->hfield_nrow, m->hfield_ncol, m->hfield_size[0], m->hfield_size[1], m->hfield_size[2], og, dg,
                                     io.znear, io.zfar);
            }
            if (t >= io.znear && t < best) { best = t; if (SCENE) best_id = g; }
        }
        if (mine) io.out[(size_t)env * io.sout + (size_t)r * W + c] = best;
        if (SCENE && io.ids && mine) io.ids[(size_t)env * ((size_t)W * H) + (size_t)r * W + c] = best_id;
        if (clamped && tile == 0 && lane == 0) wv::atomic_or(io.warn + env, WARN_TERRAIN_INDEX);
    }
