/*
 * depth_jobs.inc -- the body of the two depth-image kernels (depth_kernel.h), included once per kernel with `SCENE` a constant in
 * scope: false for cassie_depth_kernel (static planes, boxes and the height field: every `if (SCENE)` below drops out), true for
 * cassie_depth_scene_kernel (the geoms of DepthIO::geoms, moving bodies included).  It holds the camera, the pixel, which geoms are
 * rendered, the lane reads of their frames, the sphere's shortcut and the stores; the cull and the ray against a geom are scene_rays.h's.
 * THE RULE: code the kernels share takes values, never the argument struct.  This text is an include and not a function of `io`
 * because a function that takes DepthIO, inlined into a kernel, has the compiler fetch the launch arguments in other portions, and
 * the static kernel parks six more scalar registers; functions of plain values (pointers, doubles, flags) cost it none (DESIGN 4.3).
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
        const bool mine = r < H && c < W;                   /* (a lane past the image's edge has no ray) */
        const double aspect = (double)W / (double)H;
        const double dc[3] = {aspect * io.tan_half * (2.0 * (c + 0.5) / W - 1.0), io.tan_half * (1.0 - 2.0 * (r + 0.5) / H), -1.0};
        double D[3];
        mulmatvec3(D, Rc, dc);
        bool clamped;
        const float *grid = terrain_grid(io.hfield, io.hfield_stride, io.hfield_index, io.hfield_nterrain, env, &clamped);
        double best = io.zfar;
        int best_id = -1;
        /* (scene) lane g's own geom: its world position and rotation, where it is rendered (zero for a moving geom without body poses) */
        double fp[3] = {0.0, 0.0, 0.0}, fR[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (SCENE) {
            if (lane < m->ngeom && ((io.geoms >> lane) & 1u)) {
                if (m->body_weldid[m->geom_bodyid[lane]] == 0) static_geom_pose(m, PG, lane, fp, fR);
                else if (io.xpos && io.xquat) scene_geom_frame(m, PG, lane, io.xpos + (size_t)env * io.sxp, io.xquat + (size_t)env * io.sxq, fp, fR);
            }
        }
        const double DD = SCENE ? dot3(D, D) : 0.0;
        for (int g = 0; g < m->ngeom; ++g) {              /* (the same trip for every lane: the geom's pose is the wave's, not the lane's) */
            const int gt = m->geom_type[g];
            const bool solid = gt == CM_GEOM_SPHERE || gt == CM_GEOM_CAPSULE || gt == CM_GEOM_BOX;
            double gp[3], R[9];
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
            bool live = mine;
            if (SCENE && solid) {
                double e0, e1;
                const bool meets = scene_ray_bound(m, g, rel, D, DD, mine, io.znear, best, &e0, &e1);
                if (wv::ballot(meets) == 0ull) continue;
                if (gt == CM_GEOM_SPHERE) {                 /* (the shortcut: the bound is the test; kept in the loop, scene_rays.h says why) */
                    if (meets) t = depth_convex(e0, e1, io.znear, t);
                    if (t >= io.znear && t < best) { best = t; best_id = g; }
                    continue;
                }
                live = meets;
            }
            bool inside;                                    /* (`near` from inside a solid is a depth like any other) */
            t = scene_ray_geom<SCENE>(m, g, R, rel, D, live, io.znear, io.zfar, t, grid, &inside);
            if (t >= io.znear && t < best) { best = t; if (SCENE) best_id = g; }
        }
        if (mine) io.out[(size_t)env * io.sout + (size_t)r * W + c] = best;
        if (SCENE && io.ids && mine) io.ids[(size_t)env * ((size_t)W * H) + (size_t)r * W + c] = best_id;
        if (clamped && tile == 0 && lane == 0) wv::atomic_or(io.warn + env, WARN_TERRAIN_INDEX);
    }
