/*
 * wave_bodies.h -- TEST-ONLY bodies that exercise, one at a time and written against wv:: and ck:: exactly as the step
 * kernel is:
 *   - the wavefront primitives of wave.h (sums, DPP moves, readlane / writelane, shuffles, ballot, the matrix core, max_raw,
 *     the reciprocal and reciprocal-square-root seeds);
 *   - the elementary functions of pk_math.h (normalize4_fast, normalize3_fast, sincos_reduced / sincos_bounded);
 *   - all of pk_factor_solve.h: fast_rcp, the two L^T D L factorisations in both forms (factor_pair_in_registers for the
 *     run-time topology, factor_pair_by_height for Cassie-32 and the packed tray model, interleaved and split), the packed rows
 *     read back as the kernel stages them (stage_factor_row / stage_factor_h of pk_stages.h) into solve_forward /
 *     solve_backward, and one sweep of pgs_rows and of pgs_rows_fast at the three row counts the kernel instantiates.
 *   - the narrow phase of pk_collision.h.  Lane = trial (64 different trials to a wave, so that the lanes diverge into different
 *     branches): plane_sphere, sphere_sphere, segment_closest, point_box, sphere_box, capsule_box, closest_on_triangle,
 *     hfield_triangle folded over the two triangles of a grid cell the way hfield_sphere does, make_frame, impedance.  Wave = trial:
 *     box_box_lane at keepmax 4 and 8, called by all 64 lanes as in the kernel, every lane storing its keep flag and its contact.
 * Not covered here: wide_solve and the convergence logic around the sweeps (they need the step kernel's shared state);
 * hfield_sphere, hfield_spheres_wave, hfield_prism_wave and finish_contacts (they need the model and the shared state:
 * tests/test_hfield.py holds them to a numpy brute force through the emulator); the pair types env_step_collision.inc assembles
 * inline (plane-capsule, sphere-capsule, plane-box).
 *
 * The same source is compiled twice: for gfx950 with the product's flags (wave_check.hip: one workgroup of one wave per
 * trial) and into the CPU wave emulator (tests/emu/emu_runtime.cpp: the body runs through the emulator's rendezvous
 * scheduler).  tests/wave_check.py loads either and tests/test_wave_primitives.py compares both with exact references.
 *
 * A body gets its trial's slice of the buffers: input k of lane l is in[64 k + l], output k of lane l is out[64 k + l].
 * WAVE_CHECK_BODIES lists every body as X(name, inputs per lane, outputs per lane).  The bodies of WAVE_CHECK_AUX_BODIES take
 * a third argument: a read-only block of bytes every trial of a call shares (wc::FactorAux: the model the factorisations read).
 */
#ifndef CASSIE_WAVE_BODIES_H
#define CASSIE_WAVE_BODIES_H

#include <cstddef>
#include <cstring>

#define WAVE_CHECK_BODIES(X) \
    X(wave_sum, 1, 1)        \
    X(wave_sum_f32, 1, 1)    \
    X(dpp_take, 2, 12)       \
    X(readlane, 2, 1)        \
    X(writelane, 3, 4)       \
    X(from_upper_half, 1, 1) \
    X(shfl, 3, 8)            \
    X(ballot, 1, 3)          \
    X(mfma1, 6, 4)           \
    X(mfma4, 12, 4)          \
    X(max_raw, 2, 1)         \
    X(estimates, 1, 2)       \
    X(fast_rcp, 1, 1)        \
    X(normalize4_fast, 4, 4) \
    X(normalize3_fast, 3, 4) \
    X(sincos, 1, 4)          \
    X(solve_rt, 2 * 40 + 3, 2)     \
    X(solve_cassie, 2 * 32 + 3, 2) \
    X(solve_tray, 2 * 40 + 3, 2)   \
    X(pgs_guarded32, 32 + 5, 3)    \
    X(pgs_guarded48, 48 + 5, 3)    \
    X(pgs_guarded64, 64 + 5, 3)    \
    X(pgs_fast32, 32 + 5, 2)       \
    X(pgs_fast48, 48 + 5, 2)       \
    X(pgs_fast64, 64 + 5, 2)       \
    X(plane_sphere, 17, 11)        \
    X(sphere_sphere, 9, 11)        \
    X(segment_closest, 14, 2)      \
    X(point_box, 18, 4)            \
    X(sphere_box, 20, 11)          \
    X(capsule_box, 30, 21)         \
    X(closest_on_triangle, 12, 3)  \
    X(hfield_triangle, 15, 8)      \
    X(make_frame, 6, 9)            \
    X(impedance, 7, 1)             \
    X(box_box4, 31, 11)            \
    X(box_box8, 31, 11)

#define WAVE_CHECK_AUX_BODIES(X)                                                       \
    X(factor_rt, 2 * 40, (wc::factor_set_rows<40, ck::TopoRuntime>()))                \
    X(factor_cassie, 2 * 32, (2 * wc::factor_set_rows<32, ck::TopoCassie32>()))       \
    X(factor_tray, 2 * 40, (2 * wc::factor_set_rows<40, ck::TopoCassieTray38>()))

namespace wc {

/* what the factorisations read of a model: the auxiliary block of the factor_* bodies.  P = the model's own parameter block. */
struct FactorAux { cm_model_t model; double h; };
/* the part of EnvShared the factorisations and the solves' staging touch: LDS on the device, one static block in the emulator
 * (whose trials run one after the other) */
template <int NVP, class TOPO>
struct FactorShared {
    double Lp[ck::LPack<TOPO, NVP>::count], LHp[ck::LPack<TOPO, NVP>::count];
    double dinv[NVP], dinvH[NVP], rsd[NVP];
};
/* NaN into every word, so that a slot nobody wrote shows (LDS is not initialised, and the emulator's block is the last trial's) */
template <class SH> WV_DEVICE void poison(SH &S) {
    double *p = (double *)&S;
    wv::sync();
    for (int i = wv::lane(); i < (int)(sizeof(SH) / sizeof(double)); i += 64) p[i] = __builtin_nan("");
    wv::sync();
}
/* one set of a factor body's outputs, in rows of 64: Lp, LHp (rows_of_pack each), dinv, dinvH, rsd, col[NVP], colh[NVP] */
template <int NVP, class TOPO> constexpr int rows_of_pack() { return (ck::LPack<TOPO, NVP>::count + 63) / 64; }
template <int NVP, class TOPO> constexpr int factor_set_rows() { return 2 * rows_of_pack<NVP, TOPO>() + 3 + 2 * NVP; }
template <int NVP, class TOPO, class SH>
WV_DEVICE void factor_write(const SH &S, const double (&col)[NVP], const double (&colh)[NVP], double *out) {
    constexpr int C = ck::LPack<TOPO, NVP>::count, R = rows_of_pack<NVP, TOPO>();
    const int l = wv::lane();
    wv::sync();
    for (int i = l; i < C; i += 64) { out[i] = S.Lp[i]; out[R * 64 + i] = S.LHp[i]; }
    if (l < NVP) { out[2 * R * 64 + l] = S.dinv[l]; out[(2 * R + 1) * 64 + l] = S.dinvH[l]; out[(2 * R + 2) * 64 + l] = S.rsd[l]; }
#pragma unroll
    for (int i = 0; i < NVP; ++i) { out[(2 * R + 3 + i) * 64 + l] = col[i]; out[(2 * R + 3 + NVP + i) * 64 + l] = colh[i]; }
}
/* the two matrices, one column per lane: inputs i and NVP + i of lane j are M[i][j] and (M + hB)[i][j] less their diagonal
 * terms, i >= j (the rest is never read) */
template <int NVP> WV_DEVICE void factor_read(const double *in, double (&col)[NVP], double (&colh)[NVP]) {
    const int l = wv::lane();
#pragma unroll
    for (int i = 0; i < NVP; ++i) { col[i] = in[i * 64 + l]; colh[i] = in[(NVP + i) * 64 + l]; }
}
/* factor_pair_in_registers on the run-time topology: nv, the ancestor masks, armature and damping are the aux model's.  The
 * factors stay in col / colh (entry (k, j) in col[k] of lane j); Lp / LHp of the output set stay NaN. */
WV_DEVICE void factor_rt(const double *in, double *out, const void *aux) {
    WV_SHARED FactorShared<40, ck::TopoRuntime> S;
    const FactorAux *a = (const FactorAux *)aux;
    const ck::ModelPtr m = (ck::ModelPtr)&a->model;
    const ck::ParamPtr P = (ck::ParamPtr)&m->params;
    double col[40], colh[40];
    factor_read<40>(in, col, colh);
    poison(S);
    ck::factor_pair_in_registers<40, ck::TopoRuntime>(m, P, a->h, col, colh, wv::lane(), m->nv, S.dinv, S.rsd, S.dinvH);
    factor_write<40, ck::TopoRuntime>(S, col, colh, out);
}
/* factor_pair_by_height: both factorisations interleaved (the first output set), then, on a fresh copy of the inputs and a
 * poisoned block, that of M followed by that of M + hB as the two-wave form runs them (the second set) */
template <int NVP, class TOPO> WV_DEVICE void factor_static(const double *in, double *out, const void *aux) {
    WV_SHARED FactorShared<NVP, TOPO> S;
    const FactorAux *a = (const FactorAux *)aux;
    const ck::ModelPtr m = (ck::ModelPtr)&a->model;
    const ck::ParamPtr P = (ck::ParamPtr)&m->params;
    const double h = a->h;
    const int l = wv::lane();
    double col[NVP], colh[NVP];
    factor_read<NVP>(in, col, colh);
    poison(S);
    ck::factor_pair_by_height<NVP, TOPO, 2>(m, P, h, S, col, colh, l);
    factor_write<NVP, TOPO>(S, col, colh, out);
    factor_read<NVP>(in, col, colh);
    poison(S);
    ck::factor_pair_by_height<NVP, TOPO, 0>(m, P, h, S, col, colh, l);
    ck::factor_pair_by_height<NVP, TOPO, 1>(m, P, h, S, col, colh, l);
    factor_write<NVP, TOPO>(S, col, colh, out + factor_set_rows<NVP, TOPO>() * 64);
}
WV_DEVICE void factor_cassie(const double *in, double *out, const void *aux) { factor_static<32, ck::TopoCassie32>(in, out, aux); }
WV_DEVICE void factor_tray(const double *in, double *out, const void *aux) { factor_static<40, ck::TopoCassieTray38>(in, out, aux); }

/* solve_forward on z with the factor of inputs 0 .. NVP - 1, solve_backward on w with that of inputs NVP .. 2 NVP - 1 (entry
 * (k, j) of a unit-triangular factor = input k of lane j, as the factorisations leave it; parked in Lp / LHp the way they park
 * it, and staged into the lane's row / column the way the kernel stages it); then z, w, nv (read by the run-time form only) */
template <int NVP, class TOPO> WV_DEVICE void solve_body(const double *in, double *out) {
    typedef ck::LPack<TOPO, NVP> LP;
    WV_SHARED FactorShared<NVP, TOPO> S;
    const int l = wv::lane();
    const int nv = TOPO::is_static ? TOPO::nv : (int)wv::readlane(in[(2 * NVP + 2) * 64 + l], 0);
    poison(S);
#pragma unroll
    for (int k = 0; k < NVP; ++k) {
        const int at = LP::row_slot(k, l);
        S.Lp[at] = in[k * 64 + l];
        S.LHp[at] = in[(NVP + k) * 64 + l];
    }
    wv::sync();
    const bool isdof = l < nv;
    double lrow[NVP], lcol[NVP], lrowh[NVP];
    ck::stage_factor_row<NVP, TOPO>(S, l, isdof, lrow);
    ck::stage_factor_h<NVP, TOPO, 0>(S, l, isdof, nv, lcol, lrowh);
    out[l] = ck::solve_forward<NVP, TOPO>(in[2 * NVP * 64 + l], lrow, l, nv);
    out[64 + l] = ck::solve_backward<NVP, TOPO>(in[(2 * NVP + 1) * 64 + l], lcol, l, nv);
}
WV_DEVICE void solve_rt(const double *in, double *out) { solve_body<40, ck::TopoRuntime>(in, out); }
WV_DEVICE void solve_cassie(const double *in, double *out) { solve_body<32, ck::TopoCassie32>(in, out); }
WV_DEVICE void solve_tray(const double *in, double *out) { solve_body<40, ck::TopoCassieTray38>(in, out); }

/* one sweep of the projected Gauss-Seidel chain, lane = row, in the scaled domain the solve stage hands it: inputs 0 .. N - 1
 * are the lane's brow, then nrows (the same in every lane), Aii, flo, f, sres */
template <int N> WV_DEVICE void pgs_guarded(const double *in, double *out) {
    const int l = wv::lane();
    double brow[N];
#pragma unroll
    for (int t = 0; t < N; ++t) brow[t] = in[t * 64 + l];
    const int nrows = (int)wv::readlane(in[N * 64 + l], 0); /* wave-uniform, in a scalar register as the kernel's is */
    const double Aii = in[(N + 1) * 64 + l], flo = in[(N + 2) * 64 + l];
    double f = in[(N + 3) * 64 + l], sres = in[(N + 4) * 64 + l], improvement = 0;
    ck::pgs_rows<0, N>(brow, nrows, l, Aii, 0.5 * Aii, flo, f, sres, improvement);
    out[l] = f;
    out[64 + l] = sres;
    out[128 + l] = improvement;
}
template <int N> WV_DEVICE void pgs_fast(const double *in, double *out) {
    const int l = wv::lane();
    double brow[N];
#pragma unroll
    for (int t = 0; t < N; ++t) brow[t] = in[t * 64 + l];
    const int nrows = (int)wv::readlane(in[N * 64 + l], 0); /* wave-uniform, in a scalar register as the kernel's is */
    const double flo = in[(N + 2) * 64 + l], f = in[(N + 3) * 64 + l];
    double sres = in[(N + 4) * 64 + l], mys = 0;
    ck::pgs_rows_fast<0, N>(brow, nrows, l, flo - f, sres, mys);
    out[l] = sres;
    out[64 + l] = mys;
}
static_assert(ck::FAST_ROWS + 1 == 32 && ck::FAST_ROWS_TRAY + 1 == 48 && ck::NROW == 64, "the row counts the kernel instantiates the sweeps at");
WV_DEVICE void pgs_guarded32(const double *in, double *out) { pgs_guarded<32>(in, out); }
WV_DEVICE void pgs_guarded48(const double *in, double *out) { pgs_guarded<48>(in, out); }
WV_DEVICE void pgs_guarded64(const double *in, double *out) { pgs_guarded<64>(in, out); }
WV_DEVICE void pgs_fast32(const double *in, double *out) { pgs_fast<32>(in, out); }
WV_DEVICE void pgs_fast48(const double *in, double *out) { pgs_fast<48>(in, out); }
WV_DEVICE void pgs_fast64(const double *in, double *out) { pgs_fast<64>(in, out); }

/* ---- the narrow phase (pk_collision.h).  Inputs are the routine's arguments in their order, vectors and matrices element by
 * element (matrices row-major, as the kernel holds them).  A contact is stored as dist, pos, normal, tangent (10 values); a
 * contact the routine did not write stays NaN. ---- */
template <int N> WV_DEVICE void take(const double *in, int &row, double (&v)[N]) {
    const int l = wv::lane();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = in[(row + i) * 64 + l];
    row += N;
}
WV_DEVICE double take(const double *in, int &row) { return in[(row++) * 64 + wv::lane()]; }
WV_DEVICE void blank(ck::RawContact &c) {
    const double nan = __builtin_nan("");
    c.dist = nan;
    for (int i = 0; i < 3; ++i) c.pos[i] = c.normal[i] = c.tangent[i] = nan;
}
WV_DEVICE void put(double *out, int row, const ck::RawContact &c) {
    const int l = wv::lane();
    out[row * 64 + l] = c.dist;
    for (int i = 0; i < 3; ++i) { out[(row + 1 + i) * 64 + l] = c.pos[i]; out[(row + 4 + i) * 64 + l] = c.normal[i]; out[(row + 7 + i) * 64 + l] = c.tangent[i]; }
}
/* lane = trial: the count, then the contact */
WV_DEVICE void plane_sphere(const double *in, double *out) {
    int row = 0;
    double ppos[3], pmat[9], spos[3];
    take(in, row, ppos); take(in, row, pmat); take(in, row, spos);
    const double r = take(in, row), margin = take(in, row);
    ck::RawContact c;
    blank(c);
    out[wv::lane()] = (double)ck::plane_sphere(c, ppos, pmat, spos, r, margin);
    put(out, 1, c);
}
WV_DEVICE void sphere_sphere(const double *in, double *out) {
    int row = 0;
    double p1[3], p2[3];
    take(in, row, p1);
    const double r1 = take(in, row);
    take(in, row, p2);
    const double r2 = take(in, row), margin = take(in, row);
    ck::RawContact c;
    blank(c);
    out[wv::lane()] = (double)ck::sphere_sphere(c, p1, r1, p2, r2, margin);
    put(out, 1, c);
}
/* the two parameters */
WV_DEVICE void segment_closest(const double *in, double *out) {
    int row = 0;
    double p1[3], a1[3], p2[3], a2[3];
    take(in, row, p1); take(in, row, a1);
    const double l1 = take(in, row);
    take(in, row, p2); take(in, row, a2);
    const double l2 = take(in, row);
    double x1 = __builtin_nan(""), x2 = __builtin_nan("");
    ck::segment_closest(p1, a1, l1, p2, a2, l2, x1, x2);
    out[wv::lane()] = x1;
    out[64 + wv::lane()] = x2;
}
/* the signed distance, then the outward normal in world axes */
WV_DEVICE void point_box(const double *in, double *out) {
    int row = 0;
    double q[3], pb[3], mb[9], sb[3], nw[3];
    take(in, row, q); take(in, row, pb); take(in, row, mb); take(in, row, sb);
    const int l = wv::lane();
    out[l] = ck::point_box(q, pb, mb, sb, nw);
    for (int i = 0; i < 3; ++i) out[(1 + i) * 64 + l] = nw[i];
}
WV_DEVICE void sphere_box(const double *in, double *out) {
    int row = 0;
    double ps[3], pb[3], mb[9], sb[3];
    take(in, row, ps);
    const double r = take(in, row);
    take(in, row, pb); take(in, row, mb); take(in, row, sb);
    const double margin = take(in, row);
    ck::RawContact c;
    blank(c);
    out[wv::lane()] = (double)ck::sphere_box(c, ps, r, pb, mb, sb, margin);
    put(out, 1, c);
}
/* the count, then both contacts */
WV_DEVICE void capsule_box(const double *in, double *out) {
    int row = 0;
    double pc[3], mc[9], pb[3], mb[9], sb[3];
    take(in, row, pc); take(in, row, mc);
    const double rad = take(in, row), h = take(in, row);
    take(in, row, pb); take(in, row, mb); take(in, row, sb);
    const double margin = take(in, row);
    ck::RawContact c0, c1;
    blank(c0); blank(c1);
    out[wv::lane()] = (double)ck::capsule_box(c0, c1, pc, mc, rad, h, pb, mb, sb, margin);
    put(out, 1, c0);
    put(out, 11, c1);
}
WV_DEVICE void closest_on_triangle(const double *in, double *out) {
    int row = 0;
    double p[3], a[3], b[3], c[3], q[3];
    take(in, row, p); take(in, row, a); take(in, row, b); take(in, row, c);
    ck::closest_on_triangle(p, a, b, c, q);
    for (int i = 0; i < 3; ++i) out[i * 64 + wv::lane()] = q[i];
}
/* the centre p against the two triangles of the cell with corners v00, v10, v01, v11, from the start values and in the order of
 * hfield_sphere: best, bv, bdiv, then the normal the caller forms (bdiv ? bv / best : bv) */
WV_DEVICE void hfield_triangle(const double *in, double *out) {
    int row = 0;
    double p[3], v00[3], v10[3], v01[3], v11[3];
    take(in, row, p); take(in, row, v00); take(in, row, v10); take(in, row, v01); take(in, row, v11);
    double best = 1e300, bv[3] = {0, 0, 1};
    bool bdiv = false;
    ck::hfield_triangle(p, v00, v10, v01, best, bv, bdiv);
    ck::hfield_triangle(p, v11, v01, v10, best, bv, bdiv);
    const int l = wv::lane();
    out[l] = best;
    for (int i = 0; i < 3; ++i) { out[(1 + i) * 64 + l] = bv[i]; out[(5 + i) * 64 + l] = bdiv ? bv[i] / best : bv[i]; }
    out[4 * 64 + l] = bdiv ? 1.0 : 0.0;
}
/* the normal and the tangent hint in, the three rows of the frame out */
WV_DEVICE void make_frame(const double *in, double *out) {
    int row = 0;
    double six[6], fr[9];
    take(in, row, six);
    for (int i = 0; i < 6; ++i) fr[i] = six[i];
    fr[6] = fr[7] = fr[8] = 0;
    ck::make_frame(fr);
    for (int i = 0; i < 9; ++i) out[i * 64 + wv::lane()] = fr[i];
}
WV_DEVICE void impedance(const double *in, double *out) {
    int row = 0;
    double solimp[5];
    take(in, row, solimp);
    const double pos = take(in, row), margin = take(in, row);
    out[wv::lane()] = ck::impedance(solimp, pos, margin);
}
/* wave = trial: every lane holds the same two boxes and the margin, all 64 lanes call (lane = candidate, as in the kernel); each
 * lane stores whether it keeps a contact, then its contact */
template <int KEEPMAX> WV_DEVICE void box_box(const double *in, double *out) {
    int row = 0;
    double p1[3], m1[9], s1[3], p2[3], m2[9], s2[3];
    take(in, row, p1); take(in, row, m1); take(in, row, s1); take(in, row, p2); take(in, row, m2); take(in, row, s2);
    const double margin = take(in, row);
    ck::RawContact c;
    blank(c);
    const bool keep = ck::box_box_lane(c, wv::lane(), p1, m1, s1, p2, m2, s2, margin, KEEPMAX);
    out[wv::lane()] = keep ? 1.0 : 0.0;
    put(out, 1, c);
}
WV_DEVICE void box_box4(const double *in, double *out) { box_box<4>(in, out); }
WV_DEVICE void box_box8(const double *in, double *out) { box_box<8>(in, out); }

/* the wave-uniform sum, stored by every lane */
WV_DEVICE void wave_sum(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::wave_sum(in[l]);
}
/* ... in single precision (inputs and result are floats carried in doubles, which is exact) */
WV_DEVICE void wave_sum_f32(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = (double)wv::wave_sum_f32((float)in[l]);
}
/* each DPP move of the two sums, with the row mask the sum gives it: the doubles of input 0, then the floats of input 1 */
WV_DEVICE void dpp_take(const double *in, double *out) {
    const int l = wv::lane();
    const double v = in[l];
    const float f = (float)in[64 + l];
    out[0 * 64 + l] = wv::dpp_take<0xB1, 0xf>(v);
    out[1 * 64 + l] = wv::dpp_take<0x4E, 0xf>(v);
    out[2 * 64 + l] = wv::dpp_take<0x141, 0xf>(v);
    out[3 * 64 + l] = wv::dpp_take<0x140, 0xf>(v);
    out[4 * 64 + l] = wv::dpp_take<0x142, 0xa>(v);
    out[5 * 64 + l] = wv::dpp_take<0x143, 0xc>(v);
    out[6 * 64 + l] = (double)wv::dpp_take_f32<0xB1, 0xf>(f);
    out[7 * 64 + l] = (double)wv::dpp_take_f32<0x4E, 0xf>(f);
    out[8 * 64 + l] = (double)wv::dpp_take_f32<0x141, 0xf>(f);
    out[9 * 64 + l] = (double)wv::dpp_take_f32<0x140, 0xf>(f);
    out[10 * 64 + l] = (double)wv::dpp_take_f32<0x142, 0xa>(f);
    out[11 * 64 + l] = (double)wv::dpp_take_f32<0x143, 0xc>(f);
}
/* broadcast of lane src; src is read from memory (every lane holds the same value), so it is wave-uniform at run time
 * but no compile-time constant (the compiler takes it from the first lane: v_readfirstlane, then v_readlane) */
WV_DEVICE void readlane(const double *in, double *out) {
    const int l = wv::lane();
    const int src = (int)in[64 + l];
    out[l] = wv::readlane(in[l], src);
}
/* writelane into a value the instruction just before it wrote (v = x + y); s is wave-uniform (every lane holds it) */
WV_DEVICE void writelane(const double *in, double *out) {
    const int l = wv::lane();
    const double s = in[128 + l];
    const double v = in[l] + in[64 + l];
    out[0 * 64 + l] = wv::writelane<0>(v, s);
    out[1 * 64 + l] = wv::writelane<31>(v, s);
    out[2 * 64 + l] = wv::writelane<32>(v, s);
    out[3 * 64 + l] = wv::writelane<63>(v, s);
}
WV_DEVICE void from_upper_half(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::from_upper_half(in[l]);
}
/* shfl from a per-lane source (input 1), its integer form on input 2, shfl_xor with the masks 1 .. 32 */
WV_DEVICE void shfl(const double *in, double *out) {
    const int l = wv::lane();
    const double v = in[l];
    const int src = (int)in[64 + l];
    out[0 * 64 + l] = wv::shfl(v, src);
    out[1 * 64 + l] = (double)wv::shfl_i((int)in[128 + l], src);
    out[2 * 64 + l] = wv::shfl_xor(v, 1);
    out[3 * 64 + l] = wv::shfl_xor(v, 2);
    out[4 * 64 + l] = wv::shfl_xor(v, 4);
    out[5 * 64 + l] = wv::shfl_xor(v, 8);
    out[6 * 64 + l] = wv::shfl_xor(v, 16);
    out[7 * 64 + l] = wv::shfl_xor(v, 32);
}
/* ballot of (input != 0): the mask's two halves and popc64 of it */
WV_DEVICE void ballot(const double *in, double *out) {
    const int l = wv::lane();
    const unsigned long long m = wv::ballot(in[l] != 0.0);
    out[0 * 64 + l] = (double)(unsigned)(m & 0xffffffffull);
    out[1 * 64 + l] = (double)(unsigned)(m >> 32);
    out[2 * 64 + l] = (double)wv::popc64(m);
}
/* one matrix-core instruction: inputs a, b, c[0 .. 3] */
WV_DEVICE void mfma1(const double *in, double *out) {
    const int l = wv::lane();
    wv::mfma_acc acc;
    for (int v = 0; v < 4; ++v) acc.c[v] = in[(2 + v) * 64 + l];
    wv::mfma_f64_16x16x4(in[l], in[64 + l], acc);
    for (int v = 0; v < 4; ++v) out[v * 64 + l] = acc.c[v];
}
/* four dependent instructions on one accumulator: inputs a[0 .. 3], b[0 .. 3], c[0 .. 3] */
WV_DEVICE void mfma4(const double *in, double *out) {
    const int l = wv::lane();
    wv::mfma_acc acc;
    for (int v = 0; v < 4; ++v) acc.c[v] = in[(8 + v) * 64 + l];
    for (int s = 0; s < 4; ++s) wv::mfma_f64_16x16x4(in[s * 64 + l], in[(4 + s) * 64 + l], acc);
    for (int v = 0; v < 4; ++v) out[v * 64 + l] = acc.c[v];
}
WV_DEVICE void max_raw(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::max_raw(in[l], in[64 + l]);
}
/* the hardware seeds fast_rcp and the normalisations start from */
WV_DEVICE void estimates(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = wv::rcp_estimate(in[l]);
    out[64 + l] = wv::rsq_estimate(in[l]);
}
WV_DEVICE void fast_rcp(const double *in, double *out) {
    const int l = wv::lane();
    out[l] = ck::fast_rcp(in[l]);
}
WV_DEVICE void normalize4_fast(const double *in, double *out) {
    const int l = wv::lane();
    double q[4];
    for (int i = 0; i < 4; ++i) q[i] = in[i * 64 + l];
    ck::normalize4_fast(q);
    for (int i = 0; i < 4; ++i) out[i * 64 + l] = q[i];
}
/* the unit vector, then the returned norm */
WV_DEVICE void normalize3_fast(const double *in, double *out) {
    const int l = wv::lane();
    double a[3];
    for (int i = 0; i < 3; ++i) a[i] = in[i * 64 + l];
    const double n = ck::normalize3_fast(a);
    for (int i = 0; i < 3; ++i) out[i * 64 + l] = a[i];
    out[3 * 64 + l] = n;
}
/* sincos_reduced, then sincos_bounded: the kernel's choice, which takes the library's sincos for the whole wave as soon
 * as one lane is at or beyond 2^19 */
WV_DEVICE void sincos(const double *in, double *out) {
    const int l = wv::lane();
    double s, c;
    ck::sincos_reduced(in[l], s, c);
    out[0 * 64 + l] = s;
    out[1 * 64 + l] = c;
    ck::sincos_bounded(in[l], s, c);
    out[2 * 64 + l] = s;
    out[3 * 64 + l] = c;
}

}  // namespace wc

/* (host) inputs and outputs per lane of a body; -1 for a name that is not one */
extern "C" int wc_shape(const char *name, int *nin, int *nout) {
#define WC_SHAPE(n, i, o) if (!strcmp(name, #n)) { *nin = i; *nout = o; return 0; }
    WAVE_CHECK_BODIES(WC_SHAPE)
    WAVE_CHECK_AUX_BODIES(WC_SHAPE)
#undef WC_SHAPE
    return -1;
}
/* (host) the size of the auxiliary block a factor_* body reads, and where h sits in it */
extern "C" unsigned long wc_sizeof_factor_aux(void) { return sizeof(wc::FactorAux); }
extern "C" unsigned long wc_offsetof_factor_aux_h(void) { return offsetof(wc::FactorAux, h); }
/* (host) the three dof trees (which: 0 = run-time at 40 dofs, 1 = Cassie-32, 2 = the packed tray model): the padded size and the
 * words of a packed factor, the ancestor mask and elimination height of dof k (0 for the run-time tree: the model's own), and
 * the slot of entry (k, i) in Lp / LHp, -1 where the row keeps none */
extern "C" int wc_tree_size(int which, int *nvp, int *nv, int *count) {
    if (which == 0) { *nvp = 40; *nv = 0; *count = ck::LPack<ck::TopoRuntime, 40>::count; }
    else if (which == 1) { *nvp = 32; *nv = ck::TopoCassie32::nv; *count = ck::LPack<ck::TopoCassie32, 32>::count; }
    else if (which == 2) { *nvp = 40; *nv = ck::TopoCassieTray38::nv; *count = ck::LPack<ck::TopoCassieTray38, 40>::count; }
    else return -1;
    return 0;
}
extern "C" unsigned long long wc_tree_mask(int which, int k) {
    return which == 1 ? (k >= 0 && k < 32 ? ck::TopoCassie32::table[k] : 0ull) : which == 2 ? (k >= 0 && k < 40 ? ck::TopoCassieTray38::table[k] : 0ull) : 0ull;
}
extern "C" int wc_tree_slot(int which, int k, int i) {
    if (k < 0 || i < 0 || i >= k) return -1;
    if (which == 0) return k < 40 ? ck::LPack<ck::TopoRuntime, 40>::idx(k, i) : -1;
    if (which == 1) return k < 32 ? ck::LPack<ck::TopoCassie32, 32>::idx(k, i) : -1;
    if (which == 2) return k < 40 && ck::LPack<ck::TopoCassieTray38, 40>::has(k, i) ? ck::LPack<ck::TopoCassieTray38, 40>::idx(k, i) : -1;
    return -1;
}
#endif
