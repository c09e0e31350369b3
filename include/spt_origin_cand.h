/*
 * spt_origin_cand.h - which triangles can a shadow or an extension ray hit that leaves triangle T on one side?
 *
 * The fused simple shade kernels (k_shade<0, ., kFused, ..., OriginCand>, kernels.h) start both rays of a path vertex at
 * it.position, a point of the triangle T the vertex lies on.  A ray that leaves a flat triangle on one side of its plane can
 * only hit triangles that reach into that side's half-space: on a convex body, none.  The table made here holds, per triangle
 * and side, the 64-bit set of triangle slots (bit k = slot k of the staged blob) such a ray may hit; the kernel ORs the words
 * of a wave's lanes and tests exactly that set (origin_cand_closest / origin_cand_any), without the tree walk.  The sets
 * depend on the geometry and the transforms only - not on camera, sample or light - so the table is made on the host, in
 * double precision, once per scene state (creation, spt_scene_update, spt_scene_deform).  Host-only C++; the library and
 * the CPU suite (spt_host_origin_candidates) share it.
 *
 * ---- the four words of a triangle T --------------------------------------------------------------------------------
 * "up" is the side the shading normal m of T points to (m = the instance's normal matrix applied to the vertex normals), n the
 * unit geometric normal of T's WORLD plane (fwd applied to the object-space vertices; non-uniform scale keeps planes planar)
 * oriented like m, ht(x) = n . (x - p0) the height of x over that plane.
 *   word[T][0] = loose[up], word[T][1] = loose[down], word[T][2] = tight[up], word[T][3] = tight[down]
 *   loose[side]: bit U is cleared only when every vertex of U is beyond the plane on the OTHER side by more than delta.  Valid
 *     for any ray that starts within delta of the plane and truly points to `side` (d . n_side >= 0).  It keeps T, coplanar
 *     triangles and whatever touches the plane.
 *   tight[side]: valid for rays that the kernel accepts only at t > t_min = kTMinEps / max(|wi.z|, 1e-5) with |wi.z| >= z0
 *     (below).  Bit U is cleared when every vertex of U has ht_side < kTMinEps (1 - eps_z) - delta.  That clears T itself,
 *     coplanar and edge-adjacent triangles of a convex body.
 * T is FLAT when its three transformed, normalised vertex normals lie within kFlatTol / 2 of +n or all of -n.  Then it.normal
 * (shading.h: the interpolated normal, transformed and normalised in f32, rounding ~ 1e-6) is within kFlatTol of m = +-n
 * everywhere on T, and the shading frame's zw = +- it.normal.  A triangle that is not flat, or is degenerate (sigma > 1e4, below),
 * gets all slots in all four words: the kernel's side test says nothing about its geometric plane.
 *
 * ---- the kernel's choice (kernels.h) -------------------------------------------------------------------------------
 * Per lane and ray, with wi the ray direction in the shading frame (wi.z = dot(zw, d), f32) and zw = -it.normal when the
 * surface is double sided and hit from behind, else +it.normal:
 *   |wi.z| >= z0:  word = tight[(wi.z < 0) != (zw == -it.normal) ? down : up]
 *   else:          word = loose[up] | loose[down]   (no triangle is beyond the plane on both sides: every slot; rare)
 * z0 = 1e-3.  d . zw differs from wi.z by the frame's departure from orthonormality and the dot product's rounding, < 8 eps
 * |wi| ~ 5e-7 (eps = 2^-24), and zw from +-n by kFlatTol = 1e-5: d . n_side >= |wi.z| (1 - eps_z) with eps_z = (1e-5 + 5e-7) /
 * z0 < 1 / 64, in particular its sign is that of wi.z.  So a hit the kernel accepts (t > t_min, t_min rounded by one division:
 * covered by eps_z) lies at height ht_side > t_min d . n_side - delta >= kTMinEps (1 - eps_z) - delta over T's plane.
 *
 * ---- delta ---------------------------------------------------------------------------------------------------------
 * delta bounds (a) how far it.position is from T's exact world plane and (b) how far outside a triangle U a ray may pass that
 * tri_test_edges still accepts.  Lengths: c the centre of the scene's box, r its radius, rho the distance of the path's first
 * ray origin (the eye) from c; k2 = smax(fwd) smax(inv) of the instance (2-norms: 1 for a rigid motion), sigma = |e1| |e2| / |e1 x
 * e2| of the triangle in its object space (1 for a right angle at p0).  Per source, in world units:
 *  (a1) it.position = point_at(ray, t) = fl(o + fl(d t)): <= 1.8 eps (|t d| + |position|) <= 1.8 eps ((rho + r) + (|c| + r)).
 *  (a2) t itself.  tri_test_edges computes t = e2 . (s x e1) / e1 . (d x e2).  A cross product is off by <= 2.9 eps |a| |b|, a
 *       3-term dot by 3 eps |a| |b| more, the quotient by 2 eps: the error of t, times |d . n|, moves the point off the plane by
 *       <= eps S (13 sigma + 2) with S = max(|s|, |t d|) <= smax(inv) (rho + r) in object space, i.e. k2 (rho + r) in the world.
 *       (The shape factor is what the brute-force test weights its slivers for.)
 *  (a3) the object-space ray: s = fl(o' - p0) 1.8 eps S; o' = xf_point(inv, o) <= 4 eps smax(inv) (|c| + rho), d' = xf_vector
 *       <= 3 eps smax(inv) |d| over a length t; fwd inv = 1 only to 3 eps k2: together <= eps k2 (4.8 (rho + r) + 7 (|c| + rho)).
 *  (b)  the same terms for the test of U from an origin ON the scene (distance <= 2 r, |o| <= |c| + r), none of (a1): a ray whose
 *       computed v, w, u >= 0 passes within eps k2_U (2 r (13 sigma_U + 6.8) + 7 (|c| + r)) of U at the accepted t.
 * With A = max_T k2 (13 sigma + 13.8) + 1.8, B = max_T k2 (r (13 sigma + 6.8) + 7 |c|) + 1.8 (|c| + 2 r) + max_U (b):
 *   delta(rho) = eps (A rho + B).
 * The bounds are first-order worst cases (every rounding aligned); tests/test_origin_candidates.py restates the kernel's f32
 * operations and looks for a miss over weighted rays: it is the judge of this derivation.
 * RULES.  delta_scene = delta(2 r) - the scene's own extent - must be below kTMinEps / 4, else tight = loose (a scene near
 * coordinates 100 already fails it through |c|).  The table is valid for eyes within `reach` of c, where delta(reach) =
 * max(kTMinEps / 2, 2 delta_scene); the words are made with THAT delta, and a render whose eye lies farther out does not take
 * the path (spt_hip.hip).  Bounce >= 1 starts on the scene (rho <= r).
 */
#ifndef SPT_ORIGIN_CAND_H
#define SPT_ORIGIN_CAND_H

#include <stdint.h>
#include <cmath>
#include <vector>

#define SPT_OC_MAX_TRIS 64u              /* one uint64_t per word                                  */
#define SPT_OC_Z0 1e-3f                  /* z0: the kernel compares |wi.z| with it                  */
#define SPT_OC_TMIN_EPS 1e-4             /* kTMinEps of device_math.h (kernels.h asserts the match) */
#define SPT_OC_EPS_Z (1.0 / 64.0)        /* eps_z                                                  */
#define SPT_OC_FLAT_TOL 1e-5             /* kFlatTol                                               */
#define SPT_OC_WORDS 4u                  /* loose up, loose down, tight up, tight down             */

struct spt_oc_instance {                 /* spt_instance: 3 columns + translation, the normal matrix's 3 columns */
    float inv[12], fwd[12], nrm[9];
};
struct spt_oc_triangle {                 /* slot k of the blob */
    float p0[3], e1[3], e2[3];           /* object space: the vertex and the two stored edge differences */
    float n[3][3];                       /* the three vertex normals (object space)                      */
    uint32_t instance;                   /* the one instance that uses the slot's mesh                   */
    uint32_t id;                         /* the triangle's ABI index: the row of the table (hit records carry it) */
};
struct spt_oc_info {
    double center[3], radius;            /* c, r                                                   */
    double reach;                        /* eyes within this distance of c                         */
    double delta;                        /* delta(reach), world units                              */
    double delta_scene;                  /* delta(2 r)                                             */
    uint32_t tight;                      /* 0: tight = loose                                       */
    uint32_t n_rows;                     /* rows of the table: 1 + the largest id                  */
};

namespace spt_oc {
inline double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline void cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
inline double len(const double* a) { return std::sqrt(dot(a, a)); }
/* largest singular value of the 3 x 3 matrix whose columns are m[0..2], m[3..5], m[6..8]: Jacobi sweeps over M^T M */
inline double smax(const float* m) {
    double a[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            a[i][j] = 0.0;
            for (int k = 0; k < 3; ++k) a[i][j] += (double)m[3 * i + k] * (double)m[3 * j + k];
        }
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
        if (off <= 1e-18 * (std::fabs(a[0][0]) + std::fabs(a[1][1]) + std::fabs(a[2][2]))) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) { const double x = a[k][p], y = a[k][q]; a[k][p] = c * x - s * y; a[k][q] = s * x + c * y; }
                for (int k = 0; k < 3; ++k) { const double x = a[p][k], y = a[q][k]; a[p][k] = c * x - s * y; a[q][k] = s * x + c * y; }
            }
    }
    const double l = std::fmax(a[0][0], std::fmax(a[1][1], a[2][2]));
    return std::sqrt(l > 0.0 ? l : 0.0) * (1.0 + 1e-12);
}
}  // namespace spt_oc

/* Fills words[SPT_OC_WORDS * row + w] for the rows 0 .. info->n_rows - 1 (row = spt_oc_triangle::id; a row no triangle names
 * gets all slots) and *info.  `words` holds SPT_OC_WORDS * SPT_OC_MAX_TRIS entries.  Returns false, with nothing usable in
 * either, when the scene does not qualify: no triangle, more than 64 slots, an id of 64 or more or one named twice, a
 * non-finite or singular transform. */
inline bool spt_oc_build(const spt_oc_instance* inst, uint32_t n_inst, const spt_oc_triangle* tri, uint32_t n_tri, uint64_t* words, spt_oc_info* info) {
    using namespace spt_oc;
    if (n_tri == 0u || n_tri > SPT_OC_MAX_TRIS || n_inst == 0u) return false;
    const double eps = 1.0 / 16777216.0;   /* 2^-24 */
    const uint64_t all = n_tri == 64u ? ~0ull : (1ull << n_tri) - 1ull;
    struct World { double v[3][3], n[3], sigma, k2; bool degenerate, flat; };
    std::vector<World> w(n_tri);
    std::vector<double> k2_inst(n_inst);
    for (uint32_t i = 0; i < n_inst; ++i) {
        k2_inst[i] = smax(inst[i].fwd) * smax(inst[i].inv);
        if (!(k2_inst[i] > 0.0) || !std::isfinite(k2_inst[i])) return false;
    }
    uint64_t seen = 0ull;
    uint32_t n_rows = 0u;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t k = 0; k < n_tri; ++k) {
        const spt_oc_triangle& t = tri[k];
        if (t.instance >= n_inst || t.id >= SPT_OC_MAX_TRIS || ((seen >> t.id) & 1ull)) return false;
        seen |= 1ull << t.id;
        n_rows = t.id + 1u > n_rows ? t.id + 1u : n_rows;
        const float* F = inst[t.instance].fwd;
        const double e1[3] = {t.e1[0], t.e1[1], t.e1[2]}, e2[3] = {t.e2[0], t.e2[1], t.e2[2]};
        double N[3];
        cross(e1, e2, N);
        const double E = len(e1) * len(e2), nl = len(N);
        w[k].degenerate = !(nl > 1e-4 * E) || !(E > 0.0);
        w[k].sigma = w[k].degenerate ? 1.0 : E / nl;
        w[k].k2 = k2_inst[t.instance];
        for (int v = 0; v < 3; ++v) {
            const double p[3] = {(double)t.p0[0] + (v == 1 ? e1[0] : v == 2 ? e2[0] : 0.0), (double)t.p0[1] + (v == 1 ? e1[1] : v == 2 ? e2[1] : 0.0),
                                 (double)t.p0[2] + (v == 1 ? e1[2] : v == 2 ? e2[2] : 0.0)};
            for (int a = 0; a < 3; ++a) {
                w[k].v[v][a] = ((double)F[a] * p[0] + (double)F[3 + a] * p[1]) + (double)F[6 + a] * p[2] + (double)F[9 + a];
                if (!std::isfinite(w[k].v[v][a])) return false;
                lo[a] = std::fmin(lo[a], w[k].v[v][a]); hi[a] = std::fmax(hi[a], w[k].v[v][a]);
            }
        }
        double a[3], b[3];
        for (int c = 0; c < 3; ++c) { a[c] = w[k].v[1][c] - w[k].v[0][c]; b[c] = w[k].v[2][c] - w[k].v[0][c]; }
        cross(a, b, w[k].n);
        const double wl = len(w[k].n);
        if (!(wl > 0.0)) w[k].degenerate = true;
        for (int c = 0; c < 3; ++c) w[k].n[c] = w[k].degenerate ? 0.0 : w[k].n[c] / wl;
        /* flat: the transformed vertex normals against +-n; n is then oriented like them */
        w[k].flat = !w[k].degenerate;
        int sign = 0;
        const float* Nm = inst[t.instance].nrm;
        for (int v = 0; v < 3 && w[k].flat; ++v) {
            double o[3] = {t.n[v][0], t.n[v][1], t.n[v][2]};
            const double ol = len(o);
            if (!(ol > 0.0)) { w[k].flat = false; break; }
            for (int c = 0; c < 3; ++c) o[c] /= ol;
            double m[3];
            for (int c = 0; c < 3; ++c) m[c] = ((double)Nm[c] * o[0] + (double)Nm[3 + c] * o[1]) + (double)Nm[6 + c] * o[2];
            const double ml = len(m);
            if (!(ml > 0.0)) { w[k].flat = false; break; }
            for (int c = 0; c < 3; ++c) m[c] /= ml;
            const int sg = dot(m, w[k].n) >= 0.0 ? 1 : -1;
            if (sign == 0) sign = sg;
            double d[3] = {m[0] - sg * w[k].n[0], m[1] - sg * w[k].n[1], m[2] - sg * w[k].n[2]};
            if (sg != sign || !(len(d) <= 0.5 * SPT_OC_FLAT_TOL)) w[k].flat = false;
        }
        if (w[k].flat && sign < 0)
            for (int c = 0; c < 3; ++c) w[k].n[c] = -w[k].n[c];
    }
    double cl = 0.0, r = 0.0;
    for (int a = 0; a < 3; ++a) { info->center[a] = 0.5 * (lo[a] + hi[a]); cl += info->center[a] * info->center[a]; }
    cl = std::sqrt(cl);
    for (uint32_t k = 0; k < n_tri; ++k)
        for (int v = 0; v < 3; ++v) {
            const double d[3] = {w[k].v[v][0] - info->center[0], w[k].v[v][1] - info->center[1], w[k].v[v][2] - info->center[2]};
            r = std::fmax(r, len(d));
        }
    if (!(r > 0.0) || !std::isfinite(r) || !std::isfinite(cl)) return false;
    /* delta(rho) = eps (A rho + B) */
    double A = 0.0, BT = 0.0, BU = 0.0;
    for (uint32_t k = 0; k < n_tri; ++k) {
        if (w[k].degenerate) continue;
        const double k2 = w[k].k2, sg = w[k].sigma;
        A = std::fmax(A, k2 * (13.0 * sg + 13.8) + 1.8);
        BT = std::fmax(BT, k2 * (r * (13.0 * sg + 6.8) + 7.0 * cl) + 1.8 * (cl + 2.0 * r));
        BU = std::fmax(BU, k2 * (2.0 * r * (13.0 * sg + 6.8) + 7.0 * (cl + r)));
    }
    if (A == 0.0) return false;   /* every triangle degenerate */
    const double B = BT + BU;
    const double delta_scene = eps * (A * 2.0 * r + B);
    const bool tight = delta_scene < 0.25 * SPT_OC_TMIN_EPS;
    const double delta = std::fmax(0.5 * SPT_OC_TMIN_EPS, 2.0 * delta_scene);
    info->radius = r;
    info->delta_scene = delta_scene;
    info->delta = delta;
    info->reach = (delta / eps - B) / A;
    info->tight = tight ? 1u : 0u;
    info->n_rows = n_rows;
    const double h_tight = SPT_OC_TMIN_EPS * (1.0 - SPT_OC_EPS_Z) - delta;
    for (uint32_t i = 0; i < SPT_OC_WORDS * SPT_OC_MAX_TRIS; ++i) words[i] = all;
    for (uint32_t kt = 0; kt < n_tri; ++kt) {
        const World& T = w[kt];
        if (!T.flat) continue;
        uint64_t out[SPT_OC_WORDS] = {all, all, all, all};
        for (uint32_t ku = 0; ku < n_tri; ++ku) {
            const World& U = w[ku];
            if (U.degenerate) continue;   /* kept everywhere */
            double hmin = 1e300, hmax = -1e300;
            for (int v = 0; v < 3; ++v) {
                const double d[3] = {U.v[v][0] - T.v[0][0], U.v[v][1] - T.v[0][1], U.v[v][2] - T.v[0][2]};
                const double h = dot(T.n, d);
                hmin = std::fmin(hmin, h); hmax = std::fmax(hmax, h);
            }
            const uint64_t bit = 1ull << ku;
            if (hmax < -delta) out[0] &= ~bit;                   /* loose up: U wholly below          */
            if (hmin > delta) out[1] &= ~bit;                    /* loose down: U wholly above        */
            if (tight && hmax < h_tight) out[2] &= ~bit;         /* tight up: nothing of U above h    */
            if (tight && -hmin < h_tight) out[3] &= ~bit;        /* tight down                        */
        }
        if (!tight) { out[2] = out[0]; out[3] = out[1]; }
        for (uint32_t q = 0; q < SPT_OC_WORDS; ++q) words[SPT_OC_WORDS * tri[kt].id + q] = out[q];
    }
    return true;
}

#endif /* SPT_ORIGIN_CAND_H */
