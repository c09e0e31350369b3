/*
 * spt_block_cand.h — which triangles can any camera ray of one wave of k_primary hit?
 *
 * A BLOCK is the set of pixels one wave of k_primary owns: 16 columns x the 4 local rows (threadIdx.x / 16) of a 16 x 16
 * tile of the shard.  The rays of a block all start at the eye, so the set of triangles they can reach depends on the
 * camera, the image geometry and the scene, not on the sample.  k_block_candidates (kernels.h) evaluates the test below
 * once per render and block, k_primary<..., BlockCand> then runs tri_test_eye over the survivors without walking the tree.
 * The host library exposes the same code (spt_host_block_candidates) so the CPU suite can check it against brute force.
 *
 * The test is CONSERVATIVE: a triangle is dropped only when NO sample ray of the block can pass tri_test_eye (eye.h).
 * Everything is written SPT_HD: plain C++ on the host, device code under hipcc, the same f32 operations on both.
 *
 * ---- geometry ---------------------------------------------------------------------------------------------------------
 * k_primary forms x = (((float)i + ox) * width_inv - 0.5f) * aspect and y = ((float)(height - j - 1) + oy) * height_inv
 * - 0.5f with ox, oy in [0, 1), then du = (fwd * half_cot + right * x) + up * y, d = normalize(du), od = xf_vector(inv, d).
 * Every step of x and y is a monotone f32 operation, so the x of ANY sample of columns [i0, i1] lies between the same
 * formula at (i0, ox = 0) and (i1, ox = 1), likewise y for rows [j0, j1]: the block's rectangle contains the computed
 * (x, y), not only the exact ones.  The rectangle is then padded by a quarter pixel (kPad; far more than needed, and free
 * in tightness on a 16 x 4 block).  Its 4 corner directions, through xf_vector (linear), span the block's cone c_k in the
 * instance's object space; every exact M du(x, y) is a non-negative combination of the c_k.  Local rows whose image rows
 * are not consecutive (strip_rows not a multiple of 4) are split into runs and the runs' masks are OR-ed: the union.
 *
 * ---- what tri_test_eye accepts -------------------------------------------------------------------------------------------
 * With A, B, C the eye-relative vertices (A = -s, B = A + e1, C = A + e2), N = e1 x e2 and D = d . N the kernel computes
 *   v = d . (C x A) / D,  w = d . (A x B) / D,  u = 1 - v - w  ( = d . (B x C) / D exactly )
 * and accepts on COMPUTED v, w, u >= 0.  Write g_u, g_v, g_w for the three numerators, n_u = B x C, n_v = C x A, n_w = A x B for
 * their normals, l1 = |e1|, l2 = |e2|, E = l1 l2, a = |A|, eps = 2^-24 (unit roundoff), and L(d) = |M|_F |du|, which bounds
 * |M du| (the normalisation only scales a direction; everything below is homogeneous in it).
 *   - od: du is off by <= 3 eps |du| per component (orthonormal camera), the division adds eps, xf_vector 3 eps |M|_F |d|: the
 *     computed od is within 9.2 eps L of the exact M du.
 *   - a cross product is off by <= 2 eps |a| |b| per component, a 3-term dot by 3 eps |a| |b| more: det and the numerators of v
 *     and w are within 6.5 eps L (E | a l2 | a l1) of their values at od, plus 9.2 eps L (|N| | |n_v| | |n_w|) for od itself.
 *   - the sign of D is therefore certain once |D| > 16 eps E L; the test asks for 4 kTol E L and otherwise KEEPS the triangle (a
 *     block that sees the triangle's plane edge-on proves nothing).  Then 1 / det is off by delta <= 16 eps E L / |D| < 1 / 32.
 *   - u: an accepted ray has computed v, w >= 0 and 1 - v - w >= 0, so |v| + |w| <= 1 + 2 eps, and
 *     |u_c - u| |D| <= (errors of the two numerators) + (|v| + |w|) (delta + 2 eps) |D| + eps (1 + |v| + |u|) |D|
 *                   <= eps L (9.2 (|n_v| + |n_w|) + 6.5 a (l1 + l2) + 16.2 E + 3 E).
 * So a ray can only be accepted if sigma g_i >= -eta_i for i = u, v, w, sigma = sign(D), with eta_i <= 20 eps L T_i,
 *   T_v = |n_v| + a l2,   T_w = |n_w| + a l1,   T_u = |n_v| + |n_w| + a (l1 + l2) + 2 E.
 * The test's own f32 cross and dot products (on A, B, C formed from s, e1, e2) add about 11 eps L |n_i|.  It uses kTol = 2^-17 =
 * 128 eps in place of those ~31 eps: a factor 4 of head-room.
 *
 * ---- the two kinds of separating plane -------------------------------------------------------------------------------------
 * (a) eye-edge planes.  g_i is linear in d, so if sigma g_i(c_k) < -kTol L_k T_i at all 4 corners, every direction of the
 *     cone has sigma g_i < -kTol L T_i < -eta_i: the kernel computes a negative barycentric for every ray of the block.
 *     A degenerate plane (edge pointing at the eye, |n_i| ~ 0) can never beat the tolerance, so the triangle is kept.
 * (b) frustum side planes, inward normal m.  An accepted ray has exact barycentrics b_i = g_i / D >= -beta_i, beta_i =
 *     kTol T_i / Dmin with Dmin = min_k |D(c_k)| / L_k, and d = P / t with P = b_u A + b_v B + b_w C, t = det(A, B, C) / D.
 *     When all vertices are in front of the eye plane (V . h > 0, h the plane's normal in object space) by more than beta = sum
 *     beta_i times their spread, P . h > 0, and d . h > 0 for the whole cone, so t > 0 and P is a positive multiple of d:
 *     m . P >= 0.  But P is within 2 beta (l1 + l2) of a point of the triangle (move the negative weights to zero: the weights
 *     still sum to 1, so only differences of vertices enter), hence m . P <= max_V (m . V) + 2 beta |m| (l1 + l2): a plane with
 *     m . V < -|m| (2 beta (l1 + l2) + kTol R), R = max(|A|, |B|, |C|), for all three vertices rules every ray out.  beta grows as
 *     the block sees the triangle's plane at a shallower angle: a few pixels at 1024 x 1024 for the faces of a cube seen at 1 : 7.
 * (c) is no separating plane but covers the blocks that see a triangle's plane edge-on, where D has no certain sign (the horizon
 *     row of a box seen from its mid-height): see the code.
 * A triangle with a vertex at or behind the eye plane is always kept.  Any non-finite intermediate fails the comparisons
 * that drop, so it keeps too.
 */
#ifndef SPT_BLOCK_CAND_H
#define SPT_BLOCK_CAND_H

#include "spt_detmath.h"

#define SPT_BC_COLS 16u          /* pixels per block row   (k_primary: threadIdx.x % 16) */
#define SPT_BC_ROWS 4u           /* local rows per block   (one wave = 64 lanes)         */
#define SPT_BC_MAX_TRIS 64u      /* one uint64_t mask                                    */
#define SPT_BC_PAD 0.25f         /* rectangle padding in pixels                          */
#define SPT_BC_TOL 7.62939453125e-6f   /* kTol = 2^-17, see above                        */

typedef struct spt_bc_view {     /* the camera and image terms of k_primary, as it forms them */
    float fwd_hc[3];             /* forward * half_cot (f32 product)                          */
    float right[3], up[3], fwd[3];
    float width_inv, height_inv, aspect;
    uint32_t width, height;
} spt_bc_view;

typedef struct spt_bc_layout {   /* RenderCtx: which image rows the shard's local rows are   */
    uint32_t shard_index, shard_count, strip_rows, row_base, rows;
} spt_bc_layout;

typedef struct spt_bc_cone {     /* one run of a block seen from one instance's object space */
    float c[4][3];               /* corner directions, counter-clockwise or clockwise         */
    float L[4];                  /* |M|_F |du_k|                                              */
    float m[4][3];               /* inward normals of the side planes c_k, c_(k+1)            */
    float mlen[4];
    float h[3];                  /* normal of the eye plane in object space                   */
    uint32_t side_ok;            /* the side planes are usable (non-degenerate, cone in front) */
} spt_bc_cone;

SPT_HD float spt_bc_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
SPT_HD void spt_bc_cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
SPT_HD float spt_bc_len(const float* a) { return spt_sqrt(spt_bc_dot(a, a)); }

/* global_row of kernels.h */
SPT_HD uint32_t spt_bc_global_row(const spt_bc_layout* l, uint32_t row_local) {
    const uint32_t strip = row_local / l->strip_rows;
    return l->row_base + (strip * l->shard_count + l->shard_index) * l->strip_rows + (row_local - strip * l->strip_rows);
}

/* Blocks of a shard: block = tile * 4 + wave, tile = tx + tiles_x * ty (k_primary's numbering).  Returns the block's
 * columns [*i0, *i1] and its first local row; false when the block owns no pixel. */
SPT_HD bool spt_bc_block_pixels(const spt_bc_view* v, const spt_bc_layout* l, uint32_t block, uint32_t* i0, uint32_t* i1, uint32_t* row0) {
    const uint32_t tiles_x = (v->width + SPT_BC_COLS - 1u) / SPT_BC_COLS;
    const uint32_t tile = block / 4u, wave = block % 4u;
    const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
    *i0 = tx * SPT_BC_COLS;
    *i1 = (*i0 + SPT_BC_COLS <= v->width ? *i0 + SPT_BC_COLS : v->width) - 1u;
    *row0 = ty * 16u + wave * SPT_BC_ROWS;
    return *i0 < v->width && *row0 < l->rows;
}

/* The next run of consecutive image rows among the block's local rows [*row, row_end): returns false when none is left,
 * else the run's image rows [*j0, *j1] and advances *row behind it. */
SPT_HD bool spt_bc_next_run(const spt_bc_layout* l, uint32_t* row, uint32_t row_end, uint32_t* j0, uint32_t* j1) {
    if (*row >= row_end) return false;
    *j0 = *j1 = spt_bc_global_row(l, *row);
    ++*row;
    while (*row < row_end && spt_bc_global_row(l, *row) == *j1 + 1u) { ++*j1; ++*row; }
    return true;
}

/* The cone of pixels [i0, i1] x image rows [j0, j1] in the object space of the instance with matrices inv / fwd
 * (spt_instance: 3 columns + translation each). */
SPT_HD void spt_bc_cone_make(const spt_bc_view* v, uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1, const float* inv, const float* fwd,
                             spt_bc_cone* cone) {
    const float pad_x = (SPT_BC_PAD * v->width_inv) * v->aspect, pad_y = SPT_BC_PAD * v->height_inv;
    const float xs[2] = {(((float)i0 + 0.0f) * v->width_inv - 0.5f) * v->aspect - pad_x, (((float)i1 + 1.0f) * v->width_inv - 0.5f) * v->aspect + pad_x};
    const float ys[2] = {((float)(v->height - j1 - 1u) + 0.0f) * v->height_inv - 0.5f - pad_y, ((float)(v->height - j0 - 1u) + 1.0f) * v->height_inv - 0.5f + pad_y};
    float mf = 0.0f;
    for (int k = 0; k < 9; ++k) mf = mf + inv[k] * inv[k];
    mf = spt_sqrt(mf);
    for (int k = 0; k < 4; ++k) {   /* (x0,y0) (x1,y0) (x1,y1) (x0,y1): around the rectangle */
        const float x = xs[(k == 1 || k == 2) ? 1 : 0], y = ys[k >= 2 ? 1 : 0];
        float du[3];
        for (int a = 0; a < 3; ++a) du[a] = (v->fwd_hc[a] + v->right[a] * x) + v->up[a] * y;
        for (int a = 0; a < 3; ++a) cone->c[k][a] = (inv[a] * du[0] + inv[3 + a] * du[1]) + inv[6 + a] * du[2];
        cone->L[k] = mf * spt_bc_len(du);
    }
    for (int a = 0; a < 3; ++a) cone->h[a] = spt_bc_dot(fwd + 3 * a, v->fwd);   /* transpose(F) forward */
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
        spt_bc_cross(cone->c[k], cone->c[(k + 1) & 3], cone->m[k]);
        cone->mlen[k] = spt_bc_len(cone->m[k]);
        /* inward: the opposite corners are on the positive side, clearly */
        float o1 = spt_bc_dot(cone->m[k], cone->c[(k + 2) & 3]), o2 = spt_bc_dot(cone->m[k], cone->c[(k + 3) & 3]);
        if (o1 < 0.0f && o2 < 0.0f) {
            for (int a = 0; a < 3; ++a) cone->m[k][a] = -cone->m[k][a];
            o1 = -o1; o2 = -o2;
        }
        const float lim = SPT_BC_TOL * cone->mlen[k];
        ok = ok && (o1 > lim * cone->L[(k + 2) & 3]) && (o2 > lim * cone->L[(k + 3) & 3]);
        ok = ok && (spt_bc_dot(cone->c[k], cone->h) > 0.0f);
    }
    cone->side_ok = ok ? 1u : 0u;
}

/* May a ray of the cone pass tri_test_eye on the triangle (s, e1, e2) of the eye-relative blob?  false = certainly not. */
SPT_HD bool spt_bc_keep(const spt_bc_cone* cone, const float* s, const float* e1, const float* e2) {
    float V[3][3];   /* A, B, C */
    for (int a = 0; a < 3; ++a) { V[0][a] = -s[a]; V[1][a] = e1[a] - s[a]; V[2][a] = e2[a] - s[a]; }
    /* a vertex at or behind the eye plane: keep */
    const float f0 = spt_bc_dot(V[0], cone->h), f1 = spt_bc_dot(V[1], cone->h), f2 = spt_bc_dot(V[2], cone->h);
    if (!(f0 > 0.0f && f1 > 0.0f && f2 > 0.0f)) return true;
    const float R = spt_sqrt(spt_max(spt_bc_dot(V[0], V[0]), spt_max(spt_bc_dot(V[1], V[1]), spt_bc_dot(V[2], V[2]))));
    const float la = spt_bc_len(V[0]), l1 = spt_bc_len(e1), l2 = spt_bc_len(e2), E = l1 * l2;
    /* n_u = B x C, n_v = C x A, n_w = A x B and the tolerances of their numerators */
    float n[3][3], nl[3];
    for (int i = 0; i < 3; ++i) {
        spt_bc_cross(V[(i + 1) % 3], V[(i + 2) % 3], n[i]);
        nl[i] = spt_bc_len(n[i]);
    }
    const float T[3] = {((nl[1] + nl[2]) + la * (l1 + l2)) + (E + E), nl[1] + la * l2, nl[2] + la * l1};
    /* the sign of D = d . N must be certain over the whole cone */
    float N[3];
    spt_bc_cross(e1, e2, N);
    float dmin = 0.0f, dmax = 0.0f;
    int pos = 0, neg = 0;
    for (int k = 0; k < 4; ++k) {
        const float D = spt_bc_dot(cone->c[k], N), lim = ((4.0f * SPT_BC_TOL) * E) * cone->L[k];
        if (D > lim) ++pos;
        if (D < -lim) ++neg;
        const float q = spt_abs(D) / cone->L[k];
        dmin = (k == 0) ? q : spt_min(dmin, q);
        dmax = (k == 0) ? q : spt_max(dmax, q);
    }
    if (pos != 4 && neg != 4) {
        /* (c) the block sees the triangle's plane edge-on.  An accepted ray still has computed v, w in [0, 1]: its numerators are no
         * larger than its determinant.  Both are linear in d, so if |g_i| / L at every corner (one sign) exceeds the largest |D| / L
         * by the two tolerances, |v| or |w| is above 1 for every ray of the cone. */
        for (int i = 1; i < 3; ++i) {
            float gmin = 0.0f;
            int p = 0, m = 0;
            for (int k = 0; k < 4; ++k) {
                const float g = spt_bc_dot(n[i], cone->c[k]);
                if (g > 0.0f) ++p;
                if (g < 0.0f) ++m;
                const float q = spt_abs(g) / cone->L[k];
                gmin = (k == 0) ? q : spt_min(gmin, q);
            }
            if ((p == 4 || m == 4) && gmin > 1.0625f * dmax + SPT_BC_TOL * (T[i] + E)) return false;
        }
        return true;
    }
    const float sigma = pos == 4 ? 1.0f : -1.0f;
    /* (a) the three planes through the eye and an edge */
    for (int i = 0; i < 3; ++i) {
        const float tol = SPT_BC_TOL * T[i];
        bool out = true;
        for (int k = 0; k < 4; ++k) out = out && (sigma * spt_bc_dot(n[i], cone->c[k]) < -(tol * cone->L[k]));
        if (out) return false;
    }
    /* (b) the four side planes of the cone */
    if (cone->side_ok) {
        const float beta = SPT_BC_TOL * ((T[0] + T[1]) + T[2]) / dmin;
        const float fmin = spt_min(f0, spt_min(f1, f2)), fmax = spt_max(f0, spt_max(f1, f2));
        if (fmin > beta * fmax) {
            for (int k = 0; k < 4; ++k) {
                const float lim = -cone->mlen[k] * ((beta + beta) * (l1 + l2) + SPT_BC_TOL * R);
                if (spt_bc_dot(cone->m[k], V[0]) < lim && spt_bc_dot(cone->m[k], V[1]) < lim && spt_bc_dot(cone->m[k], V[2]) < lim) return false;
            }
        }
    }
    return true;
}

#endif /* SPT_BLOCK_CAND_H */
