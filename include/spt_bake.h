/* spt_bake (include/spt_abi.h, "irradiance at surface points"): the specification as code.
 * Everything is written SPT_HD: plain C++ on the host (spt_host_bake_rays of libspt_host.so, the host checks of spt_bake), device code
 * under hipcc (k_bake_intake*), the same f32 operations on both.  All arithmetic is IEEE f32, one rounded operation at a time, in the
 * written order; the build disables contraction everywhere.
 *
 * The tables are read through the ABI's own records, which the device keeps in the same layout: spt_instance (48 words), spt_mesh,
 * spt_tri_pos, spt_tri_attr, spt_light.
 *   SURFACE  u = (1.0f - v) - w; object position (p0*u + p1*v) + p2*w, to the world by fwd as xf_point does: ((c0*x + c1*y) + c2*z) + t
 *            normal as reconstruct_hit's: n = normalize((n0*u + n1*v) + n2*w), world normalize((nrm0*n.x + nrm1*n.y) + nrm2*n.z)
 *   WORLD    p, n as given
 *   FLIP     n = -n after it is resolved
 *   frame    sphere_frame(n), sphere.rs:70-82
 *   sample   rx, ry: the first two draws of spt_rng_seed(seed ^ SPT_BAKE_SEED_SALT, a, b); phi = rx * 2.0f * SPT_PI; st = spt_sqrt(ry),
 *            ct = spt_sqrt(1.0f - ry); local (st*cp, st*sp, ct); d = normalize((tangent*lx + bitangent*ly) + n*lz), true divisions;
 *            t_min = SPT_BAKE_T_EPS / spt_max(ct, 0.00001f)
 *   delta    dir, strength, dist: the directional / point / spot cases of light_sample at p; c = dot(n, dir) > 0;
 *            li = (strength * SPT_FRAC_1_PI) * c, not all zero; shadow ray (p, dir, SPT_BAKE_T_EPS / spt_max(c, 0.00001f), dist - 0.001f)
 * normalize(v) = v / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z); dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z. */
#ifndef SPT_BAKE_H
#define SPT_BAKE_H
#include "spt_abi.h"
#include "spt_detmath.h"
#include "spt_camera_models.h" /* SPT_CM_HD, spt_cm_normalize */

#define SPT_BAKE_T_EPS 0.0001f
#define SPT_BAKE_NAN_BITS 0x7fc00000u /* the result of a point that fails the predicate */

/* `inst_type_id`: the words (prim_type, prim_id) of instance 0; `inst_stride`: words from one instance's pair to the next (48 for an
 * array of spt_instance).  Nothing is read before the index that reads it is known to be in range. */
SPT_CM_HD bool spt_bake_point_ok(const spt_bake_point* pt, uint32_t n_instances, const uint32_t* inst_type_id, uint32_t inst_stride, uint32_t n_meshes,
                                 const spt_mesh* meshes) {
    if (!(pt->instance < n_instances)) return false;
    if (!spt_is_finite(pt->v) || !spt_is_finite(pt->w)) return false;
    const uint32_t* const in = inst_type_id + (size_t)pt->instance * inst_stride;
    if (in[0] != SPT_PRIM_MESH) return false;
    const uint32_t mesh = in[1];
    if (!(mesh < n_meshes)) return false;
    const uint32_t first = meshes[mesh].tri_first, count = meshes[mesh].tri_count;
    return pt->prim >= first && pt->prim - first < count;
}
SPT_CM_HD bool spt_bake_world_ok(const spt_bake_world_point* pt) {
    const bool finite = spt_is_finite(pt->p[0]) && spt_is_finite(pt->p[1]) && spt_is_finite(pt->p[2]) && spt_is_finite(pt->n[0]) && spt_is_finite(pt->n[1]) &&
                        spt_is_finite(pt->n[2]);
    return finite && !(pt->n[0] == 0.0f && pt->n[1] == 0.0f && pt->n[2] == 0.0f);
}

/* A SURFACE point that passed spt_bake_point_ok: world position and normal */
SPT_CM_HD void spt_bake_resolve(const spt_bake_point* pt, const spt_instance* in, const spt_tri_pos* tp, const spt_tri_attr* ta, float* p, float* n) {
    const float v = pt->v, w = pt->w;
    const float u = (1.0f - v) - w;
    const float ox = (tp->p0[0] * u + tp->p1[0] * v) + tp->p2[0] * w;
    const float oy = (tp->p0[1] * u + tp->p1[1] * v) + tp->p2[1] * w;
    const float oz = (tp->p0[2] * u + tp->p1[2] * v) + tp->p2[2] * w;
    const float* const f = in->fwd;
    p[0] = ((f[0] * ox + f[3] * oy) + f[6] * oz) + f[9];
    p[1] = ((f[1] * ox + f[4] * oy) + f[7] * oz) + f[10];
    p[2] = ((f[2] * ox + f[5] * oy) + f[8] * oz) + f[11];
    float on[3];
    spt_cm_normalize((ta->n[0][0] * u + ta->n[1][0] * v) + ta->n[2][0] * w, (ta->n[0][1] * u + ta->n[1][1] * v) + ta->n[2][1] * w,
                     (ta->n[0][2] * u + ta->n[1][2] * v) + ta->n[2][2] * w, on);
    const float* const m = in->nrm;
    spt_cm_normalize((m[0] * on[0] + m[3] * on[1]) + m[6] * on[2], (m[1] * on[0] + m[4] * on[1]) + m[7] * on[2], (m[2] * on[0] + m[5] * on[1]) + m[8] * on[2], n);
}

/* sphere_frame (sphere.rs:70-82) */
SPT_CM_HD void spt_bake_frame(const float* n, float* tg, float* bt) {
    const float sin_theta = spt_sqrt(1.0f - n[1] * n[1]);
    if (sin_theta != 0.0f) {
        const float s = -n[1] / sin_theta;
        bt[0] = n[0] * s; bt[1] = sin_theta; bt[2] = n[2] * s;
        tg[0] = bt[1] * n[2] - bt[2] * n[1];
        tg[1] = bt[2] * n[0] - bt[0] * n[2];
        tg[2] = bt[0] * n[1] - bt[1] * n[0];
    } else if (n[1] > 0.0f) {
        bt[0] = 1.0f; bt[1] = 0.0f; bt[2] = 0.0f;
        tg[0] = 0.0f; tg[1] = 0.0f; tg[2] = 1.0f;
    } else {
        bt[0] = -1.0f; bt[1] = 0.0f; bt[2] = 0.0f;
        tg[0] = 0.0f; tg[1] = 0.0f; tg[2] = -1.0f;
    }
}

/* The gather direction and t_min of sample b of point a */
SPT_CM_HD void spt_bake_sample(uint64_t seed, uint32_t a, uint32_t b, const float* n, const float* tg, const float* bt, float* d, float* t_min) {
    spt_rng r = spt_rng_seed(seed ^ SPT_BAKE_SEED_SALT, a, b);
    const float rx = spt_rng_f32(&r);
    const float ry = spt_rng_f32(&r);
    const float phi = rx * 2.0f * SPT_PI;
    float sp, cp;
    spt_sincos(phi, &sp, &cp);
    const float st = spt_sqrt(ry);
    const float ct = spt_sqrt(1.0f - ry);
    const float lx = st * cp, ly = st * sp, lz = ct;
    spt_cm_normalize((tg[0] * lx + bt[0] * ly) + n[0] * lz, (tg[1] * lx + bt[1] * ly) + n[1] * lz, (tg[2] * lx + bt[2] * ly) + n[2] * lz, d);
    *t_min = SPT_BAKE_T_EPS / spt_max(ct, 0.00001f);
}

/* The contribution of light `l` at (p, n) if its shadow ray (p, dir, *t_min, *t_max) finds nothing; false: the light adds nothing */
SPT_CM_HD bool spt_bake_delta(const spt_light* l, const float* p, const float* n, float* dir, float* li, float* t_min, float* t_max) {
    float s0, s1, s2, dist;
    if (l->type == SPT_LIGHT_DIRECTIONAL) {
        dir[0] = -l->dir[0]; dir[1] = -l->dir[1]; dir[2] = -l->dir[2];
        s0 = l->strength[0]; s1 = l->strength[1]; s2 = l->strength[2];
        dist = SPT_F32_MAX;
    } else if (l->type == SPT_LIGHT_POINT || l->type == SPT_LIGHT_SPOT) {
        const float sx = l->pos[0] - p[0], sy = l->pos[1] - p[1], sz = l->pos[2] - p[2];
        const float dist_sqr = (sx * sx + sy * sy) + sz * sz;
        dist = spt_sqrt(dist_sqr);
        dir[0] = sx / dist; dir[1] = sy / dist; dir[2] = sz / dist;
        s0 = l->strength[0]; s1 = l->strength[1]; s2 = l->strength[2];
        if (l->type == SPT_LIGHT_SPOT) {
            const float cs = (l->dir[0] * -dir[0] + l->dir[1] * -dir[1]) + l->dir[2] * -dir[2];
            const float atten = spt_clamp((cs - l->cos_outer) / spt_max(l->cos_inner - l->cos_outer, 0.0001f), 0.0f, 1.0f);
            s0 = s0 * atten; s1 = s1 * atten; s2 = s2 * atten;
        }
        const float inv = 1.0f / dist_sqr;
        s0 = s0 * inv; s1 = s1 * inv; s2 = s2 * inv;
    } else {
        return false;
    }
    const float c = (n[0] * dir[0] + n[1] * dir[1]) + n[2] * dir[2];
    if (!(c > 0.0f)) return false;
    li[0] = (s0 * SPT_FRAC_1_PI) * c; li[1] = (s1 * SPT_FRAC_1_PI) * c; li[2] = (s2 * SPT_FRAC_1_PI) * c;
    if (li[0] == 0.0f && li[1] == 0.0f && li[2] == 0.0f) return false;
    *t_min = SPT_BAKE_T_EPS / spt_max(c, 0.00001f);
    *t_max = dist - 0.001f;
    return true;
}
#endif /* SPT_BAKE_H */
