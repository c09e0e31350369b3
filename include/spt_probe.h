/* spt_probe (include/spt_abi.h, "spherical-harmonic light probes"): the specification as code.
 * Everything is written SPT_CM_HD: plain C++ on the host (spt_host_probe_rays and spt_host_probe_basis of libspt_host.so, the host
 * checks of spt_probe), device code under hipcc (k_probe_intake*, k_probe_finish), the same f32 operations on both.  All arithmetic is
 * IEEE f32, one rounded operation at a time, in the written order; the build disables contraction everywhere.
 *
 *   probe    valid iff p is finite
 *   sample   rx, ry: the first two draws of spt_rng_seed(seed ^ SPT_PROBE_SEED_SALT, a, b); z = 1.0f - 2.0f*rx;
 *            r = spt_sqrt(spt_max(0.0f, 1.0f - z*z)); phi = ry * 2.0f * SPT_PI; d = normalize(r*cp, r*sp, z), true divisions;
 *            t_min = SPT_BAKE_T_EPS
 *   basis    real orthonormal SH, bands 0 .. 2, no Condon-Shortley sign, j = l(l+1)+m, world axes
 *   delta    dir, strength, dist: the directional / point / spot cases of spt_bake_delta without the cosine and SPT_FRAC_1_PI;
 *            li = strength, not all zero; shadow ray (p, dir, SPT_BAKE_T_EPS, dist - 0.001f)
 *   result   sh[j][c] = D[j][c] + (((0 + x_c(0)*Y_j(d_0)) + x_c(1)*Y_j(d_1)) + ...) * w,  w = (4.0f*SPT_PI) * (1.0f/(float)S) */
#ifndef SPT_PROBE_H
#define SPT_PROBE_H
#include "spt_abi.h"
#include "spt_detmath.h"
#include "spt_camera_models.h" /* SPT_CM_HD, spt_cm_normalize */
#include "spt_bake.h"          /* SPT_BAKE_T_EPS, SPT_BAKE_NAN_BITS, spt_bake_resolve */

#define SPT_PROBE_COEFFS 9u
#define SPT_PROBE_SH_WORDS 27u   /* [9][3] */
#define SPT_PROBE_AUX_WORDS 4u

SPT_CM_HD bool spt_probe_ok(const spt_probe_point* pt) { return spt_is_finite(pt->p[0]) && spt_is_finite(pt->p[1]) && spt_is_finite(pt->p[2]); }

/* w of the result, made once on the host */
inline float spt_probe_weight(uint32_t samples) { return (4.0f * SPT_PI) * (1.0f / (float)samples); }

/* The uniform sphere map of the draws (rx, ry) */
SPT_CM_HD void spt_probe_map(float rx, float ry, float* d) {
    const float z = 1.0f - 2.0f * rx;
    const float r = spt_sqrt(spt_max(0.0f, 1.0f - z * z));
    const float phi = ry * 2.0f * SPT_PI;
    float sp, cp;
    spt_sincos(phi, &sp, &cp);
    spt_cm_normalize(r * cp, r * sp, z, d);
}

/* The gather direction of sample b of probe a */
SPT_CM_HD void spt_probe_sample(uint64_t seed, uint32_t a, uint32_t b, float* d) {
    spt_rng r = spt_rng_seed(seed ^ SPT_PROBE_SEED_SALT, a, b);
    const float rx = spt_rng_f32(&r);
    const float ry = spt_rng_f32(&r);
    spt_probe_map(rx, ry, d);
}

/* Y_j(d), j in [0, 9) */
SPT_CM_HD float spt_probe_basis_j(const float* d, uint32_t j) {
    const float x = d[0], y = d[1], z = d[2];
    switch (j) {
        case 0: return 0.282094792f;
        case 1: return 0.488602512f * y;
        case 2: return 0.488602512f * z;
        case 3: return 0.488602512f * x;
        case 4: return 1.092548431f * (x * y);
        case 5: return 1.092548431f * (y * z);
        case 6: return 0.315391565f * (3.0f * (z * z) - 1.0f);
        case 7: return 1.092548431f * (x * z);
        default: return 0.546274215f * (x * x - y * y);
    }
}
SPT_CM_HD void spt_probe_basis(const float* d, float* Y) {
    for (uint32_t j = 0; j < SPT_PROBE_COEFFS; ++j) Y[j] = spt_probe_basis_j(d, j);
}

/* The radiance of delta light `l` at p if its shadow ray (p, dir, SPT_BAKE_T_EPS, *t_max) finds nothing; false: the light adds nothing.
 * dir, strength and dist as in spt_bake_delta, without the cosine and without SPT_FRAC_1_PI */
SPT_CM_HD bool spt_probe_delta(const spt_light* l, const float* p, float* dir, float* li, float* t_max) {
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
    li[0] = s0; li[1] = s1; li[2] = s2;
    if (li[0] == 0.0f && li[1] == 0.0f && li[2] == 0.0f) return false;
    *t_max = dist - 0.001f;
    return true;
}

/* Whether a first-segment hit (instance record `in`, its triangle records) faces away from the probe: mesh instances only */
SPT_CM_HD bool spt_probe_backfacing(const spt_instance* in, uint32_t instance, uint32_t prim, float v, float w, const spt_tri_pos* tp, const spt_tri_attr* ta,
                                    const float* d) {
    if (in->prim_type != SPT_PRIM_MESH) return false;
    spt_bake_point pt;
    pt.instance = instance; pt.prim = prim; pt.v = v; pt.w = w;
    float p[3], n[3];
    spt_bake_resolve(&pt, in, tp, ta, p, n);
    return (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2] > 0.0f;
}
#endif /* SPT_PROBE_H */
