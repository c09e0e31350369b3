/* The camera models of spt_render_camera / spt_film_create_camera (include/spt_abi.h, "camera models"): the specification as code.
 * Everything is written SPT_HD: plain C++ on the host (spt_host_camera_rays of libspt_host.so), device code under hipcc
 * (k_primary_cam), the same f32 operations on both.  All arithmetic is IEEE f32, one rounded operation at a time, in the written
 * order; the build disables contraction everywhere.
 *
 * x, y are the screen point of pt.rs:269-271; hc = base.half_cot_half_fov; t_min = SPT_CM_T_MIN for every model.
 *   PERSPECTIVE   o = eye, d = normalize((forward*hc + right*x) + up*y)
 *   THIN_LENS     lens draws u1, u2: the first two of spt_rng_seed(seed ^ SPT_CAMERA_SEED_SALT, pixel, plan_index), whatever the radius
 *                 a = 2*u1 - 1, b = 2*u2 - 1; a == 0 && b == 0: lx = ly = 0; |a| > |b|: r = a, phi = (SPT_PI/4) * (b/a);
 *                 otherwise r = b, phi = SPT_PI/2 - (SPT_PI/4) * (a/b); lx = r*spt_cos(phi), ly = r*spt_sin(phi)
 *                 ft = focus_distance / hc (once, host); du = (forward*hc + right*x) + up*y
 *                 lo_k = (right_k*lx + up_k*ly) * lens_radius; o = eye + lo; d = normalize(du*ft - lo)
 *   ORTHOGRAPHIC  sx = x*view_height, sy = y*view_height; o_k = eye_k + (right_k*sx + up_k*sy); d = forward, as given
 *   PANORAMA      ph = (x * aspect_inv) * (2*SPT_PI), aspect_inv = 1.0f/aspect (once); th = (0.5f - y) * SPT_PI; st = spt_sin(th)
 *                 o = eye; d = normalize((st*spt_sin(ph), spt_cos(th), st*spt_cos(ph)))
 * Auxiliary rays: the same model at (x + aux_dx, y) and (x, y + aux_dy) with the same lens point. */
#ifndef SPT_CAMERA_MODELS_H
#define SPT_CAMERA_MODELS_H
#include "spt_abi.h"
#include "spt_detmath.h"

#define SPT_CM_T_MIN 0.0001f
/* (forced inline on the device: the model is a kernel argument, and a call through its address would copy it to scratch) */
#if defined(__HIPCC__)
#define SPT_CM_HD __host__ __device__ __forceinline__
#else
#define SPT_CM_HD inline
#endif

/* What is made once per plan on the host, in f32 */
typedef struct spt_cm_plan {
    float ft;           /* THIN_LENS: focus_distance / hc */
    float aspect_inv;   /* PANORAMA: 1.0f / aspect, aspect = (float)width / (float)height */
} spt_cm_plan;

inline spt_cm_plan spt_cm_plan_make(const spt_camera_model* m, uint32_t width, uint32_t height) {
    spt_cm_plan p;
    p.ft = m->focus_distance / m->base.half_cot_half_fov;
    p.aspect_inv = 1.0f / ((float)width / (float)height);
    return p;
}

/* NULL: the model may be rendered; else what is wrong with it (SPT_ERR_INVALID_ARG) */
inline const char* spt_cm_check(const spt_camera_model* m) {
    if (!m) return "null camera model";
    if (m->size < sizeof(spt_camera_model)) return "camera model: size is below sizeof(spt_camera_model)";
    if (m->type > SPT_CAMERA_PANORAMA) return "camera model: unknown type";
    if (m->type == SPT_CAMERA_THIN_LENS) {
        if (!spt_is_finite(m->lens_radius) || !(m->lens_radius >= 0.0f)) return "camera model: lens_radius must be finite and >= 0";
        if (!spt_is_finite(m->focus_distance) || !(m->focus_distance > 0.0f)) return "camera model: focus_distance must be finite and > 0";
    }
    if (m->type == SPT_CAMERA_ORTHOGRAPHIC && (!spt_is_finite(m->view_height) || !(m->view_height > 0.0f)))
        return "camera model: view_height must be finite and > 0";
    return 0;
}

SPT_CM_HD void spt_cm_normalize(float vx, float vy, float vz, float* d) {
    const float len = spt_sqrt((vx * vx + vy * vy) + vz * vz);
    d[0] = vx / len; d[1] = vy / len; d[2] = vz / len;
}

/* The lens point of sample plan_index of `pixel` on the unit disk */
SPT_CM_HD void spt_cm_lens_point(uint64_t seed, uint32_t pixel, uint32_t plan_index, float* lx, float* ly) {
    spt_rng r = spt_rng_seed(seed ^ SPT_CAMERA_SEED_SALT, pixel, plan_index);
    const float u1 = spt_rng_f32(&r);
    const float u2 = spt_rng_f32(&r);
    const float a = 2.0f * u1 - 1.0f, b = 2.0f * u2 - 1.0f;
    if (a == 0.0f && b == 0.0f) { *lx = 0.0f; *ly = 0.0f; return; }
    float r_, phi;
    if (spt_abs(a) > spt_abs(b)) { r_ = a; phi = (SPT_PI / 4.0f) * (b / a); }
    else { r_ = b; phi = SPT_PI / 2.0f - (SPT_PI / 4.0f) * (a / b); }
    *lx = r_ * spt_cos(phi);
    *ly = r_ * spt_sin(phi);
}

/* The ray of the model through the screen point (x, y); lx, ly: the sample's lens point (THIN_LENS only).
 * (Component by component, no loop: the arrays stay in registers on the device.) */
SPT_CM_HD float spt_cm_du(const spt_camera* c, int k, float x, float y) { return (c->forward[k] * c->half_cot_half_fov + c->right[k] * x) + c->up[k] * y; }
SPT_CM_HD float spt_cm_lens_offset(const spt_camera_model* m, int k, float lx, float ly) { return (m->base.right[k] * lx + m->base.up[k] * ly) * m->lens_radius; }
SPT_CM_HD void spt_cm_ray(const spt_camera_model* m, const spt_cm_plan* pl, float x, float y, float lx, float ly, float* o, float* d) {
    const spt_camera* c = &m->base;
    if (m->type == SPT_CAMERA_ORTHOGRAPHIC) {
        const float sx = x * m->view_height, sy = y * m->view_height;
        o[0] = c->eye[0] + (c->right[0] * sx + c->up[0] * sy);
        o[1] = c->eye[1] + (c->right[1] * sx + c->up[1] * sy);
        o[2] = c->eye[2] + (c->right[2] * sx + c->up[2] * sy);
        d[0] = c->forward[0]; d[1] = c->forward[1]; d[2] = c->forward[2];
    } else if (m->type == SPT_CAMERA_PANORAMA) {
        const float ph = (x * pl->aspect_inv) * (2.0f * SPT_PI);
        const float th = (0.5f - y) * SPT_PI;
        float st, ct, sp, cp;
        spt_sincos(th, &st, &ct);
        spt_sincos(ph, &sp, &cp);
        o[0] = c->eye[0]; o[1] = c->eye[1]; o[2] = c->eye[2];
        spt_cm_normalize(st * sp, ct, st * cp, d);
    } else {
        const float du0 = spt_cm_du(c, 0, x, y), du1 = spt_cm_du(c, 1, x, y), du2 = spt_cm_du(c, 2, x, y);
        if (m->type == SPT_CAMERA_THIN_LENS) {
            const float lo0 = spt_cm_lens_offset(m, 0, lx, ly), lo1 = spt_cm_lens_offset(m, 1, lx, ly), lo2 = spt_cm_lens_offset(m, 2, lx, ly);
            o[0] = c->eye[0] + lo0; o[1] = c->eye[1] + lo1; o[2] = c->eye[2] + lo2;
            spt_cm_normalize(du0 * pl->ft - lo0, du1 * pl->ft - lo1, du2 * pl->ft - lo2, d);
        } else {
            o[0] = c->eye[0]; o[1] = c->eye[1]; o[2] = c->eye[2];
            spt_cm_normalize(du0, du1, du2, d);
        }
    }
}

/* The screen point of pixel (i, image row j) at offsets (ox, oy): pt.rs:269-271 */
SPT_CM_HD void spt_cm_screen(uint32_t i, uint32_t j, uint32_t height, float ox, float oy, float width_inv, float height_inv, float aspect, float* x, float* y) {
    *x = (((float)i + ox) * width_inv - 0.5f) * aspect;
    *y = ((float)(height - j - 1u) + oy) * height_inv - 0.5f;
}
#endif /* SPT_CAMERA_MODELS_H */
