// The arithmetic of a BLAS refit (spt_scene_deform, large-scene form): the bounds of a leaf's triangles, the outward padding of
// a box and the quantisation of a compressed 4-wide node's children, verified with the decode of node4_test (trace.h).  Plain
// inline functions of f32 operations: the refit kernels (inst_deform.hip) and the host (scene_build.cpp, tests/
// scene_deform_refit_check.cpp) compile the same code.  No HIP intrinsic beyond what spt_detmath.h wraps.
#pragma once
#include <hip/hip_vector_types.h>   // float4

#include <cstdint>

#include "../../../include/spt_abi.h"
#include "../../../include/spt_detmath.h"
#include "scene_consts.h"

// The raw (unpadded) bounds of a subtree: what a refit keeps per node between its levels, 24 bytes
struct RefitBox {
    float lo[3], hi[3];
};

SPT_HD float refit_min(float a, float b) { return b < a ? b : a; }
SPT_HD float refit_max(float a, float b) { return b > a ? b : a; }

SPT_HD RefitBox refit_empty() {
    RefitBox b;
    for (int k = 0; k < 3; ++k) { b.lo[k] = spt_inf(); b.hi[k] = -spt_inf(); }
    return b;
}

SPT_HD void refit_grow(RefitBox& b, const RefitBox& o) {
    for (int k = 0; k < 3; ++k) { b.lo[k] = refit_min(b.lo[k], o.lo[k]); b.hi[k] = refit_max(b.hi[k], o.hi[k]); }
}

// the bounds of a triangle in ABI form (three vertices), as the BLAS builder takes them (build_sah_blas)
SPT_HD void refit_grow_tri(RefitBox& b, const float* p0, const float* p1, const float* p2) {
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = refit_min(b.lo[k], refit_min(p0[k], refit_min(p1[k], p2[k])));
        b.hi[k] = refit_max(b.hi[k], refit_max(p0[k], refit_max(p1[k], p2[k])));
    }
}

// Outward padding of a box along one axis (why these amounts: scene_build.cpp, "device-side BLAS").  Every f32 operation in it
// is monotone, so the pad of a box inside another is no larger than the other's.
SPT_HD float refit_pad(float lo, float hi) {
    return (hi - lo) * 1.52587890625e-5f /* 2^-16 */ + refit_max(spt_abs(lo), spt_abs(hi)) * 9.5367431640625e-7f /* 2^-20 */ + 1e-30f;
}

SPT_HD RefitBox refit_padded(const RefitBox& raw) {
    RefitBox p;
    for (int k = 0; k < 3; ++k) {
        const float pad = refit_pad(raw.lo[k], raw.hi[k]);
        p.lo[k] = raw.lo[k] - pad;
        p.hi[k] = raw.hi[k] + pad;
    }
    return p;
}

// The exponent e of a node's quantisation frame along one axis: the smallest with 2^e * 254 >= ext, clamped to -120 (an
// extent of 0 or below 2^-120 * 254 takes -120).  > 120: the extent cannot be quantised (infinite, or beyond 2^120 * 254).
SPT_HD int refit_exponent(float ext) {
    if (!(ext > 0.0f)) return -120;
    if (!spt_is_finite(ext)) return 127;
    const int E = (int)((spt_f2u(ext) >> 23) & 0xffu) - 127;   // ext in [2^E, 2^(E + 1)); subnormal: E = -127, clamped below
    int e = E - 7;                                            // 254 * 2^(E - 8) < 2^E <= ext, so e is E - 7 or E - 6
    if (e < -120) return -120;
    if (e <= 120 && 254.0f * spt_u2f((uint32_t)(e + 127) << 23) < ext) ++e;
    return e;
}

// p + 2^e * (float)q: the decode of node4_test
SPT_HD float refit_decode(float p, float scale, int q) {
    const float m = scale * (float)q;
    return p + m;
}

// One compressed 4-wide node from the raw bounds of its n children (build_n4's frame and rounding): origin = the padded min of
// their union, children's padded boxes rounded outward and widened until the decode contains them.  Writes f[0].xyz, the three
// exponents of f[0].w (its child count stays), f[1] and f[2].xy; the refs (f[2].zw, f[3]) are not touched.  Children c >= n keep
// the empty box (255, 0).  Returns the union.
SPT_HD RefitBox refit_node(float4* f, const RefitBox* child, uint32_t n) {
    RefitBox raw = refit_empty();
    for (uint32_t c = 0; c < n && c < 4u; ++c) refit_grow(raw, child[c]);
    const RefitBox par = refit_padded(raw);
    const float pmin[3] = {par.lo[0], par.lo[1], par.lo[2]};
    uint32_t eb[3], qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        int e = refit_exponent(par.hi[k] - par.lo[k]);
        if (e > 120) e = 120;   // (refused on the host before any kernel runs: refit_exponent of the mesh's own box)
        eb[k] = (uint32_t)(e + 127);
        const float scale = spt_u2f(eb[k] << 23), inv_scale = spt_u2f((uint32_t)(127 - e) << 23);
        for (uint32_t c = 0; c < 4u; ++c) {
            int lo = 255, hi = 0;   // absent child: empty box
            if (c < n) {
                const float pad = refit_pad(child[c].lo[k], child[c].hi[k]);
                const float clo = child[c].lo[k] - pad, chi = child[c].hi[k] + pad;
                float tl = (clo - pmin[k]) * inv_scale, th = (chi - pmin[k]) * inv_scale;
                tl = refit_min(refit_max(tl, 0.0f), 255.0f);
                th = refit_min(refit_max(th, 0.0f), 255.0f);
                if (!(tl == tl)) tl = 0.0f;
                if (!(th == th)) th = 255.0f;
                lo = (int)tl;                       // floor of a value >= 0
                hi = (int)th;
                if ((float)hi < th) ++hi;           // ceil
                while (lo > 0 && refit_decode(pmin[k], scale, lo) > clo) --lo;
                while (hi < 255 && refit_decode(pmin[k], scale, hi) < chi) ++hi;
            }
            qlo[k] |= (uint32_t)lo << (8u * c);
            qhi[k] |= (uint32_t)hi << (8u * c);
        }
    }
    const uint32_t hdr = spt_f2u(f[0].w);
    f[0].x = pmin[0]; f[0].y = pmin[1]; f[0].z = pmin[2];
    f[0].w = spt_u2f((hdr & 0xff000000u) | eb[0] | (eb[1] << 8) | (eb[2] << 16));
    f[1].x = spt_u2f(qlo[0]); f[1].y = spt_u2f(qlo[1]); f[1].z = spt_u2f(qlo[2]); f[1].w = spt_u2f(qhi[0]);
    f[2].x = spt_u2f(qhi[1]); f[2].y = spt_u2f(qhi[2]);
    return raw;
}
