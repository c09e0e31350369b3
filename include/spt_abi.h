/*
 * spt_abi.h — C ABI of the MI355X path-tracing integrator (libspt_hip.so).
 *
 * This is the drop-in seam for the reference's renderer boundary
 *     pub trait RendererT { fn render(&self, scene: &Scene, config: &OutputConfig); }
 *                                            (reference src/renderer/mod.rs:16-19)
 * selected by the renderer JSON "type" string in create_renderer
 * (src/renderer/mod.rs:26-38) and called once from src/main.rs:61.  The reference
 * has no FFI of its own; a Rust host adds a `Renderer::PathTracerHip` variant that
 * flattens its `Scene` into the POD arrays below and calls these entry points
 * (binding shown in INTEGRATION.md).
 *
 * Conventions
 *  - plain C, no C++/torch types; all pointers in descriptors are HOST pointers
 *    borrowed for the duration of the call (the library copies what it keeps).
 *  - every function returns spt_status (0 = OK); nothing panics/aborts/throws
 *    across the boundary (the reference panics: src/renderer/pt.rs:287,
 *    src/core/scene.rs:29-41); spt_last_error() gives a thread-local message.
 *  - there is NO CPU fallback behind this ABI: without a usable gfx950 device
 *    spt_scene_create fails with SPT_ERR_NO_DEVICE.
 *  - all arithmetic is IEEE f32 (reference: glam Vec3A / Color f32).
 */
#ifndef SPT_ABI_H
#define SPT_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPT_ABI_VERSION 14

typedef int32_t spt_status;
enum {
    SPT_OK = 0,
    SPT_ERR_INVALID_ARG = 1,   /* null pointer, bad size, inconsistent descriptor */
    SPT_ERR_NO_DEVICE = 2,     /* no HIP device / not gfx950 / device index out of range */
    SPT_ERR_HIP = 3,           /* a HIP runtime call failed (message has the HIP error string) */
    SPT_ERR_UNSUPPORTED = 4,   /* feature outside the hot-path scope (e.g. an unknown primitive type) */
    SPT_ERR_OUT_OF_MEMORY = 5
};

/* ---- geometry ----------------------------------------------------------------*/

/* One node of a binary BVH, 32 B = two 16-B loads.
 * Replaces the heap BvhNode {lc, rc, bbox, start, end} of src/primitive/bvh.rs:14-20.
 *   inner: a = index of left child, b = index of right child (absolute, same array)
 *   leaf : a = first item,  b = SPT_LEAF_FLAG | item count
 * Items are triangles (BLAS, absolute index into tri_pos) or instances (TLAS). */
#define SPT_LEAF_FLAG 0x80000000u
typedef struct spt_bvh_node {
    float bmin[3];
    uint32_t a;
    float bmax[3];
    uint32_t b;
} spt_bvh_node;

/* Triangle positions in BLAS leaf order (MeshVertex.position of the three
 * corners, src/primitive/triangle.rs:124-127). 48 B = three 16-B loads; the
 * 4th lane of each row is padding (36 algorithmic bytes). */
typedef struct spt_tri_pos {
    float p0[3]; float pad0;
    float p1[3]; float pad1;
    float p2[3]; float pad2;
} spt_tri_pos;

/* Per-corner shading attributes of the same triangle, read once per hit
 * (src/primitive/triangle.rs:188-212): 132 algorithmic bytes, padded to 144. */
typedef struct spt_tri_attr {
    float n[3][3];   /* normals        */
    float t[3][3];   /* tangents       */
    float b[3][3];   /* bitangents     */
    float uv[3][2];  /* texcoords      */
    float pad[3];
} spt_tri_attr;

typedef struct spt_sphere {   /* src/primitive/sphere.rs:8-12 */
    float center[3];
    float radius;
} spt_sphere;

typedef struct spt_mesh {     /* one TriMesh = one BLAS (src/primitive/triangle.rs:19-21) */
    uint32_t root;            /* index of the BLAS root in blas_nodes */
    uint32_t node_count;
    uint32_t tri_first;       /* first triangle (tri_pos / tri_attr index) */
    uint32_t tri_count;
} spt_mesh;

/* One bicubic Bezier patch (src/primitive/bezier.rs:19-22): cp[i][j] = control_points[i][j] (xyz; w unused, except:)
 * point_at(u, v) = sum_ij B_j(u) B_i(v) cp[i][j] (bezier.rs:40-44, 222-236).  The instance's box is the hull's.
 * ABI v12: cp[0][0][3] selects the intersection routine, as the reference's Cargo feature `bezier_ni` does at compile time
 * (Cargo.toml:34-36): 0 = Bezier clipping (bezier.rs:105-134, 239-422, the default build), SPT_BEZIER_NEWTON = Newton's
 * iteration from the middle of the patch inside its bounding box (bezier.rs:58-103). */
#define SPT_BEZIER_NEWTON 1.0f
typedef struct spt_bezier_patch {
    float cp[4][4][4];
} spt_bezier_patch;       /* 256 B */

enum { SPT_PRIM_SPHERE = 0, SPT_PRIM_MESH = 1, SPT_PRIM_BEZIER = 2 };

/* Instance = primitive + transform + surface (src/primitive/instance.rs:10-16).
 * Matrices are stored as glam stores them: three columns then the translation;
 * a point maps to ((c0*x + c1*y) + c2*z) + t, a vector without t
 * (Affine3A::transform_point3a / transform_vector3a). */
typedef struct spt_instance {
    float inv[12];        /* trans_inv : world -> object                        */
    float fwd[12];        /* trans     : object -> world                        */
    float nrm[9];         /* trans_it = transpose(inverse(M).matrix3), 3 columns */
    uint32_t prim_type;   /* SPT_PRIM_*                                          */
    uint32_t prim_id;     /* sphere, mesh or Bezier-patch index                  */
    uint32_t surface;     /* index into surfaces                                 */
    int32_t light;        /* index of this instance's ShapeLight in lights, -1 if not emissive
                             (instance_light_map, src/core/scene_resources.rs:112-120) */
    float bmin[3];        /* world bbox (Instance::bbox)                          */
    float bmax[3];
    float pad[5];
} spt_instance;           /* 48 words = 192 B */

/* ---- appearance ----------------------------------------------------------------*/

/* Materials with scalar textures evaluate to a constant Bxdf variant, so the
 * host resolves MaterialT::bxdf_context (src/material/{lambert,conductor,
 * dielectric,pseudo}.rs) once: alpha = roughness^2, alpha < 1e-4 -> specular. */
enum {
    SPT_BXDF_LAMBERT = 0,              /* src/bxdf/lambert.rs               */
    SPT_BXDF_MICROFACET_CONDUCTOR = 1, /* src/bxdf/microfacet_conductor.rs  */
    SPT_BXDF_SPECULAR_CONDUCTOR = 2,   /* src/bxdf/specular_conductor.rs    */
    SPT_BXDF_MICROFACET_DIELECTRIC = 3,/* src/bxdf/microfacet_dielectric.rs */
    SPT_BXDF_SPECULAR_DIELECTRIC = 4,  /* src/bxdf/specular_dielectric.rs   */
    SPT_BXDF_PSEUDO = 5,               /* src/bxdf/pseudo.rs                */
    SPT_BXDF_MICROFACET_PLASTIC = 6,   /* src/bxdf/microfacet_plastic.rs    */
    SPT_BXDF_SPECULAR_PLASTIC = 7,     /* src/bxdf/specular_plastic.rs      */
    SPT_BXDF_PNDF_CONDUCTOR = 8,       /* MicrofacetConductor over a PndfMicrofacet (src/bxdf/microfacet.rs:56-170); only ever
                                          the result of a per-hit recipe (SPT_MAT_PNDF_CONDUCTOR), never a constant material */
    SPT_BXDF_PNDF_PLASTIC = 9          /* MicrofacetPlastic over a PndfMicrofacet (SPT_MAT_PNDF_PLASTIC), per hit only too */
};
/* plastic lobes = Fresnel-weighted specular coat over a substrate (materials plastic, pbr_metallic,
 * pbr_specular; src/material/{plastic,pbr_metallic,pbr_specular}.rs) */
enum { SPT_FRESNEL_DIELECTRIC = 0, SPT_FRESNEL_SCHLICK = 1 };   /* src/bxdf/fresnel.rs:19-59 */
enum { SPT_SUBSTRATE_LAMBERT = 0, SPT_SUBSTRATE_DIFFUSE = 1,    /* src/bxdf/substrate.rs:22-45,120-180 */
       SPT_SUBSTRATE_SUBSURFACE = 2 };                           /* substrate.rs:182-350: Diffuse + a BSSRDF probe ray */
typedef struct spt_material {
    uint32_t bxdf;
    float c0[3];     /* lambert: reflectance; conductor: ior (eta); plastic: substrate reflectance */
    float c1[3];     /* conductor: ior_k; plastic with Schlick Fresnel: r0; Subsurface substrate: d  */
    float ax, ay;    /* GGX roughness_x / roughness_y (as the material hands them to GgxMicrofacet) */
    float ior;       /* dielectric / plastic: int_ior / ext_ior                                     */
    float c2[3];     /* Diffuse substrate: bxdf_wo_fresnel (Diffuse::new, substrate.rs:127-137)     */
    uint32_t fresnel;    /* SPT_FRESNEL_*   (plastic lobes; conductors: SCHLICK = SchlickFresnel with r0 = c0, else ConductorFresnel) */
    uint32_t substrate;  /* SPT_SUBSTRATE_* (plastic lobes) */
    uint32_t recipe;     /* 0: the constants above are the Bxdf; k > 0: material_recipes[k - 1] is
                            evaluated at every hit (some parameter is an image texture) and the
                            constants only hold the values at the textures' average colours */
} spt_material;      /* 16 words = 64 B */

/* ---- textures (the files of src/texture) -------------------------------------------------
 * The closed `Texture` enum (src/texture/mod.rs:187-197) as a node table.  A named texture of
 * the scene file is TexInputModifier(SrgbTex(base)) with the two wrappers present only when
 * asked for (create_texture_from_params, mod.rs:210-243); binary ops point at named textures. */
enum {
    SPT_TEX_SCALAR = 0,    /* scalar.rs: value[3], alpha 1                              */
    SPT_TEX_IMAGE = 1,     /* image_tex.rs: mip pyramid `image`, trilinear              */
    SPT_TEX_ADD = 2, SPT_TEX_SUB = 3, SPT_TEX_MUL = 4, SPT_TEX_DIV = 5,   /* binary_op.rs: a (op) b */
    SPT_TEX_SRGB = 6,      /* srgb_tex.rs: sRGB -> linear on r,g,b of child a            */
    SPT_TEX_MODIFIER = 7   /* input_modifier.rs: input * tiling + offset, mode / wrap override, child a */
};
enum { SPT_TEXMODE_SPECIFIED = 0, SPT_TEXMODE_TEXCOORDS = 1, SPT_TEXMODE_POSITION = 2, SPT_TEXMODE_NORMAL = 3,
       SPT_TEXMODE_TANGENT = 4, SPT_TEXMODE_BITANGENT = 5 };                /* mod.rs:20-28 */
enum { SPT_TEXWRAP_REPEAT = 0, SPT_TEXWRAP_MIRROR_REPEAT = 1, SPT_TEXWRAP_CLAMP = 2, SPT_TEXWRAP_MIRROR_CLAMP = 3 };  /* mod.rs:36-42 */
enum { SPT_CHAN_R = 0, SPT_CHAN_G = 1, SPT_CHAN_B = 2, SPT_CHAN_A = 3 };
typedef struct spt_texture {
    uint32_t type;        /* SPT_TEX_*                                              */
    uint32_t a, b;        /* child texture indices (always smaller than this node's) */
    uint32_t image;       /* IMAGE: index into images                                */
    float value[3];       /* SCALAR                                                  */
    int32_t mode, wrap;   /* MODIFIER: SPT_TEXMODE_* / SPT_TEXWRAP_*, -1 = keep the incoming one */
    float tiling[3];      /* MODIFIER                                                */
    float offset[3];
    uint32_t pad;
} spt_texture;            /* 16 words = 64 B */

/* ImageTex::images (image_tex.rs:7-9): level 0 is the file as RGBA8 (what DynamicImage::get_pixel
 * returns), the rest is generate_mipmap's box pyramid down to 1x1.  Texels are r | g<<8 | b<<16 | a<<24. */
typedef struct spt_image { uint32_t first_level, n_levels; } spt_image;
typedef struct spt_image_level { uint32_t width, height, first_texel, pad; } spt_image_level;

/* A material whose parameters are not all constant: MaterialT::bxdf_context
 * (src/material/{lambert,conductor,dielectric,plastic,pbr_metallic,pbr_specular}.rs) restated as data. */
enum { SPT_MAT_LAMBERT = 0, SPT_MAT_CONDUCTOR = 1, SPT_MAT_DIELECTRIC = 2, SPT_MAT_PLASTIC = 3,
       SPT_MAT_PBR_METALLIC = 4, SPT_MAT_PBR_SPECULAR = 5, SPT_MAT_SUBSURFACE = 6,
       SPT_MAT_PNDF_CONDUCTOR = 7,     /* pndf_conductor.rs:156-196: tex[0] albedo, tex[1] = index into pndfs (not a texture),
                                          tex[2] fallback_roughness (read when the pixel footprint sigma_p is 0) */
       SPT_MAT_PNDF_PLASTIC = 8 };     /* pndf_plastic.rs:163-211: the same slots + ior; DielectricFresnel, Diffuse substrate */
typedef struct spt_material_recipe {
    uint32_t type;         /* SPT_MAT_* */
    uint32_t tex[4];       /* texture indices: [0] albedo | ior | base_color | diffuse, [1] ior_k | metallic | specular | ld,
                              [2] roughness_x, [3] roughness_y (unused slots: 0) */
    uint32_t rough_chan;   /* SPT_CHAN_* read from tex[2], tex[3] (the JSON loader always says R) */
    uint32_t metal_chan;   /* SPT_CHAN_* read from tex[1] of PBR_METALLIC                      */
    float ior;             /* DIELECTRIC / PLASTIC: int_ior / ext_ior                          */
} spt_material_recipe;     /* 8 words */

/* ---- position-normal distributions ("glints", src/bxdf/pndf_bvh.rs, src/material/pndf_conductor.rs) -----------------
 * One Gaussian term per cell of the material's normal map (PndfGaussTerm, pndf_bvh.rs:4-11, 405-437). */
typedef struct spt_pndf_term {
    float u[2];        /* cell centre in texture space                                 */
    float s[2];        /* (x, y) of the normal there                                     */
    float jacobian[4]; /* ds/du, columns (dsdu, dsdv) (glam Mat2: x_axis, y_axis)      */
    float mat_a[4], mat_s[4], mat_mu[4];   /* PndfGaussTerm::new, column-major like glam */
} spt_pndf_term;       /* 20 words = 80 B */
/* A node of PndfBvh (4-D boxes over (u, s), pndf_bvh.rs:19-25, 124-190) or of PndfUvBvh (2-D boxes over u, the last two
 * box coordinates are 0; pndf_bvh.rs:35-41, 266-333).  Both split their index range in the middle, without sorting. */
typedef struct spt_pndf_node {
    float bmin[4], bmax[4];
    uint32_t start, end;   /* range in pndf_refs, relative to the owning tree's first ref */
    uint32_t lc, rc;       /* children (absolute node indices), 0xffffffff in a leaf       */
} spt_pndf_node;       /* 12 words = 48 B */
typedef struct spt_pndf {  /* PndfConductor + PndfAccel (pndf_conductor.rs:16-28, pndf_bvh.rs:49-92) */
    uint32_t first_term, n_terms;       /* pndf_terms */
    uint32_t s_block_count;             /* the s-plane [-1, 1]^2 is cut into s_block_count^2 blocks, one PndfBvh each */
    uint32_t first_root;                /* pndf_roots[first_root + x * s_block_count + y] = root node of that block or 0xffffffff,
                                           followed by the first ref of the block's term list */
    uint32_t uv_root, uv_first_ref;     /* PndfUvBvh over all terms */
    float sigma_r, sigma_hx, sigma_hy;
    float tiling[2], offset[2];         /* base_normal.tiling() / offset() (texcoords -> u) */
    uint32_t pad[3];
} spt_pndf;            /* 16 words = 64 B */

enum { SPT_SURF_DOUBLE_SIDED = 1u };
typedef struct spt_surface {  /* src/core/surface.rs:14-22 */
    uint32_t material;
    uint32_t flags;
    int32_t inside_medium;    /* medium index or -1 */
    float emissive[3];
    uint32_t normal_map;      /* texture index + 1, 0 = none (Surface::coord, surface.rs:65-78)      */
    uint32_t emissive_map;    /* texture index + 1, 0 = none (Surface::emissive, surface.rs:49-55)   */
} spt_surface;                /* 8 words */

typedef struct spt_medium {   /* src/medium/homogeneous.rs:11-15 */
    float sigma_t[3];
    float sigma_s[3];
    float g;
    float pad;
} spt_medium;

enum {
    SPT_LIGHT_DIRECTIONAL = 0, /* src/light/directional.rs (direction stored normalised) */
    SPT_LIGHT_POINT = 1,       /* src/light/point.rs       */
    SPT_LIGHT_SPOT = 2,        /* src/light/spot.rs        */
    SPT_LIGHT_SHAPE = 3,       /* src/light/shape_light.rs */
    SPT_LIGHT_ENV = 4          /* src/light/environment.rs */
};
typedef struct spt_light {
    uint32_t type;
    float pos[3];        /* point/spot position                        */
    float dir[3];        /* directional/spot direction                 */
    float strength[3];
    float cos_inner, cos_outer;
    uint32_t instance;   /* SHAPE: instance index                      */
    float power;         /* LightT::power() (alias-table input)        */
    float pad[2];
} spt_light;             /* 16 words */

enum { SPT_LIGHT_SAMPLER_UNIFORM = 0, SPT_LIGHT_SAMPLER_POWER_IS = 1 };

/* AliasTable (src/core/alias_table.rs:1-5): props / u / k, all length n. */
typedef struct spt_alias_table {
    uint32_t n;
    const float* props;
    const float* u;
    const uint32_t* k;
} spt_alias_table;

typedef struct spt_env {      /* EnvLight (src/light/environment.rs:10-17) */
    uint32_t width, height;   /* 0,0 = no environment */
    const float* texels;      /* height*width RGB f32, row 0 = theta 0 */
    float scale[3];
    spt_alias_table alias;    /* n = width*height */
} spt_env;

enum { SPT_AGGREGATE_GROUP = 0, SPT_AGGREGATE_BVH = 1 };

/* The flattened Scene (src/core/scene.rs:9-14 + everything it points to). */
typedef struct spt_scene_desc {
    uint32_t abi_version;          /* SPT_ABI_VERSION */
    uint32_t aggregate;            /* SPT_AGGREGATE_*: GROUP skips the top-level box test
                                      (src/primitive/group.rs:34-40) */
    uint32_t n_tlas_nodes;  const spt_bvh_node* tlas_nodes;  /* leaves index instances */
    uint32_t n_instances;   const spt_instance* instances;   /* in TLAS leaf order     */
    uint32_t n_meshes;      const spt_mesh* meshes;
    uint32_t n_blas_nodes;  const spt_bvh_node* blas_nodes;
    uint32_t n_tris;        const spt_tri_pos* tri_pos;  const spt_tri_attr* tri_attr;
    uint32_t n_spheres;     const spt_sphere* spheres;
    uint32_t n_surfaces;    const spt_surface* surfaces;
    uint32_t n_materials;   const spt_material* materials;
    uint32_t n_mediums;     const spt_medium* mediums;
    uint32_t n_lights;      const spt_light* lights;
    uint32_t light_sampler;        /* SPT_LIGHT_SAMPLER_* */
    int32_t env_light_index;       /* index of the ENV light in lights, -1 if none */
    spt_alias_table light_alias;   /* POWER_IS only (n = n_lights) */
    spt_env env;
    /* image textures (all zero / null for a scene with constant materials) */
    uint32_t n_textures;          const spt_texture* textures;
    uint32_t n_images;            const spt_image* images;
    uint32_t n_image_levels;      const spt_image_level* image_levels;
    uint32_t n_texels;            const uint32_t* texels;
    uint32_t n_material_recipes;  const spt_material_recipe* material_recipes;
    /* bicubic Bezier patches (instances with prim_type SPT_PRIM_BEZIER) */
    uint32_t n_bezier_patches;    const spt_bezier_patch* bezier_patches;
    /* position-normal distributions (materials with a SPT_MAT_PNDF_CONDUCTOR / _PLASTIC recipe; ABI v10) */
    uint32_t n_pndfs;             const spt_pndf* pndfs;
    uint32_t n_pndf_terms;        const spt_pndf_term* pndf_terms;
    uint32_t n_pndf_nodes;        const spt_pndf_node* pndf_nodes;
    uint32_t n_pndf_refs;         const uint32_t* pndf_refs;     /* term indices (absolute), the trees' term lists back to back */
    uint32_t n_pndf_roots;        const uint32_t* pndf_roots;    /* pairs (root node, first ref) per s-block                    */
} spt_scene_desc;

/* PerspectiveCamera after ::new (src/camera/perspective.rs:15-27). */
typedef struct spt_camera {
    float eye[3];
    float forward[3];   /* normalised                  */
    float up[3];        /* right x forward             */
    float right[3];     /* normalize(forward x up_in)  */
    float half_cot_half_fov;
} spt_camera;

enum { SPT_SAMPLER_RANDOM = 0, SPT_SAMPLER_JITTERED = 1, SPT_SAMPLER_RECURRENCE = 2 };

/* PathTracer{max_depth, pixel_sampler, filter} + OutputConfig{width,height}
 * (src/renderer/pt.rs:24-28, src/renderer/mod.rs:9-14) + the shard of the image
 * this call renders. */
typedef struct spt_render_params {
    uint32_t width, height;        /* full image */
    uint32_t spp;                  /* samples per pixel (jittered: division_x*division_y) */
    uint32_t max_depth;
    uint32_t sampler;              /* SPT_SAMPLER_* */
    uint32_t division_x, division_y; /* jittered only */
    uint64_t seed;
    /* row-strip sharding: this call renders rows j with (j / strip_rows) % shard_count
     * == shard_index; output rows are packed in increasing j.  shard_count=1 -> all. */
    uint32_t shard_index, shard_count, strip_rows;
    uint32_t samples_per_pass;     /* tuning: spp rendered per wavefront pass (0 = default) */
    uint32_t flags;                /* SPT_RENDER_* */
    uint64_t out_strip_stride;     /* bytes between the starts of consecutive strips of THIS shard in rgb_mean_out;
                                      0 = packed (strip_rows * width * 12).  shard_count * strip_rows * width * 12 with
                                      rgb_mean_out pointing at the shard's first row inside a full-image film makes every
                                      rank write its rows in place (one strided DMA, no host-side scatter) */
    float filter_radius;           /* BoxFilter::radius (src/filter/boxf.rs:5-14); read only with SPT_RENDER_BOX_RADIUS,
                                      otherwise 0.5 (every sample of a pixel and no other) */
    uint32_t stats_size;           /* sizeof(spt_render_stats) AS THE CALLER WAS COMPILED (ABI v9).  spt_render writes at most
                                      this many bytes of `stats`, so a caller built against an older, shorter struct is never
                                      written past its end (the struct only ever grows at the tail).  Must be set when `stats`
                                      is not NULL: 0 with a non-NULL `stats` is SPT_ERR_INVALID_ARG */
} spt_render_params;
enum {
    SPT_RENDER_PROFILE = 1u,       /* time each kernel class with HIP events */
    SPT_RENDER_BOX_RADIUS = 2u,    /* filter_radius is set */
    SPT_RENDER_COUNT_VISITS = 4u,  /* count BVH node / triangle / instance visits on the device (stats->*_visits); the counting
                                      kernels are separate instantiations, slower by a few per cent: measurement runs only */
    SPT_RENDER_ASYNC = 8u          /* ABI v11: return as soon as the work is queued.  The film's device-to-host copy runs on a
                                      copy stream of its own, so it overlaps the kernels of the NEXT spt_render on this scene
                                      (a caller that renders frame after frame pays max(kernels, copy) per frame instead of the
                                      sum).  rgb_mean_out (page-locked, or the copy is not asynchronous) is valid after
                                      spt_render_wait or after a later synchronous spt_render on the scene returns; `stats`
                                      must be NULL (counters would need the device to be idle) */
    ,
    SPT_RENDER_DEBUG_NORMAL = 16u  /* ABI v13: the reference's cargo feature `debug_normal` (Cargo.toml:34-36, src/renderer/pt.rs:113-118):
                                      a path's colour is `normal * 0.5 + 0.5` of the first surface it reaches (the world-space
                                      interpolated normal Instance::intersect leaves in the Intersection), nothing is shaded */
    ,
    SPT_RENDER_AOV_ALBEDO = 32u    /* additive to ABI v14 (detect it with spt_render_flags_supported): a path's colour is the ALBEDO `a` of
                                      the first surface it reaches; nothing is shaded, the path ends there, and a miss is black even
                                      with an environment.  `a` is read from the material record as evaluated at the hit (a per-hit
                                      recipe's textures, the P-NDF fallbacks), the three floats as they are:
                                        a = c0         SPT_BXDF_LAMBERT; the plastic lobes (MICROFACET_PLASTIC, SPECULAR_PLASTIC,
                                                       PNDF_PLASTIC); the conductors (MICROFACET_CONDUCTOR, SPECULAR_CONDUCTOR,
                                                       PNDF_CONDUCTOR) whose fresnel is SPT_FRESNEL_SCHLICK (r0 = c0)
                                        a = (1, 1, 1)  every other lobe: conductors with ConductorFresnel, both dielectrics, pseudo
                                      The surface's emission and its normal map do not enter.  Together with SPT_RENDER_DEBUG_NORMAL
                                      the plan is refused (SPT_ERR_INVALID_ARG) by spt_render and spt_film_create */
};
/* The SPT_RENDER_* bits this library honours (additive to ABI v14: a library without the symbol ignores unknown bits silently). */
spt_status spt_render_flags_supported(uint32_t* mask);

#define SPT_N_KERNELS 7
/* SHADE_FIRST: the shade launches of bounce 0 (one per pass, nearly all path vertices); SHADE: bounces >= 1 */
enum { SPT_K_PRIMARY = 0, SPT_K_SHADE = 1, SPT_K_SHADOW = 2, SPT_K_EXTEND = 3, SPT_K_RESOLVE = 4, SPT_K_OTHER = 5, SPT_K_SHADE_FIRST = 6 };
typedef struct spt_render_stats {
    uint64_t samples;              /* camera samples traced = rows*width*spp               */
    uint64_t segments_closest;     /* closest-hit ray segments (primary + extension)       */
    uint64_t segments_shadow;      /* any-hit ray segments                                 */
    double gpu_ms;                 /* HIP-event time of the whole call on the render stream */
    double kernel_ms[SPT_N_KERNELS];      /* per kernel class (SPT_RENDER_PROFILE only)     */
    uint32_t kernel_launches[SPT_N_KERNELS];
    uint64_t primary_hits;         /* camera samples whose primary ray hit something           */
    uint64_t path_vertices;        /* records consumed by the shade stage over all bounces     */
    uint64_t shadow_first;         /* any-hit segments issued by the bounce-0 shade launches   */
    uint64_t vertices_second;      /* path vertices of bounce 1 (= extension rays of bounce 0 that were kept) */
    uint64_t live_samples;         /* chunked k_primary: camera samples of pixels inside the screen-space bound, each of
                                      which owns a radiance slot; 0 when the un-chunked kernel ran */
    /* ABI v9, SPT_RENDER_COUNT_VISITS only (0 otherwise): what the traversal kernels fetched, summed over all ray segments */
    uint64_t node_visits;          /* BVH node records fetched (TLAS + BLAS; one record = one multi-child node)      */
    uint64_t tri_tests;            /* triangle records fetched and tested                                            */
    uint64_t instance_visits;      /* instance records fetched (ray transformed into object space)                   */
    uint64_t node_bytes;           /* bytes of the node records above (record sizes differ between the node formats)  */
    uint64_t class_visits[3][3];   /* the same three counters per kernel class: [primary, shadow, extend][node, triangle, instance] */
} spt_render_stats;

/* Closest-hit record: what BvhAccel/Group::intersect leave in `Intersection`
 * (src/core/intersection.rs:6-18) before shading: t, who was hit, barycentrics. */
typedef struct spt_hit {
    float t;              /* f32::MAX on miss */
    int32_t instance;     /* -1 on miss */
    int32_t prim;         /* triangle index (absolute) or sphere index */
    float v, w;           /* triangle barycentrics of p1, p2 (u = 1 - v - w) */
} spt_hit;

/* One ray: origin, t_min, direction, t_max (32 B). */
typedef struct spt_ray {
    float o[3]; float t_min;
    float d[3]; float t_max;
} spt_ray;

typedef struct spt_scene spt_scene;   /* opaque: device-resident copy of a spt_scene_desc */

spt_status spt_device_count(int32_t* count);
/* Validates desc, copies it to HBM on `device` (SoA-repacked), owns the copy. */
spt_status spt_scene_create(const spt_scene_desc* desc, int32_t device, spt_scene** out);
void spt_scene_destroy(spt_scene* scene);

/* spt_scene_update (additive to ABI v14: detect it by its symbol): moves instances and lights of a live scene without a rebuild.
 * The call replaces four fields of the descriptor the scene was created from - tlas_nodes, instances, lights, light_alias - and
 * keeps everything else (meshes, BLAS, triangles, spheres, patches, surfaces, materials, media, textures, P-NDF tables, the
 * environment, aggregate, light_sampler, env_light_index).  After SPT_OK every later call on the scene (spt_render, spt_film_*,
 * spt_trace_closest / _any, spt_radiance) returns the words a scene freshly created from the edited descriptor returns.
 *   - n_instances and n_lights must equal the creation's counts; the light at env_light_index keeps its type.  The arrays may be
 *     permuted (they are in the leaf order of tlas_nodes): spt_light::instance, spt_instance::light and spt_hit::instance refer to
 *     the new order.  The new arrays get every check spt_scene_create applies to these fields.
 *   - A scene created without Bezier instances refuses an update that introduces one (SPT_ERR_UNSUPPORTED); so is an update after
 *     which the traversal geometry no longer fits the form chosen at creation ("recreate the scene").
 *   - While a spt_film of the scene is alive the call is refused (SPT_ERR_INVALID_ARG): a film accumulates samples of one scene.
 *   - On any failure the scene is exactly as before.
 *   - Ordering: the uploads are queued on the scene's render stream.  Frames queued earlier with SPT_RENDER_ASYNC deliver the old
 *     scene's image, frames queued later the new one; the host waits only when the staging slot of the previous update is still
 *     being copied.
 *   - Cost: no triangle is read and no BLAS rebuilt.  Unless the traversal geometry is LDS-resident (<= 32 KB, re-uploaded whole),
 *     the bytes copied to the device are bounded by the instance and light counts (spt_debug_render_info, counter 5). */
typedef struct spt_scene_update_desc {
    uint32_t size;                 /* sizeof(spt_scene_update_desc) AS THE CALLER WAS COMPILED */
    uint32_t flags;                /* 0 */
    uint32_t n_tlas_nodes;  const spt_bvh_node* tlas_nodes;
    uint32_t n_instances;   const spt_instance* instances;   /* in the leaf order of tlas_nodes, as in spt_scene_desc */
    uint32_t n_lights;      const spt_light* lights;
    spt_alias_table light_alias;   /* POWER_IS scenes only, n = n_lights */
} spt_scene_update_desc;
spt_status spt_scene_update(spt_scene* scene, const spt_scene_update_desc* u);

/* spt_scene_deform (additive to ABI v14: detect it by its symbol): moves the vertices of meshes of a live scene.  Each named
 * mesh gets new tri_pos (and, if given, tri_attr) records for its whole range, in the order of the creation's descriptor: counts
 * and topology stay.  `u` is required - the instances' world boxes, a shape light's power and the alias table change with the
 * geometry - and gets every check and every meaning spt_scene_update gives it; n_meshes == 0 is spt_scene_update(scene, u).
 * After SPT_OK every later call on the scene returns the words a scene freshly created from the edited descriptor returns (but
 * for the triangle test's own grazing-ray false positives that any two trees over the same triangles can differ in).
 *   - Large scenes: the triangles are rewritten and the library's BLAS is refitted on the device, topology unchanged (no host
 *     build).  A tree refitted after a large deformation is walked more slowly than a rebuilt one: recreate the scene then.
 *     Scenes small enough to be walked from LDS get the named meshes' trees built again on the host.
 *   - Refused, the scene exactly as before: SPT_ERR_INVALID_ARG for a null array, a mesh index out of range or named twice, a
 *     wrong tri_count, a position that is not finite, a live film; SPT_ERR_UNSUPPORTED for a scene created under
 *     SPT_REFERENCE_BVH=1 (it walks the caller's trees), and when the geometry no longer fits the form chosen at creation.
 *   - Ordering: as spt_scene_update.  Counter 4 of spt_debug_render_info counts the call, counter 5 reports its bytes: at most
 *     the update's + 192 per triangle of the named meshes + 64; no triangle of another mesh is uploaded or read. */
typedef struct spt_mesh_deform {
    uint32_t mesh;                 /* index into the creation's meshes[] */
    uint32_t tri_count;            /* must equal meshes[mesh].tri_count */
    const spt_tri_pos*  tri_pos;   /* tri_count records, record k replaces triangle meshes[mesh].tri_first + k */
    const spt_tri_attr* tri_attr;  /* same order; NULL: the attributes stay */
} spt_mesh_deform;
spt_status spt_scene_deform(spt_scene* scene, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_deform* meshes);

/* spt_scene_mesh_topology / spt_scene_deform_vertices / spt_scene_read_triangles (additive to ABI v14: detect them by their
 * symbols): spt_scene_deform from vertex arrays.  A mesh's topology is registered once; a deformation then sends 12 bytes per
 * vertex (24 with normals) and the library makes the mesh's tri_pos / tri_attr records itself, with the loader's arithmetic
 * (include/spt_mesh_assemble.h: the tangent frames of TriMesh::calc_tangents, the records of TriMesh::new) - on the device for a
 * large scene, in front of the refit kernels of spt_scene_deform; on the host for an LDS-resident one, whose trees are built
 * there anyway.  The records are, word for word, what the host loader makes of the same vertices (a NaN stays a NaN).
 *   spt_scene_mesh_topology: indices are in FACE order, the order the tangents of a vertex are summed in; face_of_tri maps the
 *     mesh's triangle range onto the faces (the order a BLAS build chose).  Checked on the host: every index < n_vertices,
 *     face_of_tri a permutation, uv and normals finite, the mesh index, tri_count, size, null pointers (SPT_ERR_INVALID_ARG).
 *     Everything is copied: the caller's arrays may go after the call.  A second call for a mesh replaces its registration.
 *     Nothing a frame can see changes, so a live film does not refuse it.  SPT_ERR_UNSUPPORTED under SPT_REFERENCE_BVH=1.
 *   spt_scene_deform_vertices: `u`, the films rule, the ordering, atomicity on refusal and counters 4 / 5 / 6 of
 *     spt_debug_render_info are spt_scene_deform's.  Refused in addition, SPT_ERR_INVALID_ARG: a mesh without a registration, a
 *     wrong n_vertices, a value that is not finite, a mesh named twice.  Large scenes: counter 5 is at most the update's bound
 *     + 12 (24 with normals) per vertex of the named meshes + 64 per named mesh, and no record is uploaded.  An LDS-resident
 *     scene's records are made on the host and go the way of spt_scene_deform.
 *   spt_scene_read_triangles: copies records [first, first + count) of the scene's triangle arrays (the descriptor's order) out
 *     of device memory, behind everything queued on the render stream.  Range errors: SPT_ERR_INVALID_ARG. */
typedef struct spt_mesh_topology {
    uint32_t size, mesh;              /* sizeof(spt_mesh_topology) AS THE CALLER WAS COMPILED; index into the creation's meshes[] */
    uint32_t n_vertices, tri_count;   /* tri_count must equal meshes[mesh].tri_count */
    const uint32_t* indices;          /* 3 * tri_count vertex indices, in face order */
    const uint32_t* face_of_tri;      /* tri_count: triangle meshes[mesh].tri_first + k is face face_of_tri[k]; NULL = identity */
    const float* uv;                  /* 2 * n_vertices */
    const float* normals;             /* 3 * n_vertices: the normals a deformation without normals keeps */
} spt_mesh_topology;
spt_status spt_scene_mesh_topology(spt_scene* scene, const spt_mesh_topology* t);

typedef struct spt_mesh_vertices {
    uint32_t mesh, n_vertices;        /* n_vertices must equal the registration's */
    const float* positions;           /* 3 * n_vertices, host memory */
    const float* normals;             /* 3 * n_vertices, or NULL: the normals stay (the last ones given, else the registration's) */
} spt_mesh_vertices;
spt_status spt_scene_deform_vertices(spt_scene* scene, const spt_scene_update_desc* u, uint32_t n_meshes, const spt_mesh_vertices* meshes);

spt_status spt_scene_read_triangles(const spt_scene* scene, uint32_t first, uint32_t count, spt_tri_pos* tri_pos_out /* or NULL */,
                                    spt_tri_attr* tri_attr_out /* or NULL */);

/* spt_scene_origin_candidates (additive to ABI v14: detect it by its symbol): the per-origin-triangle candidate table the fused
 * simple shade kernels of the scene test their shadow and extension rays against (include/spt_origin_cand.h), as the device holds it
 * behind every update queued so far.  *n_rows_out = 0: none - the scene does not qualify (not served by the fused simple kernels,
 * an instance that is no triangle mesh, more than 64 triangles) or SPT_NO_ORIGIN_CANDIDATES=1 is set.  Else words_out (NULL: not
 * wanted; room for 4 x 64) receives 4 words per row - loose up, loose down, tight up, tight down; row = a triangle's index in
 * tri_pos, bit k = slot k of the library's own triangle order - and info_out (NULL: not wanted) 8 doubles: the scene's centre
 * (3) and radius, the reach (a render takes the path when its eye is within it of the centre), delta(reach), tight (0: the
 * tight words equal the loose ones), ns the host took to make the table. */
spt_status spt_scene_origin_candidates(const spt_scene* scene, uint64_t* words_out, uint32_t* n_rows_out, double* info_out);

/* The hot path: RendererT::render for one image shard.  rgb_mean_out receives
 * shard_rows*width*3 f32 = per-pixel mean radiance (Film::filter_pixel with the
 * box filter, src/core/film.rs:71-92: the sum of the samples of the (2 ceil(radius - 0.5) + 1)^2 pixels around it
 * over the number of those samples whose offset lies within `radius`), row 0 = top.  Synchronous. */
spt_status spt_render(const spt_scene* scene, const spt_camera* cam, const spt_render_params* params,
                      float* rgb_mean_out, spt_render_stats* stats /* may be NULL */);
/* Blocks until every spt_render queued on the scene with SPT_RENDER_ASYNC has delivered its film (ABI v11). */
spt_status spt_render_wait(const spt_scene* scene);
/* Number of image rows spt_render writes for these params. */
spt_status spt_shard_rows(const spt_render_params* params, uint32_t* rows);

/* ---- progressive rendering (ABI v14) ----------------------------------------------------------
 * A film owns one shard's running sums on the device.  `params` is the PLAN: spp stays its total and still drives the
 * jittered grid, the R2 index k = pixel * spp + s + 1 and the auxiliary-ray spread 1/sqrt(spp); each spt_film_render adds the
 * next samples of that plan in sample order, so increments summing to spp (first_sample 0) give the bits of one spt_render.
 * The film covers the samples [first_sample, first_sample + done).  Plans with SPT_RENDER_ASYNC / PROFILE / COUNT_VISITS or a
 * non-packed out_strip_stride are refused by spt_film_render (SPT_ERR_INVALID_ARG); a box filter that reaches neighbouring
 * pixels (ceil(radius - 0.5) >= 1) by spt_film_create (SPT_ERR_UNSUPPORTED) unless the film keeps its samples
 * (SPT_FILM_KEEP_SAMPLES).  Film calls take the scene's lock and never
 * touch the buffers of spt_render (an asynchronous copy-out may be reading them); a film is destroyed before its scene. */
typedef struct spt_film spt_film;
enum { SPT_FILM_MOMENTS = 1u, SPT_FILM_KEEP_SAMPLES = 2u };   /* MOMENTS: also keep the per-channel sum of squared sample radiance
                                                                 (SUM_SQ, VAR_OF_MEAN); KEEP_SAMPLES: see "films that keep
                                                                 their samples" below */
enum {
    SPT_FILM_MEAN = 0,            /* what spt_render returns for the covered samples: S * (1 / done), or S * (1 / wsum) for a box
                                     radius other than 0.5 (wsum = covered samples whose offset lies in the box); done > 0 */
    SPT_FILM_SUM = 1,             /* S: the running sum of the covered samples, in sample order                             */
    SPT_FILM_SUM_SQ = 2,          /* Q = Q + x * x per channel, in sample order (SPT_FILM_MOMENTS)                          */
    SPT_FILM_VAR_OF_MEAN = 3      /* m = S * (1/n); v = (Q * (1/n) - m * m) * (1/(n - 1)); max(v, 0); +inf at n == 1
                                     (SPT_FILM_MOMENTS, radius 0.5, n = done > 0)                                           */
};
spt_status spt_film_create(const spt_scene* scene, const spt_camera* cam, const spt_render_params* params,
                           uint32_t first_sample, uint32_t film_flags, spt_film** out);
/* Adds the next n_samples samples of the plan (0: nothing).  Synchronous.  A call that would pass the plan's spp is refused
 * (SPT_ERR_INVALID_ARG) and the film is left as it was. */
spt_status spt_film_render(spt_film* film, uint32_t n_samples);
spt_status spt_film_samples(const spt_film* film, uint32_t* done);
/* One of SPT_FILM_*: the shard's rows packed, rows * width * 3 f32 (spt_shard_rows of the plan). */
spt_status spt_film_read(spt_film* film, uint32_t what, float* out);
void spt_film_destroy(spt_film* film);   /* before spt_scene_destroy of its scene */

/* ---- films that keep their samples (additive to ABI v14: detect it by the flag) ----------------------------------------------------
 * SPT_FILM_KEEP_SAMPLES is a bit of spt_film_create's film_flags; a library without it refuses the bit as an unknown film flag
 * (SPT_ERR_INVALID_ARG).  Such a film keeps no running sums.  It keeps the radiance of every covered sample s in [first_sample,
 * first_sample + done) for every STORED row: the shard's own rows plus R = ceil(radius - 0.5) halo rows above and below every run of
 * consecutive own rows, clipped to the image.  Halo rows are traced again by this film, as spt_render does; a sample is a pure function
 * of (seed, pixel, plan index), so every copy of a row has the same bits and no shard needs another.  The store costs
 * stored rows * width * done * 12 bytes on the device and grows with every spt_film_render.
 * With the bit, spt_film_create takes every radius spt_render takes.  spt_film_read(SPT_FILM_MEAN) is Film::filter_pixel over the
 * covered samples, one rounded f32 operation at a time:
 *     color = 0; weight_sum = 0
 *     for dj = -R .. R, for di = -R .. R (pixels outside the image skipped), for the pixel's samples in increasing plan index:
 *         color += x (unweighted);  weight_sum += box_weight (1.0f if the sample's offset lies within the radius of the
 *                                                             reading pixel, else 0.0f)
 *     mean = color * (1.0f / weight_sum)
 * and SPT_FILM_SUM is `color`.  When the film covers the plan's [0, spp) the mean has the bits of spt_render with the same params, at
 * any radius and however the samples were cut into increments; for R < 0 both loops are empty and the mean is 0 * (1 / 0).  The
 * weights are 0.0f or 1.0f, so in f32 weight_sum equals min(count, 2^24) whatever the order of the additions: the library counts
 * in integers and clamps.  spt_film_read_rgb8(SPT_READ_MEAN) returns the bytes of that float read-out.
 * spt_film_read_samples returns the kept radiance itself: [count][rows][width][3] f32, the OWN rows packed like spt_film_read, plane k
 * the sample with plan index first + k.  A black sample, a pixel outside the screen bound and a plan with max_depth 0 give 0.
 * count == 0 or a film without rows: SPT_OK, nothing written.
 * Refusals leave the film as it was.  SPT_ERR_INVALID_ARG: KEEP_SAMPLES together with SPT_FILM_MOMENTS; spt_film_read_samples on a
 * null film or out, on a film without the flag, or with a range outside [first_sample, first_sample + done); spt_film_buckets on a
 * sample-keeping film.  spt_film_adapt, spt_film_denoise* and SUM_SQ / VAR_OF_MEAN are refused as for every film without moments,
 * spt_film_read_robust as for every film without buckets.  SPT_ERR_UNSUPPORTED: more than 2^31 - 1 stored pixels.
 * SPT_ERR_OUT_OF_MEMORY: an increment whose store cannot be allocated; done does not advance. */
spt_status spt_film_read_samples(spt_film* film, uint32_t first, uint32_t count, float* out);

/* ---- reconstruction filters of a sample-keeping film (additive to ABI v14: detect it by symbol) -----------------------------------
 * spt_film_filter chooses the filter of later spt_film_read(SPT_FILM_MEAN | SPT_FILM_SUM) and spt_film_read_rgb8(SPT_READ_MEAN)
 * calls on a film created with SPT_FILM_KEEP_SAMPLES.  It may be called at any time, any number of times; it launches nothing and
 * changes nothing of what the film keeps (done, the kept samples and spt_film_read_samples stay as they are).  SPT_FILTER_BOX
 * restores the state after spt_film_create, the reference's box at the plan's radius (radius, p0, p1 ignored); a film that never
 * calls spt_film_filter is read exactly as described above.
 * The plan's filter_radius still decides the stored halo, R = ceil(radius_plan - 0.5) rows.  A filter of support radius r needs
 * Rf = max(ceil(r - 0.5), 0) <= max(R, 0); because every copy of a row has the same bits, a film of a wider plan read under a
 * filter has the bits of a film whose plan radius is r.
 * The weighted read-out, every step one rounded f32 operation, no contraction, in this order:
 *     color = 0; wsum = 0
 *     for dj = -Rf .. Rf, for di = -Rf .. Rf (pixels outside the image skipped), for that pixel's covered samples in increasing
 *     plan index:
 *         ax = |(float)di + (ox - 0.5f)|;  ay = |(float)dj + (oy - 0.5f)|     (ox, oy: the sample's pixel offset, as the box derives it)
 *         skipped unless ax <= r and ay <= r
 *         w = f(ax) * f(ay);   skipped when w == 0.0f
 *         color.c = color.c + w * x.c   (c = r, g, b);   wsum = wsum + w
 *     SPT_FILM_SUM = color;   SPT_FILM_MEAN = color * (1.0f / wsum)
 *   TENT      f(a) = r - a
 *   GAUSSIAN  e_r = spt_exp(-(alpha * (r * r)));  g = spt_exp(-(alpha * (a * a))) - e_r;  f(a) = g < 0 ? 0 : g
 *             (spt_exp of spt_detmath.h)
 *   MITCHELL  t = (2.0f * a) / r, in [0, 2].  Seven coefficients are made once on the host: B and C widened to double, each
 *             expression below evaluated in double as written, left to right, and rounded once to f32.
 *               t > 1:      c3 = (-B - 6*C) / 6;  c2 = (6*B + 30*C) / 6;  c1 = (-12*B - 48*C) / 6;  c0 = (8*B + 24*C) / 6
 *                           f = ((c3 * t + c2) * t + c1) * t + c0
 *               otherwise:  q3 = (12 - 9*B - 6*C) / 6;  q2 = (-18 + 12*B + 6*C) / 6;  q0 = (6 - 2*B) / 6
 *                           f = ((q3 * t + q2) * t) * t + q0
 *             Negative lobes are kept: w may be negative.
 * Unlike the box, a sample outside the support, or one of weight 0, enters neither sum: a non-finite sample spoils only the pixels
 * whose support it lies in.
 * Refusals leave the film and its current filter as they were, all SPT_ERR_INVALID_ARG: a null film or desc; desc->size below
 * sizeof(spt_filter_desc); an unknown type; a film without SPT_FILM_KEEP_SAMPLES; for the types other than the box: r not finite
 * or <= 0, Rf above the film's stored halo (the message names the plan radius that would do), GAUSSIAN with alpha not finite or
 * <= 0, MITCHELL with B or C not finite.  Takes the scene's lock. */
enum { SPT_FILTER_BOX = 0, SPT_FILTER_TENT = 1, SPT_FILTER_GAUSSIAN = 2, SPT_FILTER_MITCHELL = 3 };
typedef struct spt_filter_desc {
    uint32_t size;     /* sizeof(spt_filter_desc) as the caller was compiled; the struct only grows at its tail */
    uint32_t type;     /* SPT_FILTER_* */
    float radius;      /* support radius r, in pixels */
    float p0, p1;      /* GAUSSIAN: p0 = alpha.  MITCHELL: p0 = B, p1 = C.  Otherwise ignored */
    uint32_t pad;
} spt_filter_desc;     /* 24 B */
spt_status spt_film_filter(spt_film* film, const spt_filter_desc* desc);

/* ---- adaptive sampling of a film (additive to ABI v14: detect it by symbol) -------------------------------------------------
 * spt_film_adapt, called between increments, RETIRES every still-active pixel whose error estimate meets the tolerance; a
 * retired pixel stays retired.  Later spt_film_render calls trace only the active pixels; a retired pixel keeps its S, its Q and
 * its sample count n_p.  All active pixels cover the same samples [first_sample, first_sample + done) (pixels only leave the
 * set), so n_p = done for them; spt_film_samples keeps returning done, the plan position, which advances on every
 * spt_film_render even when no pixel is active (that call traces nothing).  Because a sample depends only on (seed, pixel, plan
 * index) and the sums run in sample order, a retired pixel's sums are the bits of a plain film stopped at n_p samples.
 * Criterion, exact f32 (no contraction), per channel c, for an active pixel when n = done >= max(min_samples, 2), with
 * r(k) = 1.0f / (float)k:
 *     m_c = S_c * r(n);  v_c = max((Q_c * r(n) - m_c * m_c) * r(n - 1), 0)   (= SPT_FILM_VAR_OF_MEAN)
 *     tol_c = rel_error * |m_c| + abs_floor;   retire <=> v_c <= tol_c * tol_c for all three channels
 * No sqrt; a NaN never retires; rel_error = abs_floor = 0 retires exactly the zero-variance pixels.  After the first adapt,
 * SPT_FILM_MEAN is S * r(n_p) and SPT_FILM_VAR_OF_MEAN the formula above at n_p (+inf at n_p == 1), per pixel; SUM and SUM_SQ
 * are unchanged.  A film that never calls spt_film_adapt is a plain film.
 * Refusals leave the film unchanged: a null film or a film without SPT_FILM_MOMENTS (SPT_ERR_INVALID_ARG), a box radius other
 * than 0.5 (SPT_ERR_UNSUPPORTED), rel_error / abs_floor negative or not finite (SPT_ERR_INVALID_ARG).  min_samples < 2 counts
 * as 2; while done < max(min_samples, 2) the call retires nothing.  Synchronous. */
/* Retires the film's converged pixels (see above); *active_out (may be NULL) = pixels still active. */
spt_status spt_film_adapt(spt_film* film, float rel_error, float abs_floor, uint32_t min_samples, uint32_t* active_out);
/* rows * width u32: the samples each pixel covers (done for active pixels). */
spt_status spt_film_read_counts(spt_film* film, uint32_t* out);

/* ---- denoising a film (additive to ABI v14: detect it by symbol) -------------------------------------------------------------
 * spt_film_denoise READS two films and returns a filtered copy of the first one's mean; it changes neither.  The filter is a 5x5
 * a-trous wavelet (B3 spline, h = 1/16, 1/4, 3/8, 1/4, 1/16) run `iterations` times with step 2^k, whose weights compare the
 * luminance of two pixels with the variance of their means and - with a `guide` - the guide's values with the guide's variance.
 * The guide is any second film of the same scene object, size and shard layout with SPT_FILM_MOMENTS: e.g. the same plan with
 * SPT_RENDER_DEBUG_NORMAL, whose mean is the first-hit normal.  Exact f32, one rounded operation at a time, sums in this order:
 *     m, v = SPT_FILM_MEAN, SPT_FILM_VAR_OF_MEAN of the film at the pixel's own sample count; g, u = those of the guide
 *     lum(c) = (0.299f * c.r + 0.587f * c.g) + 0.114f * c.b
 *     lv_0 = ((0.299f * 0.299f) * v.r + (0.587f * 0.587f) * v.g) + (0.114f * 0.114f) * v.b;   gv = (u.r + u.g) + u.b;   c_0 = m
 *     for k = 0 .. iterations - 1, s = 1 << k, per pixel p, with ok(q) <=> c_k(q).rgb and lv_k(q) are all finite:
 *         acc = 0; ws = 0; va = 0
 *         for dy = -2 .. 2, for dx = -2 .. 2, q = p + s * (dx, dy), skipped when outside the image or !ok(q):
 *             dl = lum(c_k(p)) - lum(c_k(q));   d = (dl * dl) / ((k_color * k_color) * (lv_k(p) + lv_k(q)) + eps_color)
 *             guide: e = g(p) - g(q);   d = d + ((e.r * e.r + e.g * e.g) + e.b * e.b) / ((k_guide * k_guide) * (gv(p) + gv(q)) + eps_guide)
 *             skipped unless d < 87.0f (a NaN too)
 *             w = (h[dy + 2] * h[dx + 2]) * spt_exp(-d);   acc += w * c_k(q);   ws += w;   va += (w * w) * lv_k(q)
 *         ok(p): c_{k+1}(p) = acc / ws, lv_{k+1}(p) = va / (ws * ws);   else both pass through
 * A pixel that is not finite stays as it is and enters no other pixel's sum.  spt_exp is that of spt_detmath.h.
 * Refusals leave both films usable: SPT_ERR_INVALID_ARG for a null film or out, a film or guide without SPT_FILM_MOMENTS or with
 * fewer than 2 samples, guide == film, a guide of another scene object or with another width, height or shard layout, a guide
 * served by the other library than the film's, params->size below the struct's, iterations outside 1 .. 8, a k or eps that is
 * not finite and > 0; SPT_ERR_UNSUPPORTED for a box radius other than 0.5 on either film and for a plan with shard_count > 1 (a
 * shard's packed rows are not neighbours in the image).  Synchronous; the workspace belongs to `film` and goes with it. */
typedef struct spt_denoise_params {
    uint32_t size;         /* sizeof(spt_denoise_params): the struct only grows at its tail */
    uint32_t iterations;   /* 1 .. 8 */
    float k_color, k_guide, eps_color, eps_guide;   /* finite and > 0 */
} spt_denoise_params;
/* out: rows * width * 3 f32, packed, like spt_film_read.  guide and params may be NULL (no guide term; the defaults
 * iterations 5, k_color 2, k_guide 1, eps_color 1e-8, eps_guide 1e-2). */
spt_status spt_film_denoise(spt_film* film, spt_film* guide, const spt_denoise_params* params, float* out);

/* ---- denoising with an albedo film (additive to ABI v14: detect it by symbol) ------------------------------------------------------
 * spt_film_denoise_job is spt_film_denoise with a second guide, an ALBEDO film (any film of the same scene object, size and shard
 * layout with SPT_FILM_MOMENTS and at least 2 samples, e.g. the same plan with SPT_RENDER_AOV_ALBEDO), and with albedo
 * demodulation.  With albedo == NULL and flags without SPT_DENOISE_DEMODULATE the result is the bits of
 * spt_film_denoise(film, guide, params, out).  With an albedo film the specification above is extended, every step one rounded
 * f32 operation, in this order:
 *     al, ua = SPT_FILM_MEAN, SPT_FILM_VAR_OF_MEAN of the albedo film;   av = (ua.r + ua.g) + ua.b
 *     per tap, behind the guide's term (if there is a guide):
 *         e = al(p) - al(q);   d = d + ((e.r * e.r + e.g * e.g) + e.b * e.b) / ((k_albedo * k_albedo) * (av(p) + av(q)) + eps_albedo)
 *     SPT_DENOISE_DEMODULATE (needs an albedo film), per channel: dem = al > eps_demod ? al : eps_demod (a NaN albedo gives the floor)
 *         c_0 = m / dem;   v' = v / (dem * dem);   lv_0 from v' with the luminance weights above
 *         after the last iteration out = c_K * dem, for every pixel (those that passed through included)
 * The filter then never compares texture detail: it sees colour / albedo, and the albedo's detail comes back unblurred.
 * SPT_DENOISE_OUT_RGB8: `out` receives rows * width * 3 u8, the conversion of spt_film_read_rgb8; else rows * width * 3 f32.
 * Refusals are those of spt_film_denoise (the albedo film is checked exactly as the guide is), plus SPT_ERR_INVALID_ARG for a null
 * job, job->size below offsetof(spt_denoise_job, k_albedo), albedo == film or albedo == guide, unknown flags, DEMODULATE without an
 * albedo film, a k_albedo, eps_albedo or eps_demod that is not finite and > 0, and films that are not all served by the same
 * library.  The films are read only; the workspace belongs to `film`.  Synchronous. */
enum { SPT_DENOISE_DEMODULATE = 1u, SPT_DENOISE_OUT_RGB8 = 2u };
typedef struct spt_denoise_job {
    uint32_t size, flags;             /* sizeof(spt_denoise_job) as the caller was compiled; SPT_DENOISE_* */
    spt_film* guide;                  /* as in spt_film_denoise, may be NULL */
    spt_film* albedo;                 /* may be NULL */
    const spt_denoise_params* params; /* may be NULL: the defaults */
    float k_albedo, eps_albedo, eps_demod;   /* finite and > 0; the defaults 1, 1e-2, 1e-2 when size ends before them */
    uint32_t pad;
} spt_denoise_job;
spt_status spt_film_denoise_job(spt_film* film, const spt_denoise_job* job, void* out);

/* ---- denoising caller-provided images (additive to ABI v14: detect it by symbol) ----------------------------------------------------
 * spt_denoise_image is the filter of spt_film_denoise_job on images instead of films: what a caller has who assembled a full image
 * from shard films (spt_host_multi_film_denoise, ranks that gathered a film), none of which could be filtered on its own.  The
 * arithmetic is exactly the specification above, with m, v / g, u / al, ua taken from `mean`, `var` / `guide_mean`, `guide_var` /
 * `albedo_mean`, `albedo_var`: rows * width * 3 f32 each, packed RGB, as SPT_FILM_MEAN and SPT_FILM_VAR_OF_MEAN return them.  The
 * result has the bits of spt_film_denoise_job on films whose two read-outs are those arrays.  A +inf variance (a pixel with one
 * sample) or a NaN makes the pixel pass through and enter no other pixel's sum: ok(q) above.
 * The scene names the device and the stream; the call takes the scene's lock, its workspace (device images, page-locked staging,
 * records) belongs to the scene and goes with it, and it touches neither spt_render's buffers nor any film.  The arrays go up
 * with asynchronous copies, the host filling the staging slot of one array while the previous one is in flight.  Synchronous.
 * Refusals leave nothing changed: SPT_ERR_INVALID_ARG for a null scene, job, out, mean or var, half a pair of guide or albedo
 * arrays, job->size below offsetof(spt_image_denoise_job, k_albedo), unknown flags, DEMODULATE without the albedo arrays, and the
 * params, k_* and eps_* checks of spt_film_denoise_job; SPT_ERR_UNSUPPORTED for more than 2^32 - 4 floats per image.
 * width == 0 or rows == 0 returns SPT_OK and writes nothing. */
typedef struct spt_image_denoise_job {
    uint32_t size, flags;                    /* sizeof(spt_image_denoise_job) as the caller was compiled; SPT_DENOISE_* */
    uint32_t width, rows;
    const float *mean, *var;                 /* rows * width * 3 f32 each */
    const float *guide_mean, *guide_var;     /* both NULL or both set */
    const float *albedo_mean, *albedo_var;   /* both NULL or both set */
    const spt_denoise_params* params;        /* may be NULL: the defaults */
    float k_albedo, eps_albedo, eps_demod;   /* finite and > 0; the defaults 1, 1e-2, 1e-2 when size ends before them */
    uint32_t pad;
} spt_image_denoise_job;
/* out: rows * width * 3 f32, or u8 with SPT_DENOISE_OUT_RGB8 */
spt_status spt_denoise_image(const spt_scene* scene, const spt_image_denoise_job* job, void* out);

/* ---- bucketed films: median-of-means read-outs (additive to ABI v14: detect it by symbol) ------------------------------------
 * spt_film_buckets makes a film keep K = n_buckets bucket sums B_0 .. B_{K-1} per pixel and channel next to S (and Q).  The sample
 * with plan index s (absolute in the plan: first_sample counts) adds into bucket j = s % K, B_j = B_j + x per channel, in sample
 * order; a black sample adds nothing; B starts at +0.  S, Q, spt_film_adapt and spt_film_denoise of a bucketed film are those of
 * the same film without buckets, and a film that never calls spt_film_buckets is a plain film, bit for bit.
 * Counts (integer arithmetic): the pixel covers n_p samples - `done` for a plain film or an active pixel, the retired count of an
 * adaptive film otherwise - and bucket j holds n_j = #{ s in [first_sample, first_sample + n_p) : s % K == j } of them.
 * spt_film_read_robust, exact f32, one rounded operation at a time, no contraction, per pixel and channel, with
 * r(k) = 1.0f / (float)k as the host rounds it and h = (K - 1) / 2:
 *     n_p < K (some bucket is empty): the result is the plain mean S * r(n_p)
 *     mu_j = B_j * r(n_j);   key_j = finite(mu_j) ? mu_j + 0.0f : +inf;   a_0 <= ... <= a_{K-1}: the keys sorted ascending
 *     SPT_ROBUST_MON:  the result is a_h, the median of the bucket means
 *     SPT_ROBUST_GMON: num = sum_{i = 0 .. K-1} (float)(i + 1) * a_i and den = sum_{i = 0 .. K-1} a_i, both from i = 0 upward, from 0
 *         t = h                    if a_{K-1} is +inf (a bucket with a sample that is not finite)
 *         else t = 0               if !(den > 0)
 *         else G = (2.0f * num) / ((float)K * den) - ((float)(K + 1) / (float)K)      (the Gini coefficient of the bucket means)
 *              t = 0               if !(G > 0)
 *              t = h               if G * (float)h >= (float)h
 *              t = (uint32_t)(G * (float)h)   otherwise
 *         the result is (sum_{i = t .. K-1-t} a_i, from i = t upward) * r(K - 2t): the mean of the keys without the t lowest and
 *         the t highest - the plain mean of the bucket means where they agree, their median where they do not
 * A sample that is not finite spoils one bucket of K, not the pixel: K = 5, bucket means (0, 0, 0, 0, 10) give G = 0.8, t = 1 and
 * the result 0 (MON 0, the plain mean 2); (1, 1, 1, 1, 1) give t = 0.
 * Refusals leave the film exactly as it was.  spt_film_buckets: a null film, n_buckets even or outside 3 .. 15, a film that
 * already covers samples (done > 0) or already has buckets (SPT_ERR_INVALID_ARG); a box radius other than 0.5
 * (SPT_ERR_UNSUPPORTED); no memory (SPT_ERR_OUT_OF_MEMORY).  spt_film_read_buckets and spt_film_read_robust: a null film or out,
 * a film without buckets, an unknown estimator, spt_film_read_robust while done == 0 (SPT_ERR_INVALID_ARG).  A film without rows
 * returns SPT_OK and writes nothing.  Buckets go with any first_sample, shard layout, samples_per_pass, sampler, with and without
 * SPT_FILM_MOMENTS and SPT_RENDER_DEBUG_NORMAL.  All three calls take the scene's lock and are synchronous. */
/* Turns on K = n_buckets bucket sums.  Only while the film covers no sample (done == 0). */
spt_status spt_film_buckets(spt_film* film, uint32_t n_buckets);
/* [n_buckets][rows][width][3] f32: the bucket sums B_j, packed rows like spt_film_read. */
spt_status spt_film_read_buckets(spt_film* film, float* out);
enum { SPT_ROBUST_MON = 0, SPT_ROBUST_GMON = 1 };
/* rows * width * 3 f32 */
spt_status spt_film_read_robust(spt_film* film, uint32_t estimator, float* out);

/* ---- 8-bit read-out of a film (additive to ABI v14: detect it by symbol) -----------------------------------------------------
 * What RendererT::render saves is an 8-bit image (Film::filter_to_image -> color_to_rgb, src/core/film.rs:94-99).
 * spt_film_read_rgb8 makes the float image of `source` exactly as the matching float call does - SPT_READ_MEAN: spt_film_read
 * SPT_FILM_MEAN (adaptive counts and a box radius other than 0.5 included), SPT_READ_ROBUST_MON / _GMON: spt_film_read_robust,
 * SPT_READ_DENOISED: spt_film_denoise(film, guide, dn) - and returns its bytes, converted on the device in a pass of its own
 * behind the read-out kernel: a quarter of the bytes cross to the host.  Per channel, exact f32, one rounded operation at a time:
 *     c = x * 255.0f;   cl = c < 0 ? 0 : (c > 255 ? 255 : c);   byte = (cl != cl) ? 0 : (uint8_t)cl
 * A NaN gives 0, +inf 255, -inf and -0 give 0, the conversion truncates (no gamma, no dithering: the reference has none).
 * It changes nothing of the film: S, Q, buckets, mask and counts stay as they are.  Refusals are those of the matching float
 * call, with its status, and leave the film as it was; an unknown source or a null film or out is SPT_ERR_INVALID_ARG.  A film
 * without rows returns SPT_OK and writes nothing.  Synchronous; takes the scene's lock. */
enum { SPT_READ_MEAN = 0, SPT_READ_ROBUST_MON = 1, SPT_READ_ROBUST_GMON = 2, SPT_READ_DENOISED = 3 };
/* out: rows * width * 3 u8, packed.  guide / dn are read for SPT_READ_DENOISED only (both may be NULL, as in spt_film_denoise). */
spt_status spt_film_read_rgb8(spt_film* film, uint32_t source, spt_film* guide, const spt_denoise_params* dn, uint8_t* out);

/* Seams below the renderer, for parity tests of rows a4/a6/a8/a9/a10:
 * Primitive::intersect / intersect_test of the scene aggregate on caller rays. */
spt_status spt_trace_closest(const spt_scene* scene, uint32_t n, const spt_ray* rays, spt_hit* hits);
spt_status spt_trace_any(const spt_scene* scene, uint32_t n, const spt_ray* rays, uint8_t* occluded);

/* ---- radiance along caller-provided rays (additive to ABI v14: detect it by symbol) ---------------------------------------------
 * spt_radiance is the integrator without the camera: PathTracer::trace_ray (src/renderer/pt.rs:39-210) for rays the caller made,
 * under the scene's light sampler.  Everything the film calls compute per camera sample is computed here per ray, by the same
 * kernels from bounce 0 on; only the pinhole camera and the pixel grid are gone.
 * Per path: x(i, k) is trace_ray for the ray (o, d, t_min) of record i with the job's max_depth.  Its RNG starts at
 * spt_rng_seed(seed, stream_a, stream_b + k) (include/spt_detmath.h), advanced by rng_skip draws before the path starts (a camera
 * sample of the random sampler has drawn its two pixel offsets by then: rng_skip = 2).  Depth 0 is a camera ray's: emission and
 * the environment get weight 1, a miss adds 0 + (1 * env) * 1.  t_min holds for the first segment only (the integrator's own
 * epsilon after it); d is taken as it is, unit length is the caller's business.  max_depth == 0: every path is 0.
 * Per ray: out_i = ((0 + x(i, 0)) + x(i, 1) + ... + x(i, S - 1)) * (1.0f / (float)S) with S = repeats, added in k order, every
 * operation a rounded f32 operation, per channel.
 * Textures and glints: with `aux`, a scene that samples textures computes the differentials of the depth-0 hit from the ray's two
 * auxiliary rays, Intersection::calc_differential with (rx_o, rx_d, ry_o, ry_d); without it the first hit is textured as the
 * reference textures every later hit, without differentials.  Scenes that sample no texture never read `aux`.
 * hits_out[i] is what spt_trace_closest returns for (o, t_min, d, f32::MAX).
 * A ray's result depends on its own record and the job's scalar fields only: not on its place in the array, its neighbours,
 * rays_per_pass or how the call is cut into passes.
 * Pointers are host pointers by default; the rays go up through page-locked staging in two slots (the host checks and fills one
 * while the other is in flight) and the results come back when every pass has run.  With SPT_RADIANCE_DEVICE_POINTERS rays, aux,
 * rgb_out and hits_out are device memory on the scene's device (the base address of each is checked with hipPointerGetAttributes,
 * rays and aux for 16-byte, rgb_out and hits_out for 4-byte alignment; that each allocation holds n_rays records is the caller's
 * business, as with any pointer of this ABI): the caller has finished producing them before the call, the library has finished
 * writing when it returns.
 * Refusals write nothing and leave the scene usable.  SPT_ERR_INVALID_ARG: a null scene or job; null rays or rgb_out while
 * n_rays > 0; size below sizeof(spt_radiance_job); unknown flags; repeats == 0; a host ray whose o, d or t_min is not finite or
 * whose d is all zero (the message names the first such index); a device pointer that is not device memory of the scene's device
 * or not aligned as above.
 * SPT_ERR_UNSUPPORTED: max_depth > 255.  n_rays == 0 returns SPT_OK and does nothing.
 * Synchronous.  Takes the scene's lock, starts behind whatever an asynchronous spt_render left on the film stream, shares the
 * render workspace, and touches neither spt_render's film / out buffers nor any film.  Scenes with Bezier patches are served. */
typedef struct spt_path_ray {      /* 48 B */
    float o[3]; float t_min;       /* first segment only */
    float d[3]; uint32_t stream_a;
    uint32_t stream_b; uint32_t pad[3];
} spt_path_ray;
typedef struct spt_ray_aux {       /* 64 B: the two auxiliary rays of Intersection::calc_differential */
    float rx_o[3], pad0, rx_d[3], pad1, ry_o[3], pad2, ry_d[3], pad3;
} spt_ray_aux;
enum { SPT_RADIANCE_DEVICE_POINTERS = 1u };
typedef struct spt_radiance_job {
    uint32_t size, flags;          /* sizeof(spt_radiance_job) as the caller was compiled (the struct only grows at its tail); SPT_RADIANCE_* */
    uint64_t n_rays;
    const spt_path_ray* rays;
    const spt_ray_aux* aux;        /* NULL, or n_rays records */
    uint32_t repeats;              /* S >= 1 paths per ray */
    uint32_t max_depth;
    uint64_t seed;
    uint32_t rng_skip;             /* draws discarded from every stream before the path starts */
    uint32_t rays_per_pass;        /* tuning, 0 = default */
    float* rgb_out;                /* n_rays * 3 f32 */
    spt_hit* hits_out;             /* NULL, or n_rays records: the closest hit of each ray's first segment */
} spt_radiance_job;
spt_status spt_radiance(const spt_scene* scene, const spt_radiance_job* job);

/* ---- camera models (additive to ABI v14: detect it by symbol) ---------------------------------------------------------------------
 * spt_render_camera and spt_film_create_camera are spt_render and spt_film_create with a camera model in the camera's place.  With
 * SPT_CAMERA_PERSPECTIVE they ARE those two calls (same code path, same words); fields that do not belong to a type are ignored.
 * A film remembers its model, and every film call keeps its documented meaning on a film of any model.  The pixel offsets, the path's
 * RNG stream (seed, pixel, plan index) and the draws it has made before trace_ray starts are the pinhole plan's for every model.
 *
 * The models (include/spt_camera_models.h is this text as code; the kernel and spt_host_camera_rays of libspt_host.so include it).
 * All arithmetic is IEEE f32, one rounded operation at a time, no contraction, in the written order.  x, y are the screen point of
 * pt.rs:269-271 as spt_render computes it, hc = base.half_cot_half_fov, t_min = 0.0001f for every model.
 *   PERSPECTIVE   o = eye, d = normalize((forward*hc + right*x) + up*y): PerspectiveCamera::generate_ray.
 *   THIN_LENS     a pinhole behind a thin lens.
 *     Lens draws: u1, u2 are the first two draws of the stream spt_rng_seed(seed ^ SPT_CAMERA_SEED_SALT, pixel, plan_index), a
 *       stream of its own; the draws are made whatever the radius.
 *     Disk map:   a = 2*u1 - 1, b = 2*u2 - 1.  a == 0 && b == 0 gives lx = ly = 0.  |a| > |b| gives r = a, phi = (SPT_PI/4) * (b/a).
 *       Otherwise r = b, phi = SPT_PI/2 - (SPT_PI/4) * (a/b).  lx = r*spt_cos(phi), ly = r*spt_sin(phi).
 *     Ray:        ft = focus_distance / hc, made once on the host in f32.  du = (forward*hc + right*x) + up*y, the pinhole's.
 *       lo_k = (right_k*lx + up_k*ly) * lens_radius.  o = eye + lo.  d = normalize(du*ft - lo).
 *   ORTHOGRAPHIC  sx = x*view_height, sy = y*view_height.  o_k = eye_k + (right_k*sx + up_k*sy).  d = forward, as given.
 *   PANORAMA      equirectangular, in the environment map's own axes (environment.rs:128-133); it reads only base.eye.
 *     ph = (x * aspect_inv) * (2*SPT_PI), with aspect_inv = 1.0f/aspect made once.  th = (0.5f - y) * SPT_PI.  st = spt_sin(th).
 *     o = eye.  d = normalize((st*spt_sin(ph), spt_cos(th), st*spt_cos(ph))).  Row 0 starts at the +y pole and the image centre
 *     looks along +z.
 * normalize(v) = v / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z), a true division per component.  The vertical offset runs upward like the
 * pinhole's, so the offsets that filters and box read-outs re-derive stay valid.
 * Auxiliary rays (textured scenes): the same model at (x + aux_dx, y) and (x, y + aux_dy) with the same lens point.
 *
 * A non-perspective render takes the single-stream or the film-stream schedule; the pass pipeline, the eye-relative copy, block and
 * origin candidates, the screen bound and the row spans are derived from a pinhole eye and stay off for it.
 * Refusals for the three new types leave nothing changed.  SPT_ERR_INVALID_ARG: a null model, size below sizeof(spt_camera_model),
 * an unknown type, or a parameter of the type outside the ranges below.  SPT_ERR_UNSUPPORTED: SPT_RENDER_COUNT_VISITS;
 * SPT_RENDER_AOV_ALBEDO (the first-hit albedo kernels read the pinhole's compact records).
 * SPT_CAMERA_GENERAL=1 in the environment sends perspective renders through the camera-model kernel too (an A/B switch: same film). */
enum { SPT_CAMERA_PERSPECTIVE = 0, SPT_CAMERA_THIN_LENS = 1, SPT_CAMERA_ORTHOGRAPHIC = 2, SPT_CAMERA_PANORAMA = 3 };
#define SPT_CAMERA_SEED_SALT 0x4C454E5343414D31ull
typedef struct spt_camera_model {
    uint32_t size;          /* sizeof as the caller was compiled; grows at the tail only */
    uint32_t type;          /* SPT_CAMERA_* */
    spt_camera base;        /* eye, forward, up, right, half_cot_half_fov: as spt_render takes them */
    float lens_radius;      /* THIN_LENS: finite, >= 0 */
    float focus_distance;   /* THIN_LENS: finite, > 0, along base.forward from the eye */
    float view_height;      /* ORTHOGRAPHIC: finite, > 0, world units the image is high */
    uint32_t pad;
} spt_camera_model;
spt_status spt_render_camera(const spt_scene* scene, const spt_camera_model* model, const spt_render_params* params, float* rgb_mean_out,
                             spt_render_stats* stats /* may be NULL */);
spt_status spt_film_create_camera(const spt_scene* scene, const spt_camera_model* model, const spt_render_params* params,
                                  uint32_t first_sample, uint32_t film_flags, spt_film** out);

/* ---- irradiance at surface points (additive to ABI v14: detect it by symbol) ------------------------------------------------------
 * spt_bake returns, per point of a list of points on the scene's surfaces, the radiance a white Lambert surface would emit there:
 * E / pi, so irradiance is pi times it.  The gather rays are made on the device, where the authoritative triangle records live
 * (spt_scene_update, spt_scene_deform and spt_scene_deform_vertices move them without the host's copy).  include/spt_bake.h is this
 * text as code: SPT_HD functions the kernel and spt_host_bake_rays of libspt_host.so both include.  All arithmetic is IEEE f32, one
 * rounded operation at a time, in the written order, no contraction.
 *
 * Points.  SURFACE points are named the way spt_hit names a hit, so the hits_out of spt_radiance / spt_trace_closest can be fed
 * straight back in: `instance` indexes the scene's current instance array (the order of the last update) and must be a SPT_PRIM_MESH
 * instance; `prim` is the absolute triangle index as spt_hit::prim reports it and must lie in that mesh's [tri_first, tri_first +
 * tri_count); v and w must be finite and are not range-checked (extrapolation is the caller's business).  The point is resolved as
 *   u = (1.0f - v) - w;  object position (p0*u + p1*v) + p2*w, taken to the world by `fwd` as a point: ((c0*x + c1*y) + c2*z) + t;
 *   normal exactly as a hit's is rebuilt: object n = normalize((n0*u + n1*v) + n2*w), world normalize((nrm0*n.x + nrm1*n.y) + nrm2*n.z).
 * WORLD points give p and n as they are (unit length is the caller's business, as with spt_path_ray::d); both must be finite and n
 * not all zero.  They serve spheres, patches and free-standing probes.  SPT_BAKE_FLIP negates every normal after it is resolved.
 * spt_bake_point_ok / spt_bake_world_ok (spt_bake.h) state validity; the host refuses a call with them, the kernel uses them so that
 * a bad record arriving through device pointers never indexes anything: such a point's result is the quiet NaN 0x7fc00000 in all
 * three channels and its neighbours are unaffected.
 *
 * Per point i and sample k in [0, S): a = first_point + i (u32 wrap), b = first_sample + k.
 *   Direction: rx, ry are the first two draws of spt_rng_seed(seed ^ SPT_BAKE_SEED_SALT, a, b), a stream of their own.  The cosine
 *     map is the Lambert lobe's: phi = rx * 2.0f * SPT_PI, spt_sincos, st = spt_sqrt(ry), ct = spt_sqrt(1.0f - ry), local
 *     (st*cp, st*sp, ct).  The frame is sphere_frame(n) (sphere.rs:70-82): s = spt_sqrt(1.0f - n.y*n.y); s != 0: bitangent =
 *     n * (-n.y / s) with its y replaced by s, tangent = cross(bitangent, n); else n.y > 0: bitangent (1,0,0), tangent (0,0,1); else
 *     bitangent (-1,0,0), tangent (0,0,-1).  d = normalize((tangent*lx + bitangent*ly) + n*lz), normalize with true divisions.
 *   Gather ray: o = p, t_min = 0.0001f / spt_max(ct, 0.00001f) (the integrator's own epsilon for a bounce ray), direction d, path
 *     stream (a, b), no draws skipped.
 *   x(i, k) is what spt_radiance returns for exactly that record with repeats = 1, rng_skip = 0, no aux and the job's seed and
 *     max_depth: depth 0 is a camera ray's (emission and the environment get weight 1), a textured first hit is textured without
 *     differentials, the path starts outside any medium.
 * Per point, once, the delta lights: D = 0; for l = 0 .. n_lights - 1 in array order, types directional, point and spot only:
 *   dir, strength, dist are the three delta cases of the light sampler at position p (directional: -dir, strength, f32::MAX; point:
 *   sv = pos - p, dist = sqrt(dot(sv, sv)), sv / dist, strength * (1.0f / dot(sv, sv)); spot: the same with strength * atten,
 *   atten = clamp((dot(dir_l, -(sv / dist)) - cos_outer) / max(cos_inner - cos_outer, 0.0001f), 0, 1)).  c = dot(n, dir); skipped
 *   unless c > 0.  li = (strength * SPT_FRAC_1_PI) * c; skipped when all three channels are 0.  The shadow ray is (p, dir, t_min =
 *   0.0001f / spt_max(c, 0.00001f), t_max = dist - 0.001f), judged as spt_trace_any judges it; unoccluded: D = D + li.
 *   A deterministic sum: no light sampling, no MIS.  Area lights and the environment are found by the gather rays with weight 1 and
 *   delta lights cannot be hit, so nothing is counted twice.
 * Result: out_i = D + (((0 + x(i,0)) + x(i,1)) + ... + x(i,S-1)) * (1.0f / (float)S), per channel, in k order.  max_depth == 0 gives
 * D.  A point's result depends on its own record, on first_point + i and on the job's scalars only: not on its neighbours, on
 * points_per_pass or on how samples are cut into chunks.  first_point lets a caller cut one list over calls or devices and get the
 * same words; first_sample lets a caller add samples later and average them itself.
 *
 * Pointers, staging, the lock, the shared render workspace and scenes with Bezier patches: as spt_radiance.  With
 * SPT_BAKE_DEVICE_POINTERS points (16-byte aligned) and rgb_out (4-byte aligned) are device memory on the scene's device.
 * Refusals write nothing and leave the scene usable.  SPT_ERR_INVALID_ARG: a null scene or job; size below sizeof(spt_bake_job);
 * unknown flags or kind; samples == 0; null points or rgb_out while n_points > 0; a host point that fails the predicate or is not
 * finite (the message names the first such index); a device pointer that is not device memory of the scene's device or misaligned.
 * SPT_ERR_UNSUPPORTED: max_depth > 255.  n_points == 0 returns SPT_OK and does nothing. */
typedef struct spt_bake_point { uint32_t instance, prim; float v, w; } spt_bake_point;              /* 16 B: spt_hit without t */
typedef struct spt_bake_world_point { float p[3], pad0, n[3], pad1; } spt_bake_world_point;         /* 32 B */
enum { SPT_BAKE_POINTS_SURFACE = 0, SPT_BAKE_POINTS_WORLD = 1 };
enum { SPT_BAKE_DEVICE_POINTERS = 1u, SPT_BAKE_FLIP = 2u };
#define SPT_BAKE_SEED_SALT 0x42414B45504F4E54ull   /* "BAKEPONT": distinct from SPT_CAMERA_SEED_SALT */
typedef struct spt_bake_job {
    uint32_t size, flags;          /* sizeof(spt_bake_job) as the caller was compiled (the struct only grows at its tail); SPT_BAKE_* flags */
    uint32_t kind, pad;            /* SPT_BAKE_POINTS_* */
    uint64_t n_points;
    const void* points;            /* n_points spt_bake_point or spt_bake_world_point */
    float* rgb_out;                /* n_points * 3 f32 */
    uint32_t samples, max_depth;   /* S >= 1 gather paths per point */
    uint64_t seed;
    uint32_t first_point, first_sample;
    uint32_t points_per_pass, pad1;   /* tuning, 0 = default */
} spt_bake_job;
spt_status spt_bake(const spt_scene* scene, const spt_bake_job* job);

/* ---- spherical-harmonic light probes (additive to ABI v14: detect it by symbol) --------------------------------------------------
 * spt_probe returns, per free point in space, the incident radiance there projected onto the nine real spherical harmonics of bands
 * 0 .. 2, per colour channel, and (optionally) a visibility record that tells a probe buried in geometry from a free one.  The gather
 * rays are made on the device.  include/spt_probe.h is this text as code: functions the kernels and spt_host_probe_rays of
 * libspt_host.so both include.  All arithmetic is IEEE f32, one rounded operation at a time, in the written order, no contraction.
 *
 * A probe is spt_probe_point {p, pad}; it is valid iff p is finite (spt_probe_ok).  The host refuses a host-side list with an invalid
 * probe (the message names the first such index); an invalid probe that arrives through device pointers indexes nothing, all its
 * outputs (27 words of sh_out, 4 of aux_out) are the quiet NaN 0x7fc00000 and its neighbours are unaffected.
 *
 * Per probe i and sample k in [0, S): a = first_point + i (u32 wrap), b = first_sample + k.
 *   Direction: rx, ry are the first two draws of spt_rng_seed(seed ^ SPT_PROBE_SEED_SALT, a, b), a stream of their own.  The uniform
 *     sphere map: z = 1.0f - 2.0f*rx; r = spt_sqrt(spt_max(0.0f, 1.0f - z*z)); phi = ry * 2.0f * SPT_PI; spt_sincos(phi, &sp, &cp);
 *     d = normalize(r*cp, r*sp, z), normalize with true divisions (spt_cm_normalize).
 *   Gather ray: o = p, t_min = 0.0001f (SPT_BAKE_T_EPS), direction d, path stream (a, b) under the job's seed, no draws skipped.
 *   x(i, k) is what spt_radiance returns for exactly that record with repeats = 1, rng_skip = 0, no aux and the job's seed and
 *     max_depth: depth 0 is a camera ray's, the path starts outside any medium.
 * Basis spt_probe_basis(d, Y): real orthonormal SH without the Condon-Shortley sign, index j = l(l+1)+m, world axes as given, d =
 *   (x, y, z):  Y0 = 0.282094792f;  Y1 = 0.488602512f*y;  Y2 = 0.488602512f*z;  Y3 = 0.488602512f*x;  Y4 = 1.092548431f*(x*y);
 *   Y5 = 1.092548431f*(y*z);  Y6 = 0.315391565f*(3.0f*(z*z) - 1.0f);  Y7 = 1.092548431f*(x*z);  Y8 = 0.546274215f*(x*x - y*y).
 * Per probe, once, the delta lights (no gather ray can find them): D[j][c] = 0; for l = 0 .. n_lights - 1 in array order, types
 *   directional, point and spot only: dir, strength, dist are the three delta cases of the light sampler at p, exactly as for spt_bake;
 *   li = strength (no cosine, no 1/pi); a light whose three channels are all 0 is skipped.  The shadow ray is (p, dir, t_min =
 *   0.0001f, t_max = dist - 0.001f), judged as spt_trace_any judges it; unoccluded: D[j][c] = D[j][c] + li[c] * Y_j(dir).
 * Result: sh[j][c] = D[j][c] + (((0 + x_c(i,0)*Y_j(d_0)) + x_c(i,1)*Y_j(d_1)) + ...) * w, w = (4.0f*SPT_PI) * (1.0f/(float)S) made
 *   once on the host, the sum in k order.  max_depth == 0 gives D.  sh_out holds 27 f32 per probe, coefficient-major [9][3], RGB
 *   innermost.
 * Visibility record aux[4], over the first segments of the S gather rays (traced whatever max_depth is), inv = 1.0f/(float)S:
 *   aux[0] = (float)hits * inv;  aux[1] = (float)backfacing * inv: a hit on a SPT_PRIM_MESH instance is backfacing iff
 *   (n0*d0 + n1*d1) + n2*d2 > 0 with n the normal spt_bake_resolve gives for the hit's (instance, prim, v, w); sphere and patch hits
 *   count as front;  aux[2] = the sum of the hit distances in k order divided by (float)hits, 0 without a hit;  aux[3] = the smallest
 *   hit distance, SPT_F32_MAX without one.
 * A probe's words depend on its record, on first_point + i and on the job's scalars only: not on its neighbours, on points_per_pass
 * or on how samples are cut into chunks.
 *
 * Pointers, staging, the lock, the shared render workspace and scenes with Bezier patches: as spt_bake.  With
 * SPT_PROBE_DEVICE_POINTERS points (16-byte aligned), sh_out and aux_out (4-byte aligned) are device memory on the scene's device.
 * Refusals write nothing and leave the scene usable.  SPT_ERR_INVALID_ARG: a null scene or job; size below sizeof(spt_probe_job);
 * unknown flags; samples == 0; null points or sh_out while n_points > 0; an invalid host probe; a device pointer that is not device
 * memory of the scene's device or misaligned.  SPT_ERR_UNSUPPORTED: max_depth > 255.  n_points == 0 returns SPT_OK and does nothing. */
typedef struct spt_probe_point { float p[3]; float pad; } spt_probe_point;   /* 16 B */
enum { SPT_PROBE_DEVICE_POINTERS = 1u };
#define SPT_PROBE_SEED_SALT 0x50524F4245534831ull   /* "PROBESH1": distinct from SPT_BAKE_SEED_SALT and SPT_CAMERA_SEED_SALT */
typedef struct spt_probe_job {
    uint32_t size, flags;          /* sizeof(spt_probe_job) as the caller was compiled (the struct only grows at its tail); SPT_PROBE_* flags */
    uint64_t n_points;
    const spt_probe_point* points;
    float* sh_out;                 /* n_points * 27 f32 */
    float* aux_out;                /* NULL, or n_points * 4 f32 */
    uint32_t samples, max_depth;   /* S >= 1 gather paths per probe */
    uint64_t seed;
    uint32_t first_point, first_sample;
    uint32_t points_per_pass, pad;   /* tuning, 0 = default */
} spt_probe_job;
spt_status spt_probe(const spt_scene* scene, const spt_probe_job* job);

/* ---- first-hit surface records along caller rays (additive to ABI v14: detect it by symbol) --------------------------------------
 * spt_gbuffer returns, per caller ray, the surface the ray sees first: where, which, its normal and its albedo.  It is what lies
 * between spt_trace_closest and a path trace: the shading inputs of the integrator's depth-0 vertex, without a path.
 * All arithmetic is IEEE f32, one rounded operation at a time, in the written order, no contraction.
 * Hit.     (t, instance, prim, v, w) are word for word what spt_trace_closest returns for (o, t_min, d, f32::MAX): the hits_out
 *          of spt_radiance.
 * Miss.    t = f32::MAX, instance = prim = -1, every other word +0.
 * p        p_k = o_k + d_k * t: the point the integrator shades from.
 * n        the world-space interpolated normal of the hit as the integrator rebuilds it (what SPT_RENDER_DEBUG_NORMAL shows before
 *          its * 0.5 + 0.5).  No normal map enters, for spheres, patches and meshes alike; for a mesh it is the normal
 *          spt_bake_resolve gives for the hit.
 * albedo   the rule of SPT_RENDER_AOV_ALBEDO on the material record evaluated at the hit (per-hit recipes and P-NDF fallbacks as
 *          there; emission and the normal map do not enter).  With `aux`, a scene that samples textures computes the texture
 *          footprint from the ray's two auxiliary rays, Intersection::calc_differential with (rx_o, rx_d, ry_o, ry_d), as
 *          spt_radiance does for its depth-0 hit; without it the differentials are 0.  Scenes that sample no texture never read
 *          `aux`.
 * surface  the instance's `surface` index.
 * flags    SPT_GBUF_BACKFACING iff (n0*d0 + n1*d1) + n2*d2 > 0;  SPT_GBUF_LIGHT iff the instance's light >= 0;  bits 8..15 the
 *          instance's prim_type.
 * A record depends on its own ray (and its aux record) and on the scene only: not on its place in the array, its neighbours,
 * rays_per_pass or how the call is cut into passes.  Nothing is random: stream_a / stream_b of the rays are ignored.
 * Pointers, staging, the checks of host rays, the lock, the shared render workspace and scenes with Bezier patches: as
 * spt_radiance.  With SPT_GBUFFER_DEVICE_POINTERS rays, aux and out are device memory on the scene's device, each 16-byte aligned.
 * Refusals write nothing and leave the scene usable.  SPT_ERR_INVALID_ARG: a null scene or job; null rays or out while n_rays > 0;
 * size below sizeof(spt_gbuffer_job); unknown flags; a host ray whose o, d or t_min is not finite or whose d is all zero (the
 * message names the first such index); a device pointer that is not device memory of the scene's device or misaligned.
 * SPT_ERR_UNSUPPORTED: more than 2^40 rays.  n_rays == 0 returns SPT_OK and does nothing.
 * Synchronous.  It reads the scene's current records, so it follows spt_scene_update, spt_scene_deform and
 * spt_scene_deform_vertices like the other ray entries, and touches no film. */
enum { SPT_GBUFFER_DEVICE_POINTERS = 1u };
enum { SPT_GBUF_BACKFACING = 1u, SPT_GBUF_LIGHT = 2u };   /* spt_gbuffer_rec::flags; bits 8..15: the instance's prim_type */
typedef struct spt_gbuffer_rec {      /* 64 B: four 16-byte words */
    float p[3];      float t;         /* world hit point; t = f32::MAX on a miss */
    float n[3];      int32_t instance;/* -1 on a miss */
    float albedo[3]; int32_t prim;    /* -1 on a miss */
    float v, w;      uint32_t surface; uint32_t flags;
} spt_gbuffer_rec;
typedef struct spt_gbuffer_job {
    uint32_t size, flags;             /* sizeof(spt_gbuffer_job) as the caller was compiled (the struct only grows at its tail); SPT_GBUFFER_* */
    uint64_t n_rays;
    const spt_path_ray* rays;         /* spt_radiance's records; stream_a / stream_b are ignored */
    const spt_ray_aux* aux;           /* NULL, or one per ray: texture footprints, as spt_radiance takes them */
    uint32_t rays_per_pass, pad;      /* tuning, 0 = default */
    spt_gbuffer_rec* out;             /* n_rays records */
} spt_gbuffer_job;
spt_status spt_gbuffer(const spt_scene* scene, const spt_gbuffer_job* job);

/* ---- visibility along caller rays and at surface points (additive to ABI v14: detect them by symbol) -----------------------------
 * The any-hit siblings of spt_gbuffer and spt_bake.  All arithmetic is IEEE f32, one rounded operation at a time, in the written
 * order, no contraction.
 *
 * spt_occluded: whether anything lies on the segment (o, t_min, d, t_max) of each caller ray.
 * Result.  Byte i is word for word what spt_trace_any returns for record i: 1 occluded, 0 not.  With SPT_OCCLUDED_PACKED `out` is
 *          ceil(n_rays / 64) u64 words instead: ray i is bit i & 63 of word i >> 6, and the bits past n_rays in the last word are 0.
 *          A result depends on its own record and the scene only: not on its place, its neighbours, rays_per_pass or the cut into
 *          passes (with PACKED the pass size is rounded up to a multiple of 64).
 * Pointers.  Host pointers by default: the rays go through spt_radiance's two page-locked staging slots and are checked while they
 *          are copied.  With SPT_OCCLUDED_DEVICE_POINTERS rays (16-byte aligned) and out (any alignment; PACKED: 8-byte aligned) are
 *          device memory on the scene's device; device records are not checked.
 * Refusals write nothing and leave the scene usable.  SPT_ERR_INVALID_ARG: a null scene or job; null rays or out while n_rays > 0;
 *          size below sizeof(spt_occluded_job); unknown flags; a host ray whose o, d or t_min is not finite, whose d is all zero or
 *          whose t_max is NaN (the message names the first such index); a device pointer that is not device memory of the scene's
 *          device or misaligned.  SPT_ERR_UNSUPPORTED: more than 2^40 rays.  n_rays == 0 returns SPT_OK and does nothing.
 *
 * spt_ao: cosine-weighted ambient occlusion and the bent normal at the points spt_bake takes.
 * Points.  spt_bake's: resolved, validated and flipped exactly as there (spt_bake_point_ok / spt_bake_world_ok, spt_bake_resolve,
 *          SPT_AO_FLIP = SPT_BAKE_FLIP; include/spt_bake.h).
 * Rays.    For point i and sample k, a = first_point + i (u32 wrap), b = first_sample + k: spt_bake's gather ray, spt_bake_frame then
 *          spt_bake_sample(seed, a, b, ...) - the same salt, direction and t_min - with t_max = max_distance when that is finite, else
 *          f32::MAX, judged as spt_trace_any judges (p, t_min, d, t_max).  They are the first segments of the bake with the same
 *          (seed, first_point, first_sample): spt_host_bake_rays returns them.
 * Record.  count = the samples that are not occluded; sum = ((0 + d_k1) + d_k2) + ... over those samples in k order, per component;
 *          open = (float)count * (1.0f / (float)samples): the directions are cosine-distributed, so this is the cosine-weighted
 *          openness; bent = sum / sqrt((sum.x*sum.x + sum.y*sum.y) + sum.z*sum.z) (spt_cm_normalize) when count > 0 and sum is not
 *          all zero, else (0, 0, 0).  sum and count let a caller join calls cut by first_sample.
 *          A record depends on its point, first_point + i and the job's scalars only: not on its neighbours, points_per_pass or
 *          how the samples are cut into launches.
 * Invalid. Behind device pointers a point that fails the predicate indexes nothing: its seven float words are 0x7fc00000
 *          (SPT_BAKE_NAN_BITS), its count is 0xffffffff, and its neighbours are unaffected.  A host list with such a point is
 *          refused; the message names the first such index.
 * Pointers, staging, lock and ordering as spt_bake; with SPT_AO_DEVICE_POINTERS points and out are each 16-byte aligned.
 * Refusals.  SPT_ERR_INVALID_ARG: a null scene or job; null points or out while n_points > 0; size below sizeof(spt_ao_job);
 *          unknown flags or kind; samples == 0 or > 2^24; max_distance NaN or <= 0; a bad device pointer; an invalid host point.
 *          SPT_ERR_UNSUPPORTED: more than 2^40 points.  n_points == 0 returns SPT_OK and does nothing.
 *
 * Both are synchronous, take the scene's lock, start behind the film stream, read the scene's current records (so they follow
 * spt_scene_update, spt_scene_deform and spt_scene_deform_vertices), touch no film and none of spt_render's buffers: they need no
 * path queue and no radiance slot.  Scenes with Bezier patches are forwarded like the other ray entries. */
enum { SPT_OCCLUDED_DEVICE_POINTERS = 1u, SPT_OCCLUDED_PACKED = 2u };
typedef struct spt_occluded_job {
    uint32_t size, flags;             /* sizeof(spt_occluded_job) as the caller was compiled (the struct only grows at its tail); SPT_OCCLUDED_* */
    uint64_t n_rays;
    const spt_ray* rays;              /* o, t_min, d, t_max: spt_trace_any's records */
    void* out;                        /* n_rays u8 (1 occluded, 0 not); PACKED: ceil(n_rays / 64) u64 */
    uint32_t rays_per_pass, pad;      /* tuning, 0 = default */
} spt_occluded_job;
spt_status spt_occluded(const spt_scene* scene, const spt_occluded_job* job);

enum { SPT_AO_DEVICE_POINTERS = 1u, SPT_AO_FLIP = 2u };
typedef struct spt_ao_rec { float sum[3]; float open; float bent[3]; uint32_t count; } spt_ao_rec;   /* 32 B: two 16-byte words */
typedef struct spt_ao_job {
    uint32_t size, flags;             /* sizeof(spt_ao_job) as the caller was compiled (the struct only grows at its tail); SPT_AO_* */
    uint32_t kind, pad;               /* SPT_BAKE_POINTS_SURFACE / SPT_BAKE_POINTS_WORLD */
    uint64_t n_points;
    const void* points;               /* spt_bake_point / spt_bake_world_point */
    spt_ao_rec* out;                  /* n_points records */
    uint32_t samples;                 /* S in 1 .. 2^24 */
    float max_distance;               /* > 0, +inf allowed */
    uint64_t seed;
    uint32_t first_point, first_sample;
    uint32_t points_per_pass, pad1;   /* tuning, 0 = default */
} spt_ao_job;
spt_status spt_ao(const spt_scene* scene, const spt_ao_job* job);

/* ---- camera rays and first-hit images made on the device (additive to ABI v14: detect them by symbol) ----------------------------
 * The rays of a camera model's plan without the host in the loop, and the first-hit images of such a plan.  All arithmetic is IEEE
 * f32, one rounded operation at a time, in the written order, no contraction.
 *
 * spt_camera_rays: the rays spt_host_camera_rays of libspt_host.so makes, made by a kernel.
 * Result.  rays is [count][height][width] and aux, when given, as many: every word of both is the word
 *          spt_host_camera_rays(model, plan, first, count, rays, aux) writes - the model's ray ("camera models" above, any type,
 *          SPT_CAMERA_PERSPECTIVE included) at the plan's pixel offset of plan sample first + k, t_min = 0.0001f, stream_a = the
 *          pixel index row * width + column, stream_b = the plan index, every padding word +0.  Of the plan it reads what that
 *          call reads: width, height, spp, sampler, division_x, division_y, seed.  The words do not depend on rays_per_pass.
 * Scene.   It names the device, the stream and the lock, and is taken as spt_gbuffer takes it; no geometry is read.
 * Pointers.  Host pointers by default: the rays are made in the shared workspace pass by pass and copied out.  With
 *          SPT_CAMERA_RAYS_DEVICE_POINTERS rays and aux are device memory on the scene's device, each 16-byte aligned, checked as
 *          spt_gbuffer checks its pointers.
 * Refusals write nothing.  SPT_ERR_INVALID_ARG: a null scene or job; size below sizeof(spt_camera_rays_job); unknown flags; null
 *          rays while count > 0; whatever spt_host_camera_rays refuses - a null plan, a model that fails spt_cm_check, width, height
 *          or spp of 0, an unknown sampler, first + count > spp, a jittered sampler with a division of 0; a bad device pointer.
 *          SPT_ERR_UNSUPPORTED: more than 2^40 rays, or an image of more than 2^31 pixels.  count == 0 returns SPT_OK and does
 *          nothing.
 *
 * spt_camera_gbuffer: the first-hit images of the plan samples first .. first + count - 1 of a model.  Per pixel:
 *          A = N = (+0, +0, +0), T = +0, K = 0;
 *          for s = first .. first + count - 1, in that order, with r the spt_gbuffer_rec of the ray spt_camera_rays makes for
 *          (pixel, s) - with its aux record on a scene that samples textures -: A += r.albedo and N += r.n per component (a miss
 *          adds +0), and on a hit T += r.t and K += 1;
 *          inv = 1.0f / (float)count;  albedo = A * inv;  normal = N * inv;  depth = K > 0 ? T / (float)K : +0;
 *          coverage = (float)K / (float)count.
 *          albedo and normal are [height][width][3], depth and coverage [height][width]; a NULL image is not made.  An image does
 *          not depend on rays_per_pass or on how the call is cut into passes.
 * Pointers.  Host pointers by default; with SPT_CAMERA_GBUFFER_DEVICE_POINTERS the images are device memory on the scene's device,
 *          4-byte aligned.
 * Refusals write nothing.  SPT_ERR_INVALID_ARG: all four images NULL; count == 0; everything else as spt_camera_rays, likewise
 *          SPT_ERR_UNSUPPORTED.
 *
 * Both are synchronous, take the scene's lock, start behind the film stream and share the render workspace.  spt_camera_gbuffer reads
 * the scene's current records (so it follows spt_scene_update, spt_scene_deform and spt_scene_deform_vertices) and touches no film.
 * Scenes with Bezier patches are forwarded like the other ray entries. */
enum { SPT_CAMERA_RAYS_DEVICE_POINTERS = 1u };
typedef struct spt_camera_rays_job {
    uint32_t size, flags;              /* sizeof(spt_camera_rays_job) as the caller was compiled (the struct only grows at its tail); SPT_CAMERA_RAYS_* */
    const spt_camera_model* model;
    const spt_render_params* plan;
    uint32_t first, count;             /* plan samples [first, first + count) */
    spt_path_ray* rays;                /* [count][height][width] */
    spt_ray_aux* aux;                  /* NULL, or as many */
    uint32_t rays_per_pass, pad;       /* tuning, 0 = default */
} spt_camera_rays_job;
spt_status spt_camera_rays(const spt_scene* scene, const spt_camera_rays_job* job);

enum { SPT_CAMERA_GBUFFER_DEVICE_POINTERS = 1u };
typedef struct spt_camera_gbuffer_job {
    uint32_t size, flags;              /* sizeof(spt_camera_gbuffer_job) as the caller was compiled (the struct only grows at its tail); SPT_CAMERA_GBUFFER_* */
    const spt_camera_model* model;
    const spt_render_params* plan;
    uint32_t first, count;             /* plan samples [first, first + count); count >= 1 */
    float* albedo;                     /* [height][width][3] or NULL */
    float* normal;                     /* [height][width][3] or NULL */
    float* depth;                      /* [height][width] or NULL */
    float* coverage;                   /* [height][width] or NULL */
    uint32_t rays_per_pass, pad;       /* tuning, 0 = default */
} spt_camera_gbuffer_job;
spt_status spt_camera_gbuffer(const spt_scene* scene, const spt_camera_gbuffer_job* job);

/* ---- all hits along caller rays (additive to ABI v14: detect it by symbol) --------------------------------------------------------
 * spt_hits returns, per caller segment (o, t_min, d, t_max), the K nearest surfaces the segment crosses and how many it crosses in
 * all: what lies behind the first hit.  spt_trace_closest / spt_gbuffer answer "which surface first", spt_trace_any / spt_occluded
 * "any at all"; this is the third standard query, all hits.
 * Crossing.  A crossing of ray i is a primitive of an instance whose test succeeds with t_min < t && t < t_max.  All arithmetic is
 *          IEEE f32, one rounded operation at a time, in the written order, no contraction, and is what the closest-hit walk does:
 *          the ray goes into the instance's object space with `inv` (o as a point, d as a vector, not renormalised, so t is shared
 *          between the spaces); a triangle is tested as Triangle::intersect_ray tests it on the stored p0, p1 - p0, p2 - p0; a
 *          sphere gives the two roots mn = (-b - sqrt(delta)) / a and mx = (-b + sqrt(delta)) / a of Sphere::intersect_ray when
 *          delta >= 0.
 *          Triangle: (t, v, w) are the words of that test, prim is the absolute triangle index (spt_hit::prim), and
 *          SPT_HIT_BACKFACING is set iff det = e1 . (d x e2) < 0: the ray leaves through the object-space face e1 x e2.
 *          Sphere: up to TWO crossings, the root mn (front) and the root mx (SPT_HIT_BACKFACING), each judged on its own; prim is
 *          the sphere index and v = w = +0.
 *          Bits 8..15 of flags hold the instance's prim_type, as in spt_gbuffer_rec::flags.
 * Result.  Record j of ray i (hits[i * max_hits + j]) is its j-th crossing in ascending order of the key (t, instance, prim,
 *          backfacing).  Records past the last crossing are the miss record: t = f32::MAX, instance = prim = -1, every other word 0.
 *          Without SPT_HITS_COUNT_ALL counts[i].total is the number of records written (<= max_hits) and `back` counts the
 *          back-facing ones among them; the walk may cull behind the K-th key.  With SPT_HITS_COUNT_ALL total and back count EVERY
 *          crossing of the segment, and the records are the same K nearest, word for word.  max_hits == 0 (COUNT_ALL only) gives the
 *          counters alone; hits may then be null.
 * Consequences.
 *          Record 0 is spt_trace_closest's hit for the same spt_ray record, word for word, whenever that call reports a hit.  The one
 *          exception is a sphere root exactly equal to t_min: the closest-hit rule t = (mn < t_min) ? mx : mn; t_min < t loses the far
 *          root when mn == t_min, and this call reports it.
 *          On a scene without spheres, total > 0 under COUNT_ALL is spt_trace_any's byte.  For spheres it is not: spt_trace_any
 *          calls a segment that lies inside a sphere occluded (mn < t_max && mx > t_min), and this call reports no crossing there.
 *          A ray through an edge shared by two triangles crosses both: both records appear, with equal t, ordered by prim.
 *          back > total - back under COUNT_ALL along any ray from a point says the point is enclosed, for closed meshes whose faces
 *          point outward and for spheres.
 *          A result depends on its own record and the scene only: not on its place, its neighbours, rays_per_pass or the cut into
 *          passes; nor on the tree or the order the walk visits it in, since the K nearest are the K smallest keys.
 * Pointers, staging, checks, lock and ordering as spt_occluded.  Host pointers by default: the rays go through the two page-locked
 *          staging slots and are checked while they are copied; the results of the whole call are kept on the device and copied out
 *          behind the last pass.  A staged pass is sized so that its max_hits * 32 + 8 result bytes per ray fit the 32 MiB a default
 *          slot holds (2^20 rays, fewer as max_hits grows; rays_per_pass overrides it).  With SPT_HITS_DEVICE_POINTERS rays, hits and
 *          counts are device memory on the scene's device, 16-, 16- and 8-byte aligned, and the records are not checked.
 *          Synchronous; takes the scene's lock; starts behind the film stream; reads the scene's current records (so it follows
 *          spt_scene_update, spt_scene_deform and spt_scene_deform_vertices); touches no film and none of spt_render's buffers.
 * Refusals write nothing and leave the scene usable.  SPT_ERR_INVALID_ARG: a null scene or job; size below sizeof(spt_hits_job);
 *          unknown flags; max_hits > 64; max_hits == 0 without SPT_HITS_COUNT_ALL; null rays or counts while n_rays > 0; null hits
 *          while n_rays > 0 and max_hits > 0; a host ray whose o, d or t_min is not finite, whose d is all zero or whose t_max is NaN
 *          (the message names the first such index); a device pointer that is not device memory of the scene's device or
 *          misaligned.  SPT_ERR_UNSUPPORTED: more than 2^40 rays; a scene with Bezier-patch instances, Catmull-Clark surfaces
 *          included - the patch test yields one root by construction, so "all crossings" has no meaning there, and the call is
 *          not forwarded to libspt_hip_bez.so.  n_rays == 0 returns SPT_OK and does nothing. */
enum { SPT_HITS_DEVICE_POINTERS = 1u, SPT_HITS_COUNT_ALL = 2u };
enum { SPT_HIT_BACKFACING = 1u };     /* spt_hit_rec::flags; bits 8..15: the instance's prim_type, as in spt_gbuffer */
typedef struct spt_hit_rec {          /* 32 B: two 16-byte words */
    float t; int32_t instance; int32_t prim; uint32_t flags;
    float v, w; uint32_t pad[2];      /* pad = 0 */
} spt_hit_rec;
typedef struct spt_hit_count { uint32_t total, back; } spt_hit_count;
typedef struct spt_hits_job {
    uint32_t size, flags;             /* sizeof(spt_hits_job) as the caller was compiled (the struct only grows at its tail); SPT_HITS_* */
    uint64_t n_rays;
    const spt_ray* rays;              /* o, t_min, d, t_max */
    spt_hit_rec* hits;                /* n_rays * max_hits records, ray-major; may be null when max_hits == 0 */
    spt_hit_count* counts;            /* n_rays */
    uint32_t max_hits;                /* K in 0 .. 64; 0 only with SPT_HITS_COUNT_ALL */
    uint32_t rays_per_pass;           /* tuning, 0 = default */
} spt_hits_job;
spt_status spt_hits(const spt_scene* scene, const spt_hits_job* job);

/* Page-locked host memory for rgb_mean_out: lets the final device-to-host copy of the film run as one
 * DMA at PCIe rate instead of being staged through the runtime's bounce buffers.  Optional: any host
 * pointer is accepted by spt_render. */
spt_status spt_alloc_pinned(uint64_t bytes, void** out);
void spt_free_pinned(void* p);
/* page-lock / unlock caller memory (e.g. a shared-memory film mapped by every rank) so that spt_render's copy-out
 * into it runs at DMA speed */
spt_status spt_pin_host(void* p, uint64_t bytes);
void spt_unpin_host(void* p);

/* Test seam: evaluates one function of include/spt_detmath.h on the device (fn: 0 sin, 1 cos,
 * 2 log, 3 exp, 4 acos, 5 atan2(a,b), 6 asin, 7 round, 8 floor, 9 sqrt, 10 a/b, 11 max(a,b),
 * 12 min(a,b)), so the tests can check gfx950 returns the same bits as x86-64. */
spt_status spt_debug_detmath(int32_t device, uint32_t fn, uint32_t n, const float* a, const float* b, float* out);

/* Test seam (additive to ABI v14): the conversion kernel of spt_film_read_rgb8 on n caller floats. */
spt_status spt_debug_pack_rgb8(int32_t device, uint32_t n, const float* in, uint8_t* out);

/* Test seam (ABI v13) for rows a13-a16: BxdfT::{sample, bxdf, pdf} (src/bxdf/mod.rs:80-90) of ONE constant material record
 * (`recipe` 0), evaluated on the device for n inputs in the local shading frame (z = normal).
 *   op 0  sample: wo[3n], rng_state[n] (the PCG32 state a stream starts from, include/spt_detmath.h) ->
 *         wi_out[3n], f_out[3n], pdf_out[n], dir_out[n] (0 reflect, 1 transmit: BxdfDirType, mod.rs:30-36)
 *   op 1  bxdf + pdf: wo[3n], wi_in[3n] -> f_out[3n], pdf_out[n]
 * `scene` may be NULL (then `device` says where to run) unless the record is a position-normal-distribution lobe
 * (SPT_BXDF_PNDF_*: c1 = (1 / normalisation, sigma_p, P-NDF index as bits), ax / ay = u), whose tables live in a scene.
 * A Subsurface substrate is refused (SPT_ERR_UNSUPPORTED): its sample places the exit point with a traced probe ray. */
spt_status spt_debug_bxdf(const spt_scene* scene, int32_t device, const spt_material* mt, uint32_t op, uint32_t n, const float* wo,
                          const float* wi_in, const uint64_t* rng_state, float* wi_out, float* f_out, float* pdf_out, int32_t* dir_out);

/* Test seam (additive to ABI v14): how the scene's renders were scheduled since it was created.
 *   what 0  passes whose resolve was queued on the film stream (the overlapped schedule of an SPT_RENDER_ASYNC spt_render)
 *   what 1  passes that took the single-stream path (every other render, spt_film_render, SPT_NO_FILM_STREAM=1)
 *   what 2  nanoseconds the read-out kernels of the last spt_film_read / spt_film_read_rgb8 of a sample-keeping film
 *           (SPT_FILM_KEEP_SAMPLES) of the scene took on the device (0: none yet)
 *   what 3  frames of spt_render delivered without the runtime's copy: the finish kernel stored the image into rgb_mean_out
 *           itself (an SPT_RENDER_ASYNC frame on the overlapped schedule, radius 0.5, page-locked destination, no SPT_NO_DIRECT_OUT=1)
 *   what 4  spt_scene_update calls applied to the scene (a library without spt_scene_update refuses 4 and 5)
 *   what 5  bytes the last spt_scene_update copied to the device (0: none yet)
 *   what 6  ns the copies and kernels of the last spt_scene_deform that named a mesh took on the device (0: none yet); waits for
 *           them (a library without spt_scene_deform refuses 6).  Like every counter here a debug seam for the measuring tools
 *           (tools/scene_deform_cost.py), not part of what spt_scene_deform promises: it may change without an ABI version
 *   what 7  passes whose bounce launches ran on the scene's second stream beside the next pass's camera rays (the pass pipeline
 *           of an overlapped render of a fused plan; none with SPT_NO_PASS_PIPELINE=1).  Such a pass is resolved on the film
 *           stream and counts under 0 as well (a library without the pipeline refuses 7)
 *   what 8  passes whose camera rays came from the camera-model kernel (k_primary_cam: a non-perspective model, or any render under
 *           SPT_CAMERA_GENERAL=1; a library without the kernel refuses 8)
 * spt_scene_deform and spt_scene_deform_vertices count as an update in 4 and report their bytes in 5 (and their device time in 6). */
spt_status spt_debug_render_info(const spt_scene* scene, uint32_t what, uint64_t* out);

const char* spt_last_error(void);
uint32_t spt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPT_ABI_H */
