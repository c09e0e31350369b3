// csrc/hip/scene_build.h on the CPU: the scene builder alone, over scene files that libspt_host.so loads.  No HIP call, no device.
//
//   scene_build_check [--pair A.json B.json]... [--scene S.json]...
//
// Every scene is built under four sets of BuildOptions (the defaults, the large-scene form forced, the caller's trees, the streaming
// walker off), and for each the program checks properties, not recorded bytes:
//   1. layout      the sections of the blob follow each other in the documented order of the form in use without overlap, geo_f4 is
//                  the end of the last one, the blob has geo_f4 - first float4, the large-scene form's 4-wide TLAS starts at
//                  tail_first = o_blas + blas_f4;
//   2. references  every child reference and leaf range reachable from the TLAS root(s) and from every mesh root, 2-wide and 4-wide,
//                  lands inside its own section; the ABI indices in the triangles' pad lanes are a permutation of each mesh's own
//                  range; tlas_order is a permutation of the instances;
//   3. update      (--pair: B is A with other transforms) the update path from A's SceneFixed with B's arrays gives B's creation
//                  byte for byte - the whole blob in the LDS-resident form, the blob from tail_first on in the large-scene form -
//                  with B's classes and every field dyn_commit_host reads; A -> B -> A gives A again;
//   4. determinism building the same descriptor twice gives the same bytes;
//   5. refusals    a TLAS with a cycle, a child index out of range, a leaf range past the instances and a TLAS deeper than the
//                  traversal stack are refused with the status and message of the builder; an instance box that is not finite is
//                  built without a read out of bounds (the loader is what refuses one) and switches the bounding sphere off.
// One "digest" line per scene and option set (64-bit FNV-1a of the blob, the classes, the static arrays and the texture pools, and the
// decisions) lets two versions of the builder be compared by their output.  A scene file that does not load is reported and skipped.
// Built with -fsanitize=address,undefined (`make scene-build-check`): a read past an array is a report, not a wrong byte.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/spt_host.h"
#include "../simple-path-tracer_amd/csrc/hip/scene_build.h"

using namespace scene_build;

namespace {

int g_failures = 0;
std::string g_where;

void bad(const std::string& what) {
    std::fprintf(stderr, "scene_build_check: %s: %s\n", g_where.c_str(), what.c_str());
    ++g_failures;
}
#define CHECK(cond, what) do { if (!(cond)) bad(what); } while (0)

struct OptionSet {
    const char* name;
    BuildOptions opt;
};

std::vector<OptionSet> option_sets(bool with_bezier) {
    std::vector<OptionSet> sets(4);
    sets[0].name = "default";
    sets[1].name = "large";      sets[1].opt.lds_geo = false;          // what SPT_NO_LDS_GEO sets
    sets[2].name = "reference";  sets[2].opt.reference_bvh = true;     // what SPT_REFERENCE_BVH sets
    sets[3].name = "nostream";   sets[3].opt.stream = false;  sets[3].opt.lds_geo = false;   // (the walker only exists in the large-scene form)
    for (OptionSet& s : sets) s.opt.with_bezier = with_bezier;
    return sets;
}

struct Built {
    StaticBuild sb;
    SceneDynamic dy;
};

// What spt_scene_create runs of the builder
Built build(const spt_scene_desc& s, const BuildOptions& opt) {
    Built b;
    validate(s, opt);
    b.sb = build_static(s, opt);
    const StaticSections st = b.sb.sections();
    b.dy = build_dynamic(b.sb.fixed, dyn_view(s, b.sb.fixed.surf_emissive.data()), opt, b.sb.lds_geo, b.sb.blas_range.size(), &st);
    return b;
}

// What spt_scene_update runs of it: the scene `a` was created as, the four arrays of `s`
SceneDynamic update(const Built& a, const spt_scene_desc& s, const BuildOptions& opt) {
    const SceneFixed& fx = a.sb.fixed;
    const DynView view{fx.aggregate, fx.light_sampler, s.n_tlas_nodes, s.n_instances, s.n_lights, fx.n_spheres, fx.n_meshes, fx.n_bezier_patches, fx.n_surfaces,
                       fx.has_env, s.tlas_nodes, s.instances, s.lights, s.light_alias, fx.surf_emissive.data()};
    validate_instances(view, opt, "scene_update");
    validate_lights(view, "scene_update");
    validate_light_alias(view, "scene_update");
    const StaticSections st{fx.wblas.data(), fx.tri_sec.data()};
    return build_dynamic(fx, view, opt, a.sb.lds_geo, a.sb.blas_range.size(), fx.n4 ? nullptr : &st);
}

uint64_t fnv(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 0x100000001b3ull;
    return h;
}
template <class T>
uint64_t fnv_vec(const std::vector<T>& v, uint64_t h = 0xcbf29ce484222325ull) { return v.empty() ? h : fnv(v.data(), v.size() * sizeof(T), h); }
template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

void print_digest(const char* scene, const char* set, const Built& b) {
    const SceneFixed& fx = b.sb.fixed;
    const SceneDynamic& dy = b.dy;
    uint64_t st = fnv_vec(b.sb.wblas);
    st = fnv_vec(b.sb.tri_blob, st); st = fnv_vec(fx.mesh_rec, st); st = fnv_vec(b.sb.env_px, st); st = fnv_vec(b.sb.env_uk, st); st = fnv_vec(b.sb.ss_cdf, st);
    uint64_t tex = fnv_vec(b.sb.tex.prog);
    tex = fnv_vec(b.sb.tex.roots, tex); tex = fnv_vec(b.sb.tex.chain, tex);
    uint64_t bounds = fnv(dy.bs_center, sizeof dy.bs_center);
    bounds = fnv(&dy.bs_radius, sizeof dy.bs_radius, bounds); bounds = fnv(dy.world_lo, sizeof dy.world_lo, bounds); bounds = fnv(dy.world_hi, sizeof dy.world_hi, bounds);
    bounds = fnv_vec(dy.hull_corners, bounds);
    std::printf("digest %s %s blob=%016" PRIx64 " cls=%016" PRIx64 " static=%016" PRIx64 " tex=%016" PRIx64 " bounds=%016" PRIx64
                " geo_f4=%u tail_first=%u blas_f4=%u lds_geo=%d n4=%d own_bvh=%d swalk=%d flat=%u lds_tables=%d fused=%d simple=%d eye_ok=%d stack_cap=%u"
                " tlas_root=%08x s_root=%08x simple_fixed=%d fused_fixed=%d textured=%d subsurface=%d probe=%d pndf=%d newton=%d bs_valid=%d ranges=%zu need=%u depth=%u/%u\n",
                scene, set, fnv_vec(dy.blob), fnv_vec(dy.cls), st, tex, bounds, dy.geo_f4, fx.tail_first, fx.blas_f4, (int)b.sb.lds_geo, (int)fx.n4, (int)fx.own_bvh,
                (int)dy.swalk, dy.flat, (int)dy.lds_tables, (int)dy.fused, (int)dy.simple, (int)dy.eye_ok, dy.stack_cap, dy.tlas_root, dy.s_root, (int)fx.simple_fixed,
                (int)fx.fused_fixed, (int)b.sb.textured, (int)b.sb.subsurface, (int)b.sb.has_probe, (int)b.sb.has_pndf, (int)b.sb.bez_newton, (int)dy.bs_valid,
                b.sb.blas_range.size(), fx.max_blas_need, fx.blas_depth, fx.own_blas_depth);
}

size_t f4_of(size_t bytes) { return (bytes + 15) / 16; }

// 1. layout
void check_layout(const Built& b, const SceneDynamic& dy, uint32_t first) {
    const SceneFixed& fx = b.sb.fixed;
    struct Sec { const char* name; uint32_t off; size_t size; };
    const size_t n = fx.n_instances;
    const Sec sinst{"sinst", dy.o_sinst, dy.sinst.size()}, tlas{"tlas", dy.o_tlas, dy.wtlas.size()}, inst{"instances", dy.o_inst, f4_of(n * sizeof(spt_instance))},
        mesh{"meshes", dy.o_mesh, fx.mesh_rec.size()}, sph{"spheres", dy.o_sph, f4_of((size_t)fx.n_spheres * sizeof(spt_sphere))}, blas{"blas", dy.o_blas, fx.blas_f4},
        tri{"tri", dy.o_tri, f4_of((size_t)fx.n_tris * sizeof(spt_tri_pos))}, tord{"order", dy.o_tord, f4_of(n * sizeof(uint32_t))};
    std::vector<Sec> order;
    if (!fx.n4) {
        order = {sinst, tlas, inst, mesh, sph, blas, tri, tord};
        if (dy.lds_tables) {
            order.push_back(Sec{"attr", dy.o_attr, fx.attr_sec.size()});
            order.push_back(Sec{"surfaces", dy.o_surf, fx.surf_sec.size()});
            order.push_back(Sec{"materials", dy.o_mat, fx.mat_sec.size()});
            order.push_back(Sec{"lights", dy.o_light, f4_of((size_t)fx.n_lights * sizeof(spt_light))});
        }
    } else {
        const Sec stlas{"4-wide tlas", dy.tail_first, dy.stlas.size()};
        order = {mesh, sph, tri, blas, stlas, sinst, tlas, inst, tord};
        CHECK(dy.tail_first == dy.o_blas + fx.blas_f4, "tail_first is not o_blas + blas_f4");
        CHECK(dy.tail_first == fx.tail_first, "the layout's tail_first differs from the creation's");
        CHECK(!dy.lds_tables, "shading tables in the large-scene form");
    }
    CHECK(order.front().off == 0, std::string("the first section (") + order.front().name + ") does not start the blob");
    for (size_t k = 0; k + 1 < order.size(); ++k) {
        CHECK(order[k].off <= order[k + 1].off, std::string("section offsets decrease at ") + order[k + 1].name);
        CHECK((size_t)order[k].off + order[k].size <= order[k + 1].off, std::string(order[k].name) + " overlaps " + order[k + 1].name);
    }
    CHECK((size_t)order.back().off + order.back().size == dy.geo_f4, "geo_f4 is not the end of the last section");
    CHECK(dy.blob.size() == (size_t)dy.geo_f4 - first, "the blob's size is not geo_f4 - first");
    CHECK(!b.sb.lds_geo || lds_fits(dy.plain_f4), "an LDS-resident blob that does not fit LDS");
    CHECK(b.sb.lds_geo == !fx.n4, "lds_geo and the form of the BLAS nodes disagree");
}

uint32_t word(const float4& f, int lane) {
    const float v = lane == 0 ? f.x : lane == 1 ? f.y : lane == 2 ? f.z : f.w;
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// A walk of one tree of the blob from `root` (a ref): inner refs must name nodes [node_lo, node_hi) (units of 4 float4 behind
// `base_f4`), leaf ranges must lie in [item_lo, item_hi); `seen` marks the items the leaves cover
void walk(const std::vector<float4>& blob, bool four_wide, uint32_t base_f4, uint32_t node_lo, uint32_t node_hi, uint32_t root, uint32_t item_lo, uint32_t item_hi,
          std::vector<uint32_t>& seen, const char* what) {
    std::vector<uint32_t> todo(1, root);
    size_t visited = 0;
    while (!todo.empty()) {
        const uint32_t ref = todo.back();
        todo.pop_back();
        if (ref & kLeaf) {
            const uint32_t cnt = (ref >> 27) & 15u, first = ref & 0x07ffffffu;
            if (first < item_lo || (uint64_t)first + cnt > item_hi) { bad(std::string(what) + ": a leaf range leaves its section"); continue; }
            for (uint32_t k = 0; k < cnt; ++k) ++seen[first + k];
            continue;
        }
        if (ref < node_lo || ref >= node_hi) { bad(std::string(what) + ": a child reference leaves its section"); continue; }
        if (++visited > (size_t)node_hi - node_lo) { bad(std::string(what) + ": the nodes do not form a tree"); return; }
        const size_t at = (size_t)base_f4 + (size_t)ref * 4;
        if (at + 4 > blob.size()) { bad(std::string(what) + ": a node lies behind the blob"); continue; }
        const float4* f = &blob[at];
        if (four_wide) {
            const uint32_t n = word(f[0], 3) >> 24;
            if (n < 2 || n > 4) { bad(std::string(what) + ": a 4-wide node without 2 .. 4 children"); continue; }
            const uint32_t refs[4] = {word(f[2], 2), word(f[2], 3), word(f[3], 0), word(f[3], 1)};
            for (uint32_t c = 0; c < n; ++c) todo.push_back(refs[c]);
        } else {
            todo.push_back(word(f[0], 3));
            todo.push_back(word(f[1], 3));
        }
    }
}

// 2. references (on a creation's blob, which has every section)
void check_references(const spt_scene_desc& s, const Built& b) {
    const SceneFixed& fx = b.sb.fixed;
    const SceneDynamic& dy = b.dy;
    const std::vector<float4>& blob = dy.blob;
    const uint32_t n = s.n_instances;
    // the trees over the instances: every instance slot is covered exactly once
    if (s.aggregate == SPT_AGGREGATE_BVH && s.n_tlas_nodes && n) {
        std::vector<uint32_t> seen(n, 0u);
        walk(blob, false, dy.o_tlas, 0u, (uint32_t)(dy.wtlas.size() / 4), dy.tlas_root, 0u, n, seen, "tlas");
        for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1u, "tlas: an instance slot is not covered exactly once");
    }
    if (!dy.sinst.empty()) {   // (the 4-wide TLAS of one instance is a leaf ref and no node)
        std::vector<uint32_t> seen(n, 0u);
        const uint32_t lo = fx.blas_f4 / 4u;
        walk(blob, true, dy.o_blas, lo, lo + (uint32_t)(dy.stlas.size() / 4), dy.s_root, 0u, n, seen, "4-wide tlas");
        for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1u, "4-wide tlas: an instance slot is not covered exactly once");
        CHECK(dy.sinst.size() == (size_t)n * 6, "the streaming walker's entries are not 6 float4 per instance");
    }
    CHECK(!dy.swalk || !dy.sinst.empty(), "swalk without the streaming walker's tables");
    // the trees over the triangles: every mesh root covers exactly its own triangles
    for (uint32_t m = 0; m < s.n_meshes; ++m) {
        const spt_mesh& mm = s.meshes[m];
        std::vector<uint32_t> seen(s.n_tris, 0u);
        const uint32_t root = word(blob[(size_t)dy.o_mesh + 2 * m], 3);
        uint32_t lo = 0u, hi = fx.blas_f4 / 4u;
        if (!fx.n4) { lo = b.sb.blas_range[m].first; hi = b.sb.blas_range[m].second; }
        walk(blob, fx.n4, dy.o_blas, lo, hi, root, mm.tri_first, mm.tri_first + mm.tri_count, seen, "blas");
        for (uint32_t t = 0; t < s.n_tris; ++t)
            CHECK(seen[t] == ((t >= mm.tri_first && t < mm.tri_first + mm.tri_count) ? 1u : 0u), "blas: a mesh's leaves do not cover exactly its own triangles");
        // the ABI indices in the pad lanes: a permutation of the mesh's range
        std::vector<uint32_t> hit(mm.tri_count, 0u);
        for (uint32_t t = mm.tri_first; t < mm.tri_first + mm.tri_count; ++t) {
            const uint32_t abi = word(blob[(size_t)dy.o_tri + 3 * (size_t)t], 3);
            if (abi < mm.tri_first || abi >= mm.tri_first + mm.tri_count) { bad("a triangle's ABI index leaves its mesh"); continue; }
            ++hit[abi - mm.tri_first];
        }
        for (uint32_t h : hit) CHECK(h == 1u, "the ABI indices of a mesh are not a permutation of its range");
    }
    CHECK(!fx.n4 ? b.sb.blas_range.size() == s.n_meshes : b.sb.blas_range.empty(), "blas_range does not go with the form");
    // tlas_order: a permutation of the instances, and what the blob carries
    CHECK(dy.tlas_order.size() == n, "tlas_order does not have one entry per instance");
    std::vector<uint32_t> hit(n, 0u);
    for (uint32_t i : dy.tlas_order) { if (i < n) ++hit[i]; else bad("tlas_order names an instance out of range"); }
    for (uint32_t h : hit) CHECK(h == 1u, "tlas_order is not a permutation of the instances");
    CHECK(n == 0 || std::memcmp(&blob[dy.o_tord], dy.tlas_order.data(), (size_t)n * 4) == 0, "the blob's order section is not tlas_order");
    CHECK(dy.cls.size() == (n ? n : 1u), "the classes are not one per instance");
}

// every field dyn_commit_host reads, and the classes
void check_same_dynamic(const SceneDynamic& got, const SceneDynamic& want, bool n4, uint32_t tail_first, const char* what) {
    const std::string w(what);
    if (!n4) {
        CHECK(same(got.blob, want.blob), w + ": the blob differs");
    } else {
        CHECK(got.blob.size() + tail_first == want.blob.size() && (got.blob.empty() || std::memcmp(got.blob.data(), want.blob.data() + tail_first, got.blob.size() * 16) == 0),
              w + ": the blob from tail_first on differs");
    }
    CHECK(same(got.cls, want.cls), w + ": the classes differ");
    CHECK(got.n_tlas_nodes == want.n_tlas_nodes && got.stack_cap == want.stack_cap && got.tlas_root == want.tlas_root && got.s_root == want.s_root && got.flat == want.flat,
          w + ": roots, stack_cap or flat differ");
    CHECK(std::memcmp(got.tlas_lo, want.tlas_lo, sizeof got.tlas_lo) == 0 && std::memcmp(got.tlas_hi, want.tlas_hi, sizeof got.tlas_hi) == 0, w + ": the TLAS box differs");
    CHECK(got.o_sinst == want.o_sinst && got.o_tlas == want.o_tlas && got.o_inst == want.o_inst && got.o_mesh == want.o_mesh && got.o_sph == want.o_sph &&
              got.o_blas == want.o_blas && got.o_tri == want.o_tri && got.o_tord == want.o_tord && got.o_attr == want.o_attr && got.o_surf == want.o_surf &&
              got.o_mat == want.o_mat && got.o_light == want.o_light && got.geo_f4 == want.geo_f4 && got.tail_first == want.tail_first && got.plain_f4 == want.plain_f4,
          w + ": the offsets differ");
    CHECK(got.swalk == want.swalk && got.lds_tables == want.lds_tables && got.fused == want.fused && got.simple == want.simple && got.eye_ok == want.eye_ok,
          w + ": the kernel choices differ");
    CHECK(got.wtlas.size() == want.wtlas.size(), w + ": the 2-wide TLAS differs in size");
    CHECK(std::memcmp(got.bs_center, want.bs_center, sizeof got.bs_center) == 0 && std::memcmp(&got.bs_radius, &want.bs_radius, sizeof got.bs_radius) == 0 &&
              std::memcmp(got.world_lo, want.world_lo, sizeof got.world_lo) == 0 && std::memcmp(got.world_hi, want.world_hi, sizeof got.world_hi) == 0 &&
              got.bs_valid == want.bs_valid,
          w + ": the bounds differ");
    CHECK(same(got.hull_corners, want.hull_corners), w + ": hull_corners differ");
}

void check_same_static(const Built& x, const Built& y, const char* what) {
    const std::string w(what);
    CHECK(same(x.sb.wblas, y.sb.wblas) && same(x.sb.tri_blob, y.sb.tri_blob) && same(x.sb.fixed.mesh_rec, y.sb.fixed.mesh_rec) && same(x.sb.blas_range, y.sb.blas_range),
          w + ": the static geometry differs");
    CHECK(same(x.sb.tex.prog, y.sb.tex.prog) && same(x.sb.tex.roots, y.sb.tex.roots) && same(x.sb.tex.chain, y.sb.tex.chain), w + ": the texture pools differ");
    CHECK(same(x.sb.env_px, y.sb.env_px) && same(x.sb.env_uk, y.sb.env_uk) && same(x.sb.ss_cdf, y.sb.ss_cdf), w + ": the environment or the BSSRDF table differs");
    CHECK(x.sb.lds_geo == y.sb.lds_geo && x.sb.fixed.n4 == y.sb.fixed.n4 && x.sb.fixed.tail_first == y.sb.fixed.tail_first && x.sb.fixed.blas_f4 == y.sb.fixed.blas_f4,
          w + ": the form differs");
}

bool has_patch_instance(const spt_scene_desc& s) {
    for (uint32_t i = 0; i < s.n_instances; ++i)
        if (s.instances[i].prim_type == SPT_PRIM_BEZIER) return true;
    return false;
}

const char* base_name(const char* path) {
    const char* slash = std::strrchr(path, '/');
    return slash ? slash + 1 : path;
}

spt_host_scene* load(const char* path) {
    spt_host_scene* h = nullptr;
    if (spt_host_load_scene(path, &h) != SPT_OK || !h) {
        std::printf("skipped %s: it does not load (%s)\n", path, spt_host_last_error());
        return nullptr;
    }
    return h;
}

// properties 1, 2 and 4 of one scene under every option set (and its digest lines)
void check_scene(const char* path, const spt_scene_desc& s) {
    for (const OptionSet& os : option_sets(has_patch_instance(s))) {
        g_where = std::string(base_name(path)) + " [" + os.name + "]";
        try {
            const Built b = build(s, os.opt);
            print_digest(base_name(path), os.name, b);
            check_layout(b, b.dy, 0u);
            check_references(s, b);
            CHECK(b.sb.fixed.own_bvh == !os.opt.reference_bvh, "own_bvh does not follow the options");
            CHECK(os.opt.lds_geo || !b.sb.lds_geo, "the LDS-resident form although the options forbid it");
            CHECK(os.opt.stream || !b.dy.swalk, "the streaming walker although the options forbid it");
            const Built again = build(s, os.opt);
            check_same_static(again, b, "a second build");
            check_same_dynamic(again.dy, b.dy, false, 0u, "a second build");
        } catch (const AbiError& e) {
            bad("refused (" + std::to_string((int)e.code) + "): " + e.msg);
        }
    }
}

// property 3: B is A with other instance transforms, lights and alias table
void check_pair(const char* path_a, const spt_scene_desc& a, const char* path_b, const spt_scene_desc& b) {
    for (const OptionSet& os : option_sets(has_patch_instance(a))) {
        g_where = std::string(base_name(path_a)) + " -> " + base_name(path_b) + " [" + os.name + "]";
        try {
            const Built ba = build(a, os.opt), bb = build(b, os.opt);
            check_same_static(ba, bb, "the two creations");   // (what an update keeps really is the same in both files)
            const uint32_t tail = ba.sb.fixed.n4 ? ba.sb.fixed.tail_first : 0u;
            const SceneDynamic ab = update(ba, b, os.opt);
            check_layout(ba, ab, tail);
            check_same_dynamic(ab, bb.dy, ba.sb.fixed.n4, tail, "A updated to B against B");
            const SceneDynamic aba = update(ba, a, os.opt);   // (the fixed part does not change with an update: from the same SceneFixed)
            check_same_dynamic(aba, ba.dy, ba.sb.fixed.n4, tail, "A -> B -> A against A");
            CHECK(!same(ab.blob, aba.blob), "A and B do not differ: the pair checks nothing");
        } catch (const AbiError& e) {
            bad("refused (" + std::to_string((int)e.code) + "): " + e.msg);
        }
    }
}

void expect_refusal(const spt_scene_desc& s, const BuildOptions& opt, spt_status code, const char* msg, const char* what) {
    g_where = std::string("refusal: ") + what;
    try {
        build(s, opt);
        bad("was built");
    } catch (const AbiError& e) {
        CHECK(e.code == code && e.msg == msg, "refused with (" + std::to_string((int)e.code) + ") '" + e.msg + "', expected (" + std::to_string((int)code) + ") '" + msg + "'");
    }
}

// property 5, on a scene with a bvh aggregate whose TLAS root is an inner node
void check_refusals(const spt_scene_desc& s) {
    g_where = "refusals";
    if (s.aggregate != SPT_AGGREGATE_BVH || s.n_tlas_nodes < 3 || (s.tlas_nodes[0].b & SPT_LEAF_FLAG)) { bad("the scene has no TLAS with an inner root"); return; }
    const std::vector<spt_bvh_node> nodes(s.tlas_nodes, s.tlas_nodes + s.n_tlas_nodes);
    const std::vector<OptionSet> sets = option_sets(false);
    for (size_t k = 0; k < 3; ++k) {   // the defaults, the large-scene form, the caller's trees
        const BuildOptions& opt = sets[k].opt;
        spt_scene_desc d = s;
        std::vector<spt_bvh_node> t = nodes;
        d.tlas_nodes = t.data();
        t[0].b = 0u;   // the root is its own child
        expect_refusal(d, opt, SPT_ERR_INVALID_ARG, "tlas: node graph is not a tree", "a node array with a cycle");
        t = nodes;
        t[0].a = s.n_tlas_nodes + 7u;
        expect_refusal(d, opt, SPT_ERR_INVALID_ARG, "tlas: node index out of range", "a child index out of range");
        t = nodes;
        for (spt_bvh_node& nd : t)
            if (nd.b & SPT_LEAF_FLAG) { nd.a = s.n_instances; break; }
        expect_refusal(d, opt, SPT_ERR_INVALID_ARG, "tlas: leaf item range out of bounds", "a leaf range past the item count");
        // a chain: inner node 2 k has the leaf 2 k + 1 and the next inner node (the last one two leaves), 60 levels
        const uint32_t levels = 60u;
        t.assign(2 * levels + 1, nodes[0]);
        for (uint32_t l = 0; l < levels; ++l) {
            t[2 * l].a = 2 * l + 1;
            t[2 * l].b = 2 * l + 2;
            t[2 * l + 1].a = 0u;
            t[2 * l + 1].b = SPT_LEAF_FLAG | 1u;
        }
        t[2 * levels].a = 0u;
        t[2 * levels].b = SPT_LEAF_FLAG | 1u;
        d.tlas_nodes = t.data();
        d.n_tlas_nodes = (uint32_t)t.size();
        expect_refusal(d, opt, SPT_ERR_UNSUPPORTED,
                       opt.reference_bvh ? "BVH deeper than the traversal stack (48 levels)" : "TLAS deeper than the traversal stack (48 levels)", "a TLAS deeper than the traversal stack");
        // an instance box that is not finite: the builder has no refusal of its own for it (the loader refuses the transform that
        // makes one); it must read nothing out of bounds, and the bounding sphere, which the pixel culling trusts, must be off
        for (const float v : {std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) {
            g_where = std::string("a non-finite instance box [") + sets[k].name + "]";
            d = s;
            std::vector<spt_instance> inst(s.instances, s.instances + s.n_instances);
            inst[s.n_instances / 2].bmax[1] = v;
            d.instances = inst.data();
            try {
                const Built b = build(d, opt);
                CHECK(!b.dy.bs_valid && b.dy.hull_corners.empty(), "a bounding sphere of a box that is not finite");
                check_layout(b, b.dy, 0u);
            } catch (const AbiError& e) {
                bad("refused (" + std::to_string((int)e.code) + "): " + e.msg + " (the builder had no such refusal: give this case its status and text)");
            }
        }
    }
}

// BuildOptions::from_env(): the nine variables, their defaults and clamps (the only place this program touches the environment)
void check_from_env() {
    g_where = "from_env";
    const char* names[] = {"SPT_BVH_MAX_LEAF", "SPT_BVH_TRAVERSAL_COST", "SPT_DEBUG_BVH", "SPT_NO_STREAM", "SPT_FLAT_BUDGET", "SPT_NO_EYE_BLOB", "SPT_REFERENCE_BVH",
                           "SPT_NO_LDS_GEO", "SPT_BEZ_LDS"};
    for (const char* n : names) unsetenv(n);
    setenv("SPT_NO_STREAMS", "1", 1);   // names that only begin like one of the nine
    setenv("SPT_BEZ_LDS_X", "1", 1);
    BuildOptions o = BuildOptions::from_env();
    const BuildOptions d;
    CHECK(o.bvh_max_leaf == d.bvh_max_leaf && o.bvh_traversal_cost == d.bvh_traversal_cost && !o.debug_bvh && o.stream && o.flat_budget == kFlatBudget && o.eye_blob &&
              !o.reference_bvh && o.lds_geo && !o.bez_lds && !o.with_bezier,
          "an empty environment does not give the defaults");
    CHECK(d.bvh_max_leaf == 4u && d.bvh_traversal_cost == 1.2f, "the defaults of the BLAS builder changed");
    setenv("SPT_BVH_MAX_LEAF", "99", 1);
    setenv("SPT_BVH_TRAVERSAL_COST", "0.75", 1);
    setenv("SPT_FLAT_BUDGET", "0", 1);
    for (const char* n : {"SPT_DEBUG_BVH", "SPT_NO_STREAM", "SPT_NO_EYE_BLOB", "SPT_REFERENCE_BVH", "SPT_NO_LDS_GEO", "SPT_BEZ_LDS"}) setenv(n, "1", 1);
    o = BuildOptions::from_env();
    CHECK(o.bvh_max_leaf == 15u && o.bvh_traversal_cost == 0.75f && o.debug_bvh && !o.stream && o.flat_budget == 0u && !o.eye_blob && o.reference_bvh && !o.lds_geo && o.bez_lds,
          "the nine variables do not arrive in the options");
    setenv("SPT_BVH_MAX_LEAF", "0", 1);
    setenv("SPT_NO_LDS_GEO", "", 1);   // set, if empty, counts
    o = BuildOptions::from_env();
    CHECK(o.bvh_max_leaf == 1u && !o.lds_geo, "clamp of SPT_BVH_MAX_LEAF, or an empty value");
    for (const char* n : names) unsetenv(n);
    unsetenv("SPT_NO_STREAMS");
    unsetenv("SPT_BEZ_LDS_X");
}

}  // namespace

int main(int argc, char** argv) {
    check_from_env();
    int scenes = 0;
    bool refusals_done = false;
    for (int i = 1; i < argc; ++i) {
        const std::string arg(argv[i]);
        if (arg == "--pair" && i + 2 < argc) {
            spt_host_scene *a = load(argv[i + 1]), *b = load(argv[i + 2]);
            if (a && b) {
                check_scene(argv[i + 1], *spt_host_scene_desc(a));
                check_scene(argv[i + 2], *spt_host_scene_desc(b));
                check_pair(argv[i + 1], *spt_host_scene_desc(a), argv[i + 2], *spt_host_scene_desc(b));
                if (!refusals_done && spt_host_scene_desc(a)->aggregate == SPT_AGGREGATE_BVH) {
                    check_refusals(*spt_host_scene_desc(a));
                    refusals_done = true;
                }
                scenes += 2;
            }
            if (a) spt_host_scene_free(a);
            if (b) spt_host_scene_free(b);
            i += 2;
        } else if (arg == "--scene" && i + 1 < argc) {
            if (spt_host_scene* h = load(argv[i + 1])) {
                check_scene(argv[i + 1], *spt_host_scene_desc(h));
                spt_host_scene_free(h);
                ++scenes;
            }
            i += 1;
        } else {
            std::fprintf(stderr, "usage: scene_build_check [--pair A.json B.json]... [--scene S.json]...\n");
            return 2;
        }
    }
    g_where = "arguments";
    CHECK(scenes > 0, "no scene was checked");
    CHECK(refusals_done, "no pair with a bvh aggregate: the refusals were not checked");
    if (g_failures) {
        std::fprintf(stderr, "scene_build_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("scene_build_check ok: %d scenes\n", scenes);
    return 0;
}
