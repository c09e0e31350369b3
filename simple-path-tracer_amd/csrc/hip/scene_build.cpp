// The scene builder (scene_build.h): host code only.
#include "scene_build.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>

#include "../../../include/spt_detmath.h"   // spt_ss_cdf_entry
#include "../../../include/spt_pndf.h"      // SPT_PNDF_STACK
#include "scene_refit.h"

namespace scene_build {

BuildOptions BuildOptions::from_env() {
    BuildOptions o;
    if (const char* v = std::getenv("SPT_BVH_MAX_LEAF")) o.bvh_max_leaf = (uint32_t)std::min(15, std::max(1, std::atoi(v)));
    if (const char* v = std::getenv("SPT_BVH_TRAVERSAL_COST")) o.bvh_traversal_cost = (float)std::atof(v);
    o.debug_bvh = std::getenv("SPT_DEBUG_BVH") != nullptr;
    o.stream = std::getenv("SPT_NO_STREAM") == nullptr;
    if (const char* v = std::getenv("SPT_FLAT_BUDGET")) o.flat_budget = (uint64_t)std::atoi(v);
    o.eye_blob = std::getenv("SPT_NO_EYE_BLOB") == nullptr;
    o.reference_bvh = std::getenv("SPT_REFERENCE_BVH") != nullptr;   // see build_sah_blas
    o.lds_geo = std::getenv("SPT_NO_LDS_GEO") == nullptr;            // tests: drive small scenes through the large-scene path
    o.bez_lds = std::getenv("SPT_BEZ_LDS") != nullptr;
    return o;
}

namespace {

uint32_t bvh_depth(const spt_bvh_node* nodes, uint32_t n_nodes, uint32_t root, uint32_t n_items, const char* what) {
    // iterative DFS; also validates indices so the kernels never read out of bounds
    if (n_nodes == 0) return 0;
    std::vector<std::pair<uint32_t, uint32_t>> st;
    st.emplace_back(root, 1u);
    uint32_t depth = 0, visited = 0;
    while (!st.empty()) {
        auto [ni, d] = st.back();
        st.pop_back();
        if (ni >= n_nodes) fail(SPT_ERR_INVALID_ARG, std::string(what) + ": node index out of range");
        if (++visited > n_nodes) fail(SPT_ERR_INVALID_ARG, std::string(what) + ": node graph is not a tree");
        depth = std::max(depth, d);
        const spt_bvh_node& nd = nodes[ni];
        if (nd.b & SPT_LEAF_FLAG) {
            uint32_t cnt = nd.b & ~SPT_LEAF_FLAG;
            if ((uint64_t)nd.a + cnt > n_items) fail(SPT_ERR_INVALID_ARG, std::string(what) + ": leaf item range out of bounds");
        } else {
            st.emplace_back(nd.a, d + 1);
            st.emplace_back(nd.b, d + 1);
        }
    }
    return depth;
}

// ---- device-side BLAS ---------------------------------------------------------------------------
// The ABI hands over the caller's trees (the reference side would flatten ITS BvhAccel, whose builder bins
// a primitive by (centroid - its OWN bbox min) / bucket length, src/primitive/bvh.rs:52-57, i.e. by size
// rather than position; libspt_host.so builds a proper binned-SAH tree but always splits down to <= 4).
// A closest / any hit does not depend on the tree, only on the set of triangles, so the library does not
// rely on the caller's tree quality: it builds its own binned-SAH tree per mesh (32 bins, 3 axes, SAH
// leaf termination, leaves of <= 4) over the same triangles.  Node boxes are padded outward (2^-16 of
// the extent + 2^-20 of the magnitude) so that every ray the triangle test accepts also passes the boxes
// above that triangle.  What can differ from a walk of the caller's tree are only the triangle test's own
// false positives for rays grazing a triangle's plane outside its padded box (~1e-7 per ray; none in any
// committed parity case); SPT_REFERENCE_BVH=1 walks the ABI trees instead, and the GPU parity suite is
// green (bit-identical films) in both modes.  Triangles are re-ordered into leaf order in the traversal
// blob; each carries its ABI index in the pad lane of its first vertex (tie-rule key, tri_attr index).
// Measured against libspt_host's trees: cfg2 38.4 -> 39.3 Gsamples/s, cfg5 761 -> 777 Msamples/s.
// Outward padding of a device-side box along one axis.  It has to stay well below Ray::T_MIN_EPS (1e-4):
// a ray leaving a convex object is rejected at the object's root box because it exits the box before
// t_min - with 2^-12 of the extent the cube's rays entered the tree and the fused shade kernel went from
// 2.6 to 3.5 ms (measured).  The slab test only fails for a ray that the triangle test accepts when the
// hit lies within the rounding error of a box EDGE (two slabs barely overlapping), so this small pad
// already makes a wrongly culled hit a ~1e-8-per-ray event.
// (the arithmetic lives in scene_refit.h: the refit kernels of spt_scene_deform pad with the same function)
inline float box_pad(float lo, float hi) { return refit_pad(lo, hi); }
struct SahTri {
    float lo[3], hi[3], c[3];
    uint32_t id;
};
void build_sah(std::vector<SahTri>& t, uint32_t tri_first, uint32_t max_leaf, float traversal_cost, bool debug, std::vector<spt_bvh_node>& nodes,
               std::vector<uint32_t>& order, const char* what);

void build_sah_blas(const spt_tri_pos* mesh_tris /* the mesh's own records */, uint32_t tri_first, uint32_t tri_count, const BuildOptions& opt,
                    std::vector<spt_bvh_node>& nodes, std::vector<uint32_t>& order /* slot (absolute) -> ABI triangle index, filled for this mesh's range */) {
    std::vector<SahTri> t(tri_count);
    for (uint32_t i = 0; i < tri_count; ++i) {
        const spt_tri_pos& p = mesh_tris[i];
        for (int k = 0; k < 3; ++k) {
            t[i].lo[k] = std::min(p.p0[k], std::min(p.p1[k], p.p2[k]));
            t[i].hi[k] = std::max(p.p0[k], std::max(p.p1[k], p.p2[k]));
            t[i].c[k] = 0.5f * (t[i].lo[k] + t[i].hi[k]);
        }
        t[i].id = tri_first + i;
    }
    build_sah(t, tri_first, opt.bvh_max_leaf, opt.bvh_traversal_cost, opt.debug_bvh, nodes, order, "BLAS");   // (the tuning knobs: BuildOptions)
}

// CubicBezier::intersect_ray ACCEPTS a candidate point of the patch that lies within a tolerance of the ray
// (|cross(p - o, d)|^2 < 1e-5 in the patch's object space, bezier.rs:121-131), so a ray that misses the hull of the control
// points by a hair can still "hit" - and the hit's t can lie a hair in front of the box.  Which of those near misses a
// walker sees would then depend on how tight its boxes are and on the order of its visits (fuzz seeds 3017 / 3034 of round
// 2: the streaming walker's quantised boxes against the padded ones, one or two pixels per 600 k samples).  Every box this
// library culls a patch with is therefore widened by the largest distance, in world space, at which the test can
// accept: sqrt(1e-5) over the smallest singular value of cof(M^-1) = sqrt(1e-5) * s1 * s2 (the two largest stretches of
// the instance's M), bounded here by |M|_F^2 / 2.  With that, "tested" is a superset of "can be accepted" for every walker,
// and all of them return what testing every patch returns.  (SPT_REFERENCE_BVH=1 keeps the caller's exact boxes and the
// reference's visit order: that mode reproduces the reference's own loss of such hits.)
float bezier_box_margin(const spt_instance& in) {
    if (in.prim_type != SPT_PRIM_BEZIER) return 0.0f;
    double f2 = 0.0;
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) f2 += (double)in.fwd[3 * c + r] * (double)in.fwd[3 * c + r];   // the 3 x 3 part (columns), not the translation
    return (float)(0.0031623 * 1.02 * 0.5 * f2 + 1e-6);
}

// The same builder over the instances' world boxes: the device-side TLAS.  An instance visit (transform the ray, walk
// a BLAS) costs far more than a node visit, so leaves hold one instance unless the split is useless.
void build_sah_tlas(const spt_instance* inst, uint32_t n, const BuildOptions& opt, std::vector<spt_bvh_node>& nodes, std::vector<uint32_t>& order) {
    std::vector<SahTri> t(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float margin = bezier_box_margin(inst[i]);
        for (int k = 0; k < 3; ++k) {
            t[i].lo[k] = inst[i].bmin[k] - margin;
            t[i].hi[k] = inst[i].bmax[k] + margin;
            t[i].c[k] = 0.5f * (t[i].lo[k] + t[i].hi[k]);
        }
        t[i].id = i;
    }
    order.assign(n, 0u);
    build_sah(t, 0u, 2u, 0.125f, opt.debug_bvh, nodes, order, "TLAS");
}

// items [0, t.size()) -> a tree appended to `nodes`; leaves index slots tri_first + k, order[slot] = item id
void build_sah(std::vector<SahTri>& t, uint32_t tri_first, uint32_t kMaxLeaf, float kTraversalCost, bool debug, std::vector<spt_bvh_node>& nodes,
               std::vector<uint32_t>& order, const char* what) {
    const uint32_t tri_count = (uint32_t)t.size();
    constexpr int kBins = 32;
    auto half_area = [](const float* lo, const float* hi) {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    struct Task { uint32_t begin, end, node, depth; };
    std::vector<Task> st;
    const size_t root_index = nodes.size();
    nodes.push_back(spt_bvh_node{});
    st.push_back(Task{0u, tri_count, (uint32_t)nodes.size() - 1u, 0u});
    while (!st.empty()) {
        const Task tk = st.back();
        st.pop_back();
        const uint32_t n = tk.end - tk.begin;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t i = tk.begin; i < tk.end; ++i)
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], t[i].lo[k]); hi[k] = std::max(hi[k], t[i].hi[k]);
                clo[k] = std::min(clo[k], t[i].c[k]); chi[k] = std::max(chi[k], t[i].c[k]);
            }
        spt_bvh_node nd;
        for (int k = 0; k < 3; ++k) {
            const float pad = box_pad(lo[k], hi[k]);
            nd.bmin[k] = lo[k] - pad;
            nd.bmax[k] = hi[k] + pad;
        }
        auto make_leaf = [&]() {
            nd.a = tri_first + tk.begin;
            nd.b = SPT_LEAF_FLAG | n;
            nodes[tk.node] = nd;
        };
        if (n == 1) { make_leaf(); continue; }
        // best binned split over the three axes
        float best_cost = INFINITY;
        int best_axis = -1, best_bin = 0;
        for (int k = 0; k < 3; ++k) {
            const float ext = chi[k] - clo[k];
            if (!(ext > 0.0f) || !std::isfinite(ext)) continue;
            const float scale = (float)kBins / ext;
            uint32_t cnt[kBins] = {};
            float blo[kBins][3], bhi[kBins][3];
            for (int b = 0; b < kBins; ++b)
                for (int j = 0; j < 3; ++j) { blo[b][j] = INFINITY; bhi[b][j] = -INFINITY; }
            for (uint32_t i = tk.begin; i < tk.end; ++i) {
                int b = std::min(kBins - 1, std::max(0, (int)((t[i].c[k] - clo[k]) * scale)));
                ++cnt[b];
                for (int j = 0; j < 3; ++j) { blo[b][j] = std::min(blo[b][j], t[i].lo[j]); bhi[b][j] = std::max(bhi[b][j], t[i].hi[j]); }
            }
            float right_area[kBins];
            uint32_t right_cnt[kBins];
            {
                float rl[3] = {INFINITY, INFINITY, INFINITY}, rh[3] = {-INFINITY, -INFINITY, -INFINITY};
                uint32_t rc = 0;
                for (int b = kBins - 1; b >= 1; --b) {
                    for (int j = 0; j < 3; ++j) { rl[j] = std::min(rl[j], blo[b][j]); rh[j] = std::max(rh[j], bhi[b][j]); }
                    rc += cnt[b];
                    right_area[b] = rc ? half_area(rl, rh) : 0.0f;
                    right_cnt[b] = rc;
                }
            }
            float ll[3] = {INFINITY, INFINITY, INFINITY}, lh[3] = {-INFINITY, -INFINITY, -INFINITY};
            uint32_t lc = 0;
            for (int b = 1; b < kBins; ++b) {   // split between bin b-1 and b
                for (int j = 0; j < 3; ++j) { ll[j] = std::min(ll[j], blo[b - 1][j]); lh[j] = std::max(lh[j], bhi[b - 1][j]); }
                lc += cnt[b - 1];
                if (lc == 0 || right_cnt[b] == 0) continue;
                const float cost = half_area(ll, lh) * (float)lc + right_area[b] * (float)right_cnt[b];
                if (cost < best_cost) { best_cost = cost; best_axis = k; best_bin = b; }
            }
        }
        const float node_area = half_area(lo, hi);
        uint32_t mid;
        if (best_axis >= 0 && tk.depth < 56u) {
            const float split_cost = kTraversalCost + (node_area > 0.0f ? best_cost / node_area : (float)n);
            if (n <= kMaxLeaf && (float)n <= split_cost) { make_leaf(); continue; }
            const float ext = chi[best_axis] - clo[best_axis];
            const float scale = (float)kBins / ext;
            auto it = std::partition(t.begin() + tk.begin, t.begin() + tk.end, [&](const SahTri& x) {
                int b = std::min(kBins - 1, std::max(0, (int)((x.c[best_axis] - clo[best_axis]) * scale)));
                return b < best_bin;
            });
            mid = (uint32_t)(it - t.begin());
        } else {
            // all centroids coincide (or the tree got too deep): leaf if it fits, else split the range in half
            if (n <= kMaxLeaf) { make_leaf(); continue; }
            mid = tk.begin + n / 2;
            if (best_axis >= 0) {
                const int ax = best_axis;
                std::nth_element(t.begin() + tk.begin, t.begin() + mid, t.begin() + tk.end, [&](const SahTri& x, const SahTri& y) { return x.c[ax] < y.c[ax]; });
            }
        }
        if (mid == tk.begin || mid == tk.end) mid = tk.begin + n / 2;
        nd.a = (uint32_t)nodes.size();
        nd.b = nd.a + 1u;
        nodes[tk.node] = nd;
        nodes.push_back(spt_bvh_node{});
        nodes.push_back(spt_bvh_node{});
        st.push_back(Task{mid, tk.end, nd.b, tk.depth + 1u});
        st.push_back(Task{tk.begin, mid, nd.a, tk.depth + 1u});
    }
    for (uint32_t i = 0; i < tri_count; ++i) order[tri_first + i] = t[i].id;
    if (debug) {
        uint32_t hist[16] = {}, leaves = 0, inner = 0;
        for (size_t k = root_index; k < nodes.size(); ++k) {
            if (nodes[k].b & SPT_LEAF_FLAG) { ++leaves; ++hist[std::min(15u, nodes[k].b & ~SPT_LEAF_FLAG)]; }
            else ++inner;
        }
        std::fprintf(stderr, "[spt] device %s: %u items, %u inner nodes, %u leaves, leaf sizes 1:%u 2:%u 3:%u 4:%u >4:%u\n", what, tri_count, inner, leaves,
                     hist[1], hist[2], hist[3], hist[4], leaves - hist[1] - hist[2] - hist[3] - hist[4]);
    }
}

// Repack one 32-byte-node tree into 64-byte wide nodes (see trace.h).  Returns the index of the
// super-root inside `wide` (in wide-node units).  The first `bfs_nodes` wide nodes are numbered
// breadth-first (they are the ones staged into LDS for large scenes), the subtrees below them
// depth-first so that deep subtrees stay contiguous in memory.
uint32_t build_wide(const spt_bvh_node* nodes, uint32_t root, std::vector<float4>& wide, uint32_t bfs_nodes, const char* what, bool pad_boxes = false) {
    auto leaf_ref = [&](const spt_bvh_node& nd) -> uint32_t {
        uint32_t cnt = nd.b & ~SPT_LEAF_FLAG;
        if (cnt > 15u) fail(SPT_ERR_UNSUPPORTED, std::string(what) + ": BVH leaf with more than 15 items");
        if (nd.a >= (1u << 27)) fail(SPT_ERR_UNSUPPORTED, std::string(what) + ": more than 2^27 items");
        return kLeaf | (cnt << 27) | nd.a;
    };
    auto set_child = [&](uint32_t w, int side, const spt_bvh_node& ch, uint32_t ref) {
        float4* f = &wide[(size_t)w * 4];
        float4 lo = make_float4(ch.bmin[0], ch.bmin[1], ch.bmin[2], 0.0f), hi = make_float4(ch.bmax[0], ch.bmax[1], ch.bmax[2], 0.0f);
        if (pad_boxes && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z) {
            const float px = box_pad(lo.x, hi.x), py = box_pad(lo.y, hi.y), pz = box_pad(lo.z, hi.z);
            lo.x -= px; lo.y -= py; lo.z -= pz;
            hi.x += px; hi.y += py; hi.z += pz;
        }
        if (side == 0) { f[0].x = lo.x; f[0].y = lo.y; f[0].z = lo.z; f[1].x = hi.x; f[1].y = hi.y; f[1].z = hi.z; std::memcpy(&f[0].w, &ref, 4); }
        else { f[2] = lo; f[3] = hi; std::memcpy(&f[1].w, &ref, 4); }
    };
    auto new_wide = [&]() -> uint32_t {
        uint32_t w = (uint32_t)(wide.size() / 4);
        const float inf = std::numeric_limits<float>::infinity();
        wide.push_back(make_float4(inf, inf, inf, 0.0f));    // empty boxes: never hit
        wide.push_back(make_float4(-inf, -inf, -inf, 0.0f));
        wide.push_back(make_float4(inf, inf, inf, 0.0f));
        wide.push_back(make_float4(-inf, -inf, -inf, 0.0f));
        return w;
    };
    const uint32_t first = (uint32_t)(wide.size() / 4);
    const uint32_t super = new_wide();
    struct Item { uint32_t node, parent, side; };
    // breadth-first part
    std::vector<Item> frontier;
    frontier.push_back(Item{root, super, 0});
    size_t head = 0;
    while (head < frontier.size() && (uint32_t)(wide.size() / 4) - first < bfs_nodes) {
        Item it = frontier[head++];
        const spt_bvh_node& nd = nodes[it.node];
        if (nd.b & SPT_LEAF_FLAG) {
            set_child(it.parent, (int)it.side, nd, leaf_ref(nd));
        } else {
            const uint32_t w = new_wide();
            set_child(it.parent, (int)it.side, nd, w);
            frontier.push_back(Item{nd.a, w, 0});
            frontier.push_back(Item{nd.b, w, 1});
        }
    }
    // depth-first below the frontier
    for (size_t k = head; k < frontier.size(); ++k) {
        std::vector<Item> st;
        st.push_back(frontier[k]);
        while (!st.empty()) {
            Item it = st.back();
            st.pop_back();
            const spt_bvh_node& nd = nodes[it.node];
            if (nd.b & SPT_LEAF_FLAG) {
                set_child(it.parent, (int)it.side, nd, leaf_ref(nd));
            } else {
                const uint32_t w = new_wide();
                set_child(it.parent, (int)it.side, nd, w);
                st.push_back(Item{nd.b, w, 1});
                st.push_back(Item{nd.a, w, 0});
            }
        }
    }
    return super;
}

// Collapse a 2-ary tree of 32-byte nodes into compressed 4-wide nodes (see trace.h).  Returns the ref of
// the root (node index in `out` / 4, or a leaf ref).  Children boxes are quantised OUTWARD and verified
// with exactly the f32 decode arithmetic of node4_test.
// `stack_need` receives the worst-case number of simultaneously pending entries of a near-first walk: a
// node with n children leaves n - 1 of them pending while the first is descended, in whatever order.
// `base`: the node index of out[0] (spt_scene_update builds the streaming walker's TLAS into an array of its own that sits behind
// the BLAS nodes on the device).  `height`: receives the height of the root node (0: all its children are leaves, also for a
// root that is a leaf ref) - the number of levels above the lowest that a bottom-up refit of the tree takes.
uint32_t build_n4(const spt_bvh_node* nodes, uint32_t root, std::vector<float4>& out, uint32_t* stack_need, const char* what, uint32_t base = 0u,
                  uint32_t* height = nullptr) {
    *stack_need = 0;
    if (height) *height = 0;
    auto leaf_ref = [&](const spt_bvh_node& nd) -> uint32_t {
        uint32_t cnt = nd.b & ~SPT_LEAF_FLAG;
        if (cnt > 15u) fail(SPT_ERR_UNSUPPORTED, std::string(what) + ": BVH leaf with more than 15 items");
        if (nd.a >= (1u << 27)) fail(SPT_ERR_UNSUPPORTED, std::string(what) + ": more than 2^27 items");
        return kLeaf | (cnt << 27) | nd.a;
    };
    auto area = [&](const spt_bvh_node& nd) {
        float dx = nd.bmax[0] - nd.bmin[0], dy = nd.bmax[1] - nd.bmin[1], dz = nd.bmax[2] - nd.bmin[2];
        return dx * dy + dy * dz + dz * dx;
    };
    if (nodes[root].b & SPT_LEAF_FLAG) return leaf_ref(nodes[root]);
    struct Item { uint32_t node32, n4; };
    std::vector<Item> st;
    auto alloc = [&]() -> uint32_t {
        uint32_t i = base + (uint32_t)(out.size() / 4);
        out.resize(out.size() + 4, make_float4(0, 0, 0, 0));
        return i;
    };
    const uint32_t root_n4 = alloc();
    st.push_back(Item{root, root_n4});
    while (!st.empty()) {
        Item it = st.back();
        st.pop_back();
        const spt_bvh_node& par = nodes[it.node32];
        // gather up to 4 children by repeatedly opening the inner child with the largest box
        uint32_t ch[4] = {par.a, par.b, 0, 0};
        uint32_t n = 2;
        while (n < 4) {
            int best = -1;
            float best_area = -1.0f;
            for (uint32_t k = 0; k < n; ++k)
                if (!(nodes[ch[k]].b & SPT_LEAF_FLAG) && area(nodes[ch[k]]) > best_area) { best_area = area(nodes[ch[k]]); best = (int)k; }
            if (best < 0) break;
            const spt_bvh_node& open = nodes[ch[best]];
            ch[best] = open.a;
            ch[n++] = open.b;
        }
        // quantisation frame: p = parent min, scale = 2^e >= extent / 254
        uint32_t eb[3];
        float scale[3];
        for (int k = 0; k < 3; ++k) {
            float ext = par.bmax[k] - par.bmin[k];
            int e = -120;
            if (ext > 0.0f && std::isfinite(ext)) {
                e = (int)std::ceil(std::log2((double)ext / 254.0));
                if (e < -120) e = -120;
                if (e > 120) fail(SPT_ERR_UNSUPPORTED, std::string(what) + ": node extent too large to quantise");
            }
            eb[k] = (uint32_t)(e + 127);
            uint32_t bits = eb[k] << 23;
            std::memcpy(&scale[k], &bits, 4);
        }
        uint32_t qlo[3][4], qhi[3][4], refs[4] = {0, 0, 0, 0};
        for (uint32_t c = 0; c < 4; ++c)
            for (int k = 0; k < 3; ++k) { qlo[k][c] = 255u; qhi[k][c] = 0u; }   // absent child: empty box
        for (uint32_t c = 0; c < n; ++c) {
            const spt_bvh_node& cn = nodes[ch[c]];
            for (int k = 0; k < 3; ++k) {
                const float p = par.bmin[k];
                int lo = (int)std::floor(((double)cn.bmin[k] - (double)p) / (double)scale[k]);
                int hi = (int)std::ceil(((double)cn.bmax[k] - (double)p) / (double)scale[k]);
                lo = std::max(0, std::min(255, lo));
                hi = std::max(0, std::min(255, hi));
                // verify with the device's arithmetic: p + scale * q (f32 multiply, then f32 add)
                auto dec = [&](int q) { float m = scale[k] * (float)q; return p + m; };
                while (lo > 0 && dec(lo) > cn.bmin[k]) --lo;
                while (hi < 255 && dec(hi) < cn.bmax[k]) ++hi;
                if (dec(lo) > cn.bmin[k] || dec(hi) < cn.bmax[k]) fail(SPT_ERR_UNSUPPORTED, std::string(what) + ": cannot quantise a child box conservatively");
                qlo[k][c] = (uint32_t)lo;
                qhi[k][c] = (uint32_t)hi;
            }
            if (cn.b & SPT_LEAF_FLAG) {
                refs[c] = leaf_ref(cn);
            } else {
                refs[c] = alloc();
                st.push_back(Item{ch[c], refs[c]});
            }
        }
        auto pack4 = [](const uint32_t q[4]) { return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24); };
        auto as_f = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
        float4* f = &out[(size_t)(it.n4 - base) * 4];
        f[0] = make_float4(par.bmin[0], par.bmin[1], par.bmin[2], as_f(eb[0] | (eb[1] << 8) | (eb[2] << 16) | (n << 24)));
        f[1] = make_float4(as_f(pack4(qlo[0])), as_f(pack4(qlo[1])), as_f(pack4(qlo[2])), as_f(pack4(qhi[0])));
        f[2] = make_float4(as_f(pack4(qhi[1])), as_f(pack4(qhi[2])), as_f(refs[0]), as_f(refs[1]));
        f[3] = make_float4(as_f(refs[2]), as_f(refs[3]), 0.0f, 0.0f);
    }
    // children are allocated after their parent, so one reverse sweep sees every child before its parent
    const uint32_t end_n4 = base + (uint32_t)(out.size() / 4);
    std::vector<uint32_t> need(end_n4 - root_n4, 0u), hgt(height ? end_n4 - root_n4 : 0u, 0u);
    for (uint32_t i = end_n4; i-- > root_n4;) {
        const float4* f = &out[(size_t)(i - base) * 4];
        uint32_t hdr, refs[4];
        std::memcpy(&hdr, &f[0].w, 4);
        std::memcpy(&refs[0], &f[2].z, 4);
        std::memcpy(&refs[1], &f[2].w, 4);
        std::memcpy(&refs[2], &f[3].x, 4);
        std::memcpy(&refs[3], &f[3].y, 4);
        const uint32_t n = hdr >> 24;
        uint32_t deepest = 0;
        for (uint32_t c = 0; c < n; ++c)
            if (!(refs[c] & kLeaf)) {
                deepest = std::max(deepest, need[refs[c] - root_n4]);
                if (height) hgt[i - root_n4] = std::max(hgt[i - root_n4], hgt[refs[c] - root_n4] + 1u);
            }
        need[i - root_n4] = n - 1 + deepest;
    }
    *stack_need = need[0];
    if (height) *height = hgt[0];
    return root_n4;
}

bool surface_emits(const spt_surface& sf) { return 0.299f * sf.emissive[0] + 0.587f * sf.emissive[1] + 0.114f * sf.emissive[2] > 0.0f; }

}  // namespace

DynView dyn_view(const spt_scene_desc& s, const uint8_t* surf_emissive) {
    return DynView{s.aggregate, s.light_sampler, s.n_tlas_nodes, s.n_instances, s.n_lights, s.n_spheres, s.n_meshes, s.n_bezier_patches, s.n_surfaces,
                   s.env.width != 0 && s.env.height != 0, s.tlas_nodes, s.instances, s.lights, s.light_alias, surf_emissive};
}

// The checks of the arrays an update replaces: spt_scene_create ("scene desc") and spt_scene_update ("scene_update") share them
void validate_instances(const DynView& s, const BuildOptions& opt, const char* who) {
    const std::string w(who);
    for (uint32_t i = 0; i < s.n_instances; ++i) {
        const spt_instance& in = s.instances[i];
        if (in.prim_type == SPT_PRIM_SPHERE) {
            if (in.prim_id >= s.n_spheres) fail(SPT_ERR_INVALID_ARG, w + ": instance sphere index out of range");
        } else if (in.prim_type == SPT_PRIM_MESH) {
            if (in.prim_id >= s.n_meshes) fail(SPT_ERR_INVALID_ARG, w + ": instance mesh index out of range");
        } else if (in.prim_type == SPT_PRIM_BEZIER) {
            if (!opt.with_bezier) fail(SPT_ERR_UNSUPPORTED, w + ": Bezier instances are served by libspt_hip_bez.so");   // not reached: spt_scene_create forwards
            if (in.prim_id >= s.n_bezier_patches) fail(SPT_ERR_INVALID_ARG, w + ": instance Bezier patch index out of range");
            // CubicBezier::sample / pdf / surface_area are `unimplemented!` in the reference (bezier.rs:180-190)
            if (in.light >= 0) fail(SPT_ERR_UNSUPPORTED, w + ": a Bezier patch cannot be a shape light");
        } else {
            fail(SPT_ERR_INVALID_ARG, w + ": bad instance prim_type");
        }
        if (in.surface >= s.n_surfaces) fail(SPT_ERR_INVALID_ARG, w + ": instance surface index out of range");
        if (in.light >= (int32_t)s.n_lights) fail(SPT_ERR_INVALID_ARG, w + ": instance light index out of range");
        if (in.light >= 0 && (s.lights[in.light].type != SPT_LIGHT_SHAPE || s.lights[in.light].instance != i))
            fail(SPT_ERR_INVALID_ARG, w + ": instance light does not name the shape light of this instance");
        // pdf_shape_light of the power_is sampler looks the instance up in its light map (power_is.rs:84-86; the reference
        // panics on a missing key): an emissive instance that is not a light would index light_alias.props[-1]
        if (s.light_sampler == SPT_LIGHT_SAMPLER_POWER_IS && in.light < 0) {
            if (s.surf_emissive[in.surface])
                fail(SPT_ERR_INVALID_ARG, w + ": power_is light sampler and an emissive instance without a shape light");
        }
    }
}

void validate_lights(const DynView& s, const char* who) {
    const std::string w(who);
    for (uint32_t i = 0; i < s.n_lights; ++i) {
        const spt_light& l = s.lights[i];
        if (l.type > SPT_LIGHT_ENV) fail(SPT_ERR_INVALID_ARG, w + ": unknown light type");
        if (l.type == SPT_LIGHT_SHAPE && l.instance >= s.n_instances) fail(SPT_ERR_INVALID_ARG, w + ": shape light instance out of range");
        if (l.type == SPT_LIGHT_ENV && !s.has_env) fail(SPT_ERR_INVALID_ARG, w + ": env light without env map");
    }
}

void validate_light_alias(const DynView& s, const char* who) {
    const std::string w(who);
    if (s.light_sampler == SPT_LIGHT_SAMPLER_POWER_IS && s.n_lights) {
        if (s.light_alias.n != s.n_lights || !s.light_alias.props || !s.light_alias.u || !s.light_alias.k)
            fail(SPT_ERR_INVALID_ARG, w + ": power_is sampler needs an alias table over the lights");
        for (uint32_t i = 0; i < s.n_lights; ++i)
            if (s.light_alias.k[i] >= s.n_lights) fail(SPT_ERR_INVALID_ARG, w + ": light alias index out of range");
    }
}

void validate(const spt_scene_desc& s, const BuildOptions& opt) {
    if (s.abi_version != SPT_ABI_VERSION) fail(SPT_ERR_INVALID_ARG, "scene desc: abi_version mismatch");
    if (s.aggregate > SPT_AGGREGATE_BVH) fail(SPT_ERR_INVALID_ARG, "scene desc: bad aggregate");
    auto need = [](const void* p, uint32_t n, const char* what) {
        if (n && !p) fail(SPT_ERR_INVALID_ARG, std::string("scene desc: null array '") + what + "'");
    };
    need(s.tlas_nodes, s.n_tlas_nodes, "tlas_nodes");
    need(s.instances, s.n_instances, "instances");
    need(s.meshes, s.n_meshes, "meshes");
    need(s.blas_nodes, s.n_blas_nodes, "blas_nodes");
    need(s.tri_pos, s.n_tris, "tri_pos");
    need(s.tri_attr, s.n_tris, "tri_attr");
    need(s.spheres, s.n_spheres, "spheres");
    need(s.bezier_patches, s.n_bezier_patches, "bezier_patches");
    for (uint32_t i = 0; i < s.n_bezier_patches; ++i) {
        const float method = s.bezier_patches[i].cp[0][0][3];
        if (method != 0.0f && method != SPT_BEZIER_NEWTON) fail(SPT_ERR_INVALID_ARG, "scene desc: unknown Bezier intersection method (cp[0][0][3])");
    }
    need(s.surfaces, s.n_surfaces, "surfaces");
    need(s.materials, s.n_materials, "materials");
    need(s.mediums, s.n_mediums, "mediums");
    need(s.lights, s.n_lights, "lights");
    if (s.n_instances && s.aggregate == SPT_AGGREGATE_BVH && s.n_tlas_nodes == 0)
        fail(SPT_ERR_INVALID_ARG, "scene desc: bvh aggregate without TLAS nodes");
    std::vector<uint8_t> emissive(s.n_surfaces, 0);
    for (uint32_t i = 0; i < s.n_surfaces; ++i) emissive[i] = surface_emits(s.surfaces[i]) ? 1 : 0;
    const DynView v = dyn_view(s, emissive.data());
    validate_instances(v, opt, "scene desc");
    for (uint32_t i = 0; i < s.n_meshes; ++i) {
        const spt_mesh& m = s.meshes[i];
        if (m.root >= s.n_blas_nodes || (uint64_t)m.tri_first + m.tri_count > s.n_tris || m.tri_count == 0)
            fail(SPT_ERR_INVALID_ARG, "scene desc: mesh ranges out of bounds");
    }
    for (uint32_t i = 0; i < s.n_surfaces; ++i) {
        if (s.surfaces[i].material >= s.n_materials) fail(SPT_ERR_INVALID_ARG, "scene desc: surface material out of range");
        if (s.surfaces[i].inside_medium >= (int32_t)s.n_mediums) fail(SPT_ERR_INVALID_ARG, "scene desc: surface medium out of range");
        if (s.surfaces[i].inside_medium >= 254) fail(SPT_ERR_UNSUPPORTED, "scene desc: more than 254 mediums");
    }
    for (uint32_t i = 0; i < s.n_materials; ++i) {
        if (s.materials[i].bxdf > SPT_BXDF_SPECULAR_PLASTIC) fail(SPT_ERR_INVALID_ARG, "scene desc: unknown bxdf tag");   // SPT_BXDF_PNDF_CONDUCTOR only exists per hit
        if (s.materials[i].recipe > s.n_material_recipes) fail(SPT_ERR_INVALID_ARG, "scene desc: material recipe out of range");
    }
    need(s.textures, s.n_textures, "textures");
    need(s.images, s.n_images, "images");
    need(s.image_levels, s.n_image_levels, "image_levels");
    need(s.texels, s.n_texels, "texels");
    need(s.material_recipes, s.n_material_recipes, "material_recipes");
    for (uint32_t i = 0; i < s.n_images; ++i) {
        const spt_image& im = s.images[i];
        if (im.n_levels == 0 || (uint64_t)im.first_level + im.n_levels > s.n_image_levels) fail(SPT_ERR_INVALID_ARG, "scene desc: image level range out of bounds");
    }
    for (uint32_t i = 0; i < s.n_image_levels; ++i) {
        const spt_image_level& L = s.image_levels[i];
        if (L.width == 0 || L.height == 0 || (uint64_t)L.width * L.height > 0x7fffffffull ||
            (uint64_t)L.first_texel + (uint64_t)L.width * L.height > s.n_texels)
            fail(SPT_ERR_INVALID_ARG, "scene desc: image level texels out of bounds");
    }
    for (uint32_t i = 0; i < s.n_textures; ++i) {
        const spt_texture& t = s.textures[i];
        if (t.type > SPT_TEX_MODIFIER) fail(SPT_ERR_INVALID_ARG, "scene desc: unknown texture type");
        if (t.type == SPT_TEX_IMAGE && t.image >= s.n_images) fail(SPT_ERR_INVALID_ARG, "scene desc: texture image out of range");
        const bool unary = t.type == SPT_TEX_SRGB || t.type == SPT_TEX_MODIFIER, binary = t.type >= SPT_TEX_ADD && t.type <= SPT_TEX_DIV;
        if ((unary || binary) && t.a >= i) fail(SPT_ERR_INVALID_ARG, "scene desc: texture child must precede its parent");
        if (binary && t.b >= i) fail(SPT_ERR_INVALID_ARG, "scene desc: texture child must precede its parent");
        if (t.type == SPT_TEX_MODIFIER && (t.mode > SPT_TEXMODE_BITANGENT || t.wrap > SPT_TEXWRAP_MIRROR_CLAMP))
            fail(SPT_ERR_INVALID_ARG, "scene desc: bad texture input mode / wrap");
    }
    for (uint32_t i = 0; i < s.n_material_recipes; ++i) {
        const spt_material_recipe& r = s.material_recipes[i];
        if (r.type > SPT_MAT_PNDF_PLASTIC || r.rough_chan > SPT_CHAN_A || r.metal_chan > SPT_CHAN_A) fail(SPT_ERR_INVALID_ARG, "scene desc: bad material recipe");
        for (int k = 0; k < 4; ++k) {
            if (r.type >= SPT_MAT_PNDF_CONDUCTOR && k == 1) {
                if (r.tex[k] >= s.n_pndfs) fail(SPT_ERR_INVALID_ARG, "scene desc: material recipe P-NDF out of range");
            } else if (r.tex[k] >= s.n_textures) {
                fail(SPT_ERR_INVALID_ARG, "scene desc: material recipe texture out of range");
            }
        }
    }
    // position-normal distributions: every index the per-hit tree walks of include/spt_pndf.h follow
    need(s.pndfs, s.n_pndfs, "pndfs");
    need(s.pndf_terms, s.n_pndf_terms, "pndf_terms");
    need(s.pndf_nodes, s.n_pndf_nodes, "pndf_nodes");
    need(s.pndf_refs, s.n_pndf_refs, "pndf_refs");
    need(s.pndf_roots, s.n_pndf_roots, "pndf_roots");
    for (uint32_t i = 0; i < s.n_pndf_refs; ++i)
        if (s.pndf_refs[i] >= s.n_pndf_terms) fail(SPT_ERR_INVALID_ARG, "scene desc: P-NDF term reference out of range");
    for (uint32_t i = 0; i < s.n_pndf_nodes; ++i) {
        const spt_pndf_node& n = s.pndf_nodes[i];
        const bool leaf = n.lc == 0xffffffffu;
        // children behind their parent: no walk can cycle
        if (!leaf && (n.lc <= i || n.rc <= i || n.lc >= s.n_pndf_nodes || n.rc >= s.n_pndf_nodes)) fail(SPT_ERR_INVALID_ARG, "scene desc: P-NDF node children out of order");
        if (n.start > n.end || n.end > s.n_pndf_refs) fail(SPT_ERR_INVALID_ARG, "scene desc: P-NDF node range out of bounds");
    }
    {
        // the leaves' ranges are relative to their tree's first ref: one pass over every tree
        // ... and every node belongs to exactly ONE tree and is reached once (a shared child would make this walk - and a
        // DAG-shaped descriptor the device's - exponential), at a depth the walks' fixed stacks hold: spt_pndf_calc /
        // spt_pndf_uv_walk pop one node and push two, so an inner node at depth d (root = 1) leaves d + 1 entries pending;
        // beyond SPT_PNDF_STACK they would drop subtrees silently (a wrong density, not an error)
        std::vector<std::pair<uint32_t, uint32_t>> todo;
        std::vector<uint8_t> seen(s.n_pndf_nodes, 0);
        auto check_tree = [&](uint32_t root, uint32_t first_ref) {
            if (root == 0xffffffffu) return;
            if (root >= s.n_pndf_nodes || first_ref > s.n_pndf_refs) fail(SPT_ERR_INVALID_ARG, "scene desc: P-NDF tree root out of range");
            todo.assign(1, std::make_pair(root, 1u));
            while (!todo.empty()) {
                const uint32_t ni = todo.back().first, depth = todo.back().second;
                todo.pop_back();
                if (seen[ni]) fail(SPT_ERR_INVALID_ARG, "scene desc: a P-NDF node is reachable twice (trees must not share nodes)");
                seen[ni] = 1;
                const spt_pndf_node& n = s.pndf_nodes[ni];
                if ((uint64_t)first_ref + n.end > s.n_pndf_refs) fail(SPT_ERR_INVALID_ARG, "scene desc: P-NDF leaf range out of bounds");
                if (n.lc != 0xffffffffu) {
                    if (depth + 1u > SPT_PNDF_STACK) fail(SPT_ERR_UNSUPPORTED, "scene desc: P-NDF tree deeper than the walks' stack (" + std::to_string(SPT_PNDF_STACK) + " pending entries)");
                    todo.emplace_back(n.lc, depth + 1u);
                    todo.emplace_back(n.rc, depth + 1u);
                }
            }
        };
        for (uint32_t i = 0; i < s.n_pndfs; ++i) {
            const spt_pndf& pd = s.pndfs[i];
            if (pd.n_terms == 0 || (uint64_t)pd.first_term + pd.n_terms > s.n_pndf_terms) fail(SPT_ERR_INVALID_ARG, "scene desc: P-NDF term range out of bounds");
            if (pd.s_block_count == 0 || pd.s_block_count > 4096u || (uint64_t)pd.first_root + 2ull * pd.s_block_count * pd.s_block_count > s.n_pndf_roots)
                fail(SPT_ERR_INVALID_ARG, "scene desc: P-NDF block table out of bounds");
            for (uint32_t b = 0; b < pd.s_block_count * pd.s_block_count; ++b) check_tree(s.pndf_roots[pd.first_root + 2u * b], s.pndf_roots[pd.first_root + 2u * b + 1u]);
            check_tree(pd.uv_root, pd.uv_first_ref);
        }
    }
    for (uint32_t i = 0; i < s.n_surfaces; ++i)
        if (s.surfaces[i].normal_map > s.n_textures || s.surfaces[i].emissive_map > s.n_textures)
            fail(SPT_ERR_INVALID_ARG, "scene desc: surface map out of range");
    validate_lights(v, "scene desc");
    if (s.env_light_index >= (int32_t)s.n_lights) fail(SPT_ERR_INVALID_ARG, "scene desc: env_light_index out of range");
    if (s.light_sampler > SPT_LIGHT_SAMPLER_POWER_IS) fail(SPT_ERR_INVALID_ARG, "scene desc: bad light_sampler");
    validate_light_alias(v, "scene desc");
    if (s.env.width || s.env.height) {
        uint64_t n = (uint64_t)s.env.width * s.env.height;
        if (n == 0 || n > 0x7fffffffull) fail(SPT_ERR_INVALID_ARG, "scene desc: bad env size");
        if (!s.env.texels || !s.env.alias.props || !s.env.alias.u || !s.env.alias.k || s.env.alias.n != n)
            fail(SPT_ERR_INVALID_ARG, "scene desc: env map needs texels and an alias table");
        for (uint64_t i = 0; i < n; ++i)
            if (s.env.alias.k[i] >= n) fail(SPT_ERR_INVALID_ARG, "scene desc: env alias index out of range");
    }
}

// ---- the instance-dependent part of a scene (spt_scene_create, spt_scene_update) ----------------------------------------
namespace {

uint8_t shade_class(const spt_scene_desc& s, const spt_material& m) {
    // the class a hit is queued under for the shade stage of bounce >= 1 (kernels.h, kClasses): by the code path its material
    // takes through mat_sample / mat_eval / mat_pdf and by whether it has a light sample at all
    uint32_t b = m.bxdf;
    if (m.recipe != 0u) {      // evaluated per hit: the kind the recipe usually resolves to
        switch (s.material_recipes[m.recipe - 1u].type) {
        case SPT_MAT_LAMBERT: b = SPT_BXDF_LAMBERT; break;
        case SPT_MAT_CONDUCTOR: b = SPT_BXDF_MICROFACET_CONDUCTOR; break;
        case SPT_MAT_DIELECTRIC: b = SPT_BXDF_MICROFACET_DIELECTRIC; break;
        default: b = SPT_BXDF_MICROFACET_PLASTIC; break;
        }
    }
    switch (b) {
    case SPT_BXDF_LAMBERT: return 0;
    case SPT_BXDF_MICROFACET_CONDUCTOR: return 1;
    case SPT_BXDF_SPECULAR_CONDUCTOR: return 2;
    case SPT_BXDF_MICROFACET_DIELECTRIC: return 3;
    case SPT_BXDF_SPECULAR_DIELECTRIC: return 4;
    case SPT_BXDF_PSEUDO: return 5;
    default: return 6;       // the plastic / PBR lobes, glints
    }
}

bool only_delta_lights(const DynView& s) {
    bool delta = true;
    for (uint32_t i = 0; i < s.n_lights; ++i) delta = delta && s.lights[i].type <= SPT_LIGHT_SPOT;
    return delta;
}

// The trees over the instances, the streaming walker's entries and the instances' classes.
void dyn_trees(const SceneFixed& fx, const DynView& s, const BuildOptions& opt, bool n4, SceneDynamic& dy) {
    // stack need: reference-order traversal holds at most depth+1 entries per level of nesting
    uint32_t tlas_depth = 0;
    if (s.aggregate == SPT_AGGREGATE_BVH) tlas_depth = bvh_depth(s.tlas_nodes, s.n_tlas_nodes, 0, s.n_instances, "tlas");
    // near-first traversal pushes at most one (far) child per 2-wide level (4-wide trees: see build_n4)
    const uint32_t cap = tlas_depth + fx.blas_depth + 2;
    if (!fx.own_bvh && cap > kLdsStack + kSpillStack) fail(SPT_ERR_UNSUPPORTED, "BVH deeper than the traversal stack (48 levels)");
    if (tlas_depth + 2 > kLdsStack + kSpillStack) fail(SPT_ERR_UNSUPPORTED, "TLAS deeper than the traversal stack (48 levels)");
    dy.stack_cap = cap;
    dy.n_tlas_nodes = s.n_tlas_nodes;
    dy.cls.assign(std::max<uint32_t>(s.n_instances, 1u), 0);
    for (uint32_t i = 0; i < s.n_instances; ++i) dy.cls[i] = fx.surf_class[s.instances[i].surface];
    dy.wtlas.clear();
    dy.tlas_root = 0;
    for (int k = 0; k < 3; ++k) { dy.tlas_lo[k] = 0.0f; dy.tlas_hi[k] = 0.0f; }
    // TLAS leaf slot -> instance index: identity for the caller's tree (its leaves index the instance array) and
    // for a GROUP aggregate, the leaf order of the device-built tree otherwise
    dy.tlas_order.resize(s.n_instances);
    for (uint32_t i = 0; i < s.n_instances; ++i) dy.tlas_order[i] = i;
    std::vector<spt_bvh_node> own_tlas;
    if (s.aggregate == SPT_AGGREGATE_BVH && s.n_tlas_nodes) {
        if (fx.own_bvh && s.n_instances) {
            build_sah_tlas(s.instances, s.n_instances, opt, own_tlas, dy.tlas_order);   // boxes padded by the builder
            tlas_depth = bvh_depth(own_tlas.data(), (uint32_t)own_tlas.size(), 0, s.n_instances, "device tlas");
            if (tlas_depth + 2 > kLdsStack + kSpillStack) fail(SPT_ERR_UNSUPPORTED, "device TLAS deeper than the traversal stack (48 levels)");
        }
        const spt_bvh_node* tlas_src = own_tlas.empty() ? s.tlas_nodes : own_tlas.data();
        const uint32_t sup = build_wide(tlas_src, 0, dy.wtlas, 0xffffffffu, "tlas", false);
        std::memcpy(&dy.tlas_root, &dy.wtlas[(size_t)sup * 4].w, 4);      // left child of the super-root = real root
        for (int k = 0; k < 3; ++k) { dy.tlas_lo[k] = tlas_src[0].bmin[k]; dy.tlas_hi[k] = tlas_src[0].bmax[k]; }
    }
    if (fx.own_bvh && fx.n_meshes && tlas_depth + fx.own_blas_depth + 2 > kLdsStack + kSpillStack)
        fail(SPT_ERR_UNSUPPORTED, "device BVH deeper than the traversal stack (48 levels)");
    if (n4 && fx.n_meshes && tlas_depth + fx.max_blas_need + 2 > kLdsStack + kSpillStack)
        fail(SPT_ERR_UNSUPPORTED, "4-wide BVH needs more than the traversal stack (48 entries)");
    // streaming walker (stream.h): a 4-wide TLAS behind the BLAS nodes (refs of both levels index one array) and
    // 96-byte instance entry records in its leaf order.  Its boxes only cull (quantised outward, relaxed
    // test), so one tree serves both BVH modes and a GROUP aggregate alike.
    dy.swalk = false;
    dy.s_root = 0u;
    dy.stlas.clear();
    dy.sinst.clear();
    if (n4 && s.n_instances) {
        try {
            std::vector<spt_bvh_node> group_tlas;
            std::vector<uint32_t> s_order = dy.tlas_order;
            const spt_bvh_node* src = nullptr;
            if (s.aggregate == SPT_AGGREGATE_BVH && s.n_tlas_nodes) {
                src = own_tlas.empty() ? s.tlas_nodes : own_tlas.data();
            } else {
                build_sah_tlas(s.instances, s.n_instances, opt, group_tlas, s_order);
                src = group_tlas.data();
                for (int k = 0; k < 3; ++k) { dy.tlas_lo[k] = src[0].bmin[k]; dy.tlas_hi[k] = src[0].bmax[k]; }
            }
            uint32_t need_t = 0;
            dy.s_root = build_n4(src, 0, dy.stlas, &need_t, "tlas", fx.blas_f4 / 4u);
            // + 1: a TLAS leaf of several instances keeps its remaining instances as one extra entry
            if (need_t + fx.max_blas_need + 3 > kLdsStack + kSpillStack) fail(SPT_ERR_UNSUPPORTED, "4-wide TLAS + BLAS need more than the traversal stack");
            dy.sinst.assign((size_t)s.n_instances * 6, make_float4(0, 0, 0, 0));
            auto as_f = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
            for (uint32_t slot = 0; slot < s.n_instances; ++slot) {
                const uint32_t ii = s_order[slot];
                const spt_instance& in = s.instances[ii];
                float4* r = &dy.sinst[(size_t)slot * 6];
                std::memcpy(r, in.inv, 48);
                r[3] = make_float4(as_f(ii), as_f(in.prim_type), as_f(in.prim_id), 0.0f);
                if (in.prim_type == SPT_PRIM_MESH) { r[4] = fx.mesh_rec[2 * in.prim_id]; r[5] = fx.mesh_rec[2 * in.prim_id + 1]; }
                else if (in.prim_type == SPT_PRIM_SPHERE) { const spt_sphere& sp = fx.spheres[in.prim_id]; r[4] = make_float4(sp.center[0], sp.center[1], sp.center[2], sp.radius); }
            }
            dy.swalk = opt.stream;
            // (patches under the caller's exact boxes: only the reference's visit order reproduces which near misses it loses)
            if (!fx.own_bvh && fx.n_bezier_patches != 0) dy.swalk = false;
        } catch (const AbiError&) {
            dy.stlas.clear();   // e.g. an instance box too large to quantise: the walkers of trace.h serve the scene
            dy.sinst.clear();
            dy.swalk = false;
        }
    }
}

// Where the sections of the traversal blob sit, in float4.  LDS-resident form: [sinst | tlas | instances | meshes | spheres | blas |
// tri | order] and, when they fit, the shading tables [attr | surfaces | materials | lights].  Large-scene form (n4): the sections
// an update keeps first, [meshes | spheres | tri | blas], then the ones it rewrites in place, [4-wide TLAS | sinst | tlas |
// instances | order] (the 4-wide TLAS directly behind the BLAS nodes: refs of both levels index one array from o_blas).
// Returns the length without the tables.
size_t dyn_layout(const SceneFixed& fx, SceneDynamic& dy, bool n4, bool tables) {
    auto f4 = [](size_t bytes) { return (bytes + 15) / 16; };
    size_t at = 0;
    auto put = [&](size_t n) { const size_t off = at; at += n; return (uint32_t)off; };
    const size_t n = fx.n_instances;
    const size_t inst_f4 = f4(n * sizeof(spt_instance)), mesh_f4 = fx.mesh_rec.size(), sph_f4 = f4((size_t)fx.n_spheres * sizeof(spt_sphere)),
                 tri_f4 = f4((size_t)fx.n_tris * sizeof(spt_tri_pos)), ord_f4 = f4(n * sizeof(uint32_t));
    if (!n4) {
        dy.o_sinst = put(dy.sinst.size());
        dy.o_tlas = put(dy.wtlas.size());
        dy.o_inst = put(inst_f4);
        dy.o_mesh = put(mesh_f4);
        dy.o_sph = put(sph_f4);
        dy.o_blas = put(fx.blas_f4);
        dy.o_tri = put(tri_f4);
        dy.o_tord = put(ord_f4);
    } else {
        dy.o_mesh = put(mesh_f4);
        dy.o_sph = put(sph_f4);
        dy.o_tri = put(tri_f4);
        dy.o_blas = put(fx.blas_f4);
        if (at > 0x7fffffffull / 16) fail(SPT_ERR_UNSUPPORTED, "scene geometry larger than 32 GiB");
        dy.tail_first = (uint32_t)at;
        put(dy.stlas.size());
        dy.o_sinst = put(dy.sinst.size());
        dy.o_tlas = put(dy.wtlas.size());
        dy.o_inst = put(inst_f4);
        dy.o_tord = put(ord_f4);
    }
    const size_t plain = at;
    dy.o_attr = dy.o_surf = dy.o_mat = dy.o_light = 0;
    if (tables) {
        dy.o_attr = put(fx.attr_sec.size());
        dy.o_surf = put(fx.surf_sec.size());
        dy.o_mat = put(fx.mat_sec.size());
        dy.o_light = put(f4((size_t)fx.n_lights * sizeof(spt_light)));
    }
    if (at > 0x7fffffffull / 16) fail(SPT_ERR_UNSUPPORTED, "scene geometry larger than 32 GiB");
    dy.geo_f4 = (uint32_t)at;
    return plain;
}


// Writes the sections from float4 `first` on into dy.blob (first = 0: the whole blob, which needs `st`).
void dyn_fill(const SceneFixed& fx, const DynView& s, SceneDynamic& dy, bool n4, uint32_t first, const StaticSections* st) {
    dy.blob.assign((size_t)dy.geo_f4 - first, make_float4(0, 0, 0, 0));
    auto write = [&](uint32_t off, const void* src, size_t bytes) {
        if (bytes) std::memcpy(&dy.blob[off - first], src, bytes);
    };
    if (first == 0 && st) {   // (no `st` at 0: a large scene without static sections)
        write(dy.o_mesh, fx.mesh_rec.data(), fx.mesh_rec.size() * 16);
        write(dy.o_sph, fx.spheres.data(), fx.spheres.size() * sizeof(spt_sphere));
        write(dy.o_blas, st->wblas, (size_t)fx.blas_f4 * 16);
        write(dy.o_tri, st->tri, (size_t)fx.n_tris * sizeof(spt_tri_pos));
    }
    if (n4) write(dy.o_blas + fx.blas_f4, dy.stlas.data(), dy.stlas.size() * 16);
    write(dy.o_sinst, dy.sinst.data(), dy.sinst.size() * 16);
    write(dy.o_tlas, dy.wtlas.data(), dy.wtlas.size() * 16);
    {   // the instance records as they are, pad[0] carrying the instance's class (hit_push<true> reads it from the staged copy)
        std::vector<spt_instance> inst_copy(s.instances, s.instances + s.n_instances);
        for (uint32_t i = 0; i < s.n_instances; ++i) { const uint32_t c = dy.cls[i]; std::memcpy(&inst_copy[i].pad[0], &c, 4); }
        write(dy.o_inst, inst_copy.data(), (size_t)s.n_instances * sizeof(spt_instance));
    }
    write(dy.o_tord, dy.tlas_order.data(), dy.tlas_order.size() * sizeof(uint32_t));
    if (dy.lds_tables) {
        write(dy.o_attr, fx.attr_sec.data(), fx.attr_sec.size() * 16);
        write(dy.o_surf, fx.surf_sec.data(), fx.surf_sec.size() * 16);
        write(dy.o_mat, fx.mat_sec.data(), fx.mat_sec.size() * 16);
        write(dy.o_light, s.lights, (size_t)s.n_lights * sizeof(spt_light));
    }
}

// The choices that follow from the instances and the lights once the form of the geometry is known (`plain_f4`: the blob without
// the shading tables), and the layout with the tables when they fit.
void dyn_decide(const SceneFixed& fx, const DynView& s, const BuildOptions& opt, SceneDynamic& dy, bool lds_geo, size_t plain_f4, size_t n_blas_ranges) {
    // a handful of primitives: every lane tests all of them (flat.h) instead of walking the trees.  The budget is in
    // triangle tests per ray (an instanced mesh counts once per instance, a sphere as one); SPT_FLAT_BUDGET=0 turns it off.
    {
        uint64_t cost = 0;
        bool ok = lds_geo && fx.own_bvh && fx.n_bezier_patches == 0 && fx.n_tris < 65536u;   // (the caller's exact trees are walked as they are)
        for (uint32_t i = 0; i < s.n_instances && ok; ++i) {
            const spt_instance& in = s.instances[i];
            if (in.prim_type == SPT_PRIM_MESH) cost += fx.mesh_tris[in.prim_id];
            else if (in.prim_type == SPT_PRIM_SPHERE) cost += 1;
            else ok = false;
        }
        dy.flat = ok && s.n_instances != 0 && cost <= opt.flat_budget ? 1u : 0u;
    }
    const bool delta_lights = only_delta_lights(s);
    // fused bounces (k_shade<0, ., kFused>): LDS-resident geometry + the lean simple-scene shade kernel, and
    // the shading tables must fit behind the geometry too (see tab_ld in shading.h)
    dy.lds_tables = lds_geo && lds_fits(plain_f4, fx.tables_bytes);
    dy.fused = dy.lds_tables && fx.fused_fixed && delta_lights;
    dy.simple = fx.simple_fixed && delta_lights;
    if (dy.lds_tables) dyn_layout(fx, dy, false, true);
    {   // eye.h: an eye-relative copy per camera position is possible when every box has ONE origin to be relative to
        bool ok = lds_geo && fx.own_bvh && fx.n_bezier_patches == 0 && fx.n_tris < 65536u && s.n_instances != 0 && opt.eye_blob;
        std::vector<uint32_t> mesh_uses(fx.n_meshes, 0u);
        for (uint32_t i = 0; i < s.n_instances && ok; ++i) {
            const spt_instance& in = s.instances[i];
            if (in.prim_type == SPT_PRIM_MESH) ok = ++mesh_uses[in.prim_id] == 1u;
            else ok = in.prim_type == SPT_PRIM_SPHERE;   // (a sphere's relative centre rides in its instance record: primitives may be shared)
        }
        const size_t eye_bytes = ((size_t)dy.geo_f4 + fx.n_tris) * 16;
        dy.eye_ok = ok && eye_bytes <= 36u * 1024u && kStackBytes + eye_bytes <= 64u * 1024u && n_blas_ranges == fx.n_meshes;
    }
}

// The bounding sphere of all instance boxes, their union and the 8 world-space corners of every instance's object-space box
void dyn_bounds(const SceneFixed& fx, const DynView& s, SceneDynamic& dy) {
    dy.bs_valid = false;
    dy.hull_corners.clear();
    if (!s.n_instances) return;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    bool finite = true;
    for (uint32_t i = 0; i < s.n_instances; ++i) {
        const double margin = bezier_box_margin(s.instances[i]);   // the screen-space bound and the bounding sphere cull too
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], (double)s.instances[i].bmin[k] - margin);
            hi[k] = std::max(hi[k], (double)s.instances[i].bmax[k] + margin);
            finite = finite && std::isfinite(s.instances[i].bmin[k]) && std::isfinite(s.instances[i].bmax[k]);
        }
    }
    double r2 = 0;
    for (int k = 0; k < 3; ++k) {
        dy.bs_center[k] = 0.5 * (lo[k] + hi[k]);
        dy.world_lo[k] = lo[k];
        dy.world_hi[k] = hi[k];
        r2 += 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]);
    }
    dy.bs_radius = std::sqrt(r2) * 1.001 + 1e-4;
    dy.bs_valid = finite && std::isfinite(dy.bs_radius) && dy.bs_radius < 1e18;
    // Object-space boxes for the per-row spans: the exact bounds of a mesh's vertices / a sphere (kept from creation), padded
    // a little, carried to world space by the instance matrix (a rotated cube's world AABB is far larger than its silhouette).
    // Patches keep their (margin-widened) world box: the clipping test accepts near misses (bezier_box_margin).
    if (dy.bs_valid && s.n_instances <= 256u) {
        dy.hull_corners.resize(s.n_instances);
        for (uint32_t i = 0; i < s.n_instances && !dy.hull_corners.empty(); ++i) {
            const spt_instance& in = s.instances[i];
            double olo[3] = {1e300, 1e300, 1e300}, ohi[3] = {-1e300, -1e300, -1e300};
            bool object_space = true;
            if (in.prim_type == SPT_PRIM_MESH) {
                for (int k = 0; k < 3; ++k) { olo[k] = fx.mesh_box[in.prim_id][k]; ohi[k] = fx.mesh_box[in.prim_id][3 + k]; }
            } else if (in.prim_type == SPT_PRIM_SPHERE) {
                const spt_sphere& sp = fx.spheres[in.prim_id];
                for (int k = 0; k < 3; ++k) { olo[k] = (double)sp.center[k] - std::fabs((double)sp.radius); ohi[k] = (double)sp.center[k] + std::fabs((double)sp.radius); }
            } else {
                object_space = false;
                const double margin = bezier_box_margin(in);
                for (int k = 0; k < 3; ++k) { olo[k] = (double)in.bmin[k] - margin; ohi[k] = (double)in.bmax[k] + margin; }
            }
            double ext = 1e-30;
            for (int k = 0; k < 3; ++k) ext = std::max(ext, ohi[k] - olo[k]);
            bool ok = true;
            for (int c = 0; c < 8; ++c) {
                double o[3];
                for (int k = 0; k < 3; ++k) o[k] = ((c >> k) & 1) ? ohi[k] + 1e-4 * ext : olo[k] - 1e-4 * ext;
                for (int r = 0; r < 3; ++r) {
                    double w = o[r];
                    if (object_space) w = (double)in.fwd[r] * o[0] + (double)in.fwd[3 + r] * o[1] + (double)in.fwd[6 + r] * o[2] + (double)in.fwd[9 + r];
                    dy.hull_corners[i][3 * c + r] = w;
                    ok = ok && std::isfinite(w);
                }
            }
            if (!ok) dy.hull_corners.clear();
        }
    }
}

}  // namespace

bool lds_fits(size_t plain_f4, size_t extra_bytes) {
    return plain_f4 * 16 + extra_bytes <= 32u * 1024u && kStackBytes + plain_f4 * 16 + extra_bytes <= 64u * 1024u;
}

SceneDynamic build_dynamic(const SceneFixed& fx, const DynView& s, const BuildOptions& opt, bool lds_geo, size_t n_blas_ranges, const StaticSections* st) {
    if (!st && !fx.n4) fail(SPT_ERR_INVALID_ARG, "the LDS-resident blob is written whole: it needs its static sections");
    SceneDynamic dy;
    dyn_trees(fx, s, opt, fx.n4, dy);
    dy.plain_f4 = dyn_layout(fx, dy, fx.n4, false);
    dyn_decide(fx, s, opt, dy, lds_geo, dy.plain_f4, n_blas_ranges);
    dyn_fill(fx, s, dy, fx.n4, st ? 0u : fx.tail_first, st);   // (the static sections have not moved: dy.tail_first == fx.tail_first)
    dyn_bounds(fx, s, dy);
    return dy;
}

namespace {

// postfix program per texture node (see shading.h "textures"); children precede parents, so a
// node's program is its children's programs followed by its own op
TexturePools compile_textures(const spt_scene_desc& s) {
    TexturePools tp;
    std::vector<uint32_t>& chain_pool = tp.chain;
    std::vector<uint4>& prog_pool = tp.prog;
    tp.roots.resize(s.n_textures);
    // emit(node, chain): instructions of `node` evaluated under the modifier chain `chain`
    std::function<uint32_t(uint32_t, std::vector<uint32_t>&, std::vector<uint4>&)> emit =
        [&](uint32_t node, std::vector<uint32_t>& chain, std::vector<uint4>& out) -> uint32_t {
        const spt_texture& t = s.textures[node];
        auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
        switch (t.type) {
        case SPT_TEX_SCALAR:
            out.push_back(make_uint4(TEXOP_SCALAR, bits(t.value[0]), bits(t.value[1]), bits(t.value[2])));
            return 1u;
        case SPT_TEX_IMAGE: {
            const uint32_t first = (uint32_t)chain_pool.size();
            chain_pool.insert(chain_pool.end(), chain.begin(), chain.end());
            out.push_back(make_uint4(TEXOP_IMAGE, t.image, first, (uint32_t)chain.size()));
            return 1u;
        }
        case SPT_TEX_SRGB: {
            const uint32_t d = emit(t.a, chain, out);
            out.push_back(make_uint4(TEXOP_SRGB, 0, 0, 0));
            return d;
        }
        case SPT_TEX_MODIFIER: {
            chain.push_back(node);
            const uint32_t d = emit(t.a, chain, out);
            chain.pop_back();
            return d;
        }
        default: {
            const uint32_t da = emit(t.a, chain, out);
            const uint32_t db = emit(t.b, chain, out);
            out.push_back(make_uint4(TEXOP_ADD + (t.type - SPT_TEX_ADD), 0, 0, 0));
            return std::max(da, db + 1u);
        }
        }
    };
    for (uint32_t i = 0; i < s.n_textures; ++i) {
        std::vector<uint32_t> chain;
        std::vector<uint4> code;
        const uint32_t depth = emit(i, chain, code);
        if (depth > 4u) fail(SPT_ERR_UNSUPPORTED, "texture expression needs more than 4 pending values");
        if (prog_pool.size() + code.size() > 0x7fffffffull) fail(SPT_ERR_UNSUPPORTED, "texture programs too large");
        tp.roots[i] = make_uint2((uint32_t)prog_pool.size(), (uint32_t)code.size());
        prog_pool.insert(prog_pool.end(), code.begin(), code.end());
    }
    if (chain_pool.empty()) chain_pool.push_back(0u);
    return tp;
}

// What an update needs again of the descriptor, and what follows from the part of it that an update keeps without a tree
void fixed_of_desc(const spt_scene_desc& s, const BuildOptions& opt, SceneFixed& fx) {
    fx.aggregate = s.aggregate; fx.light_sampler = s.light_sampler;
    fx.n_instances = s.n_instances; fx.n_lights = s.n_lights; fx.n_meshes = s.n_meshes; fx.n_spheres = s.n_spheres;
    fx.n_surfaces = s.n_surfaces; fx.n_bezier_patches = s.n_bezier_patches; fx.n_tris = s.n_tris;
    fx.env_light_index = s.env_light_index;
    fx.env_light_type = s.env_light_index >= 0 ? s.lights[s.env_light_index].type : 0u;
    fx.has_env = s.env.width != 0 && s.env.height != 0;
    for (uint32_t i = 0; i < s.n_meshes; ++i) {
        // each BLAS must index triangles inside its own mesh range
        fx.blas_depth = std::max(fx.blas_depth, bvh_depth(s.blas_nodes, s.n_blas_nodes, s.meshes[i].root, s.n_tris, "blas"));
    }
    fx.own_bvh = !opt.reference_bvh;   // see build_sah_blas
    fx.spheres.assign(s.spheres, s.spheres + s.n_spheres);
    fx.mesh_tris.resize(s.n_meshes);
    fx.mesh_first.resize(s.n_meshes);
    fx.mesh_box.resize(s.n_meshes);
    for (uint32_t i = 0; i < s.n_meshes; ++i) {   // (the per-row spans' object-space boxes: an update reads no triangle)
        const spt_mesh& m = s.meshes[i];
        fx.mesh_tris[i] = m.tri_count;
        fx.mesh_first[i] = m.tri_first;
        double olo[3] = {1e300, 1e300, 1e300}, ohi[3] = {-1e300, -1e300, -1e300};
        for (uint32_t t = m.tri_first; t < m.tri_first + m.tri_count; ++t) {
            const float* v[3] = {s.tri_pos[t].p0, s.tri_pos[t].p1, s.tri_pos[t].p2};
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < 3; ++k) { olo[k] = std::min(olo[k], (double)v[c][k]); ohi[k] = std::max(ohi[k], (double)v[c][k]); }
        }
        for (int k = 0; k < 3; ++k) { fx.mesh_box[i][k] = olo[k]; fx.mesh_box[i][3 + k] = ohi[k]; }
    }
    fx.surf_class.resize(s.n_surfaces);
    fx.surf_emissive.resize(s.n_surfaces);
    for (uint32_t i = 0; i < s.n_surfaces; ++i) {
        fx.surf_class[i] = shade_class(s, s.materials[s.surfaces[i].material]);
        fx.surf_emissive[i] = surface_emits(s.surfaces[i]) ? 1 : 0;
    }
    fx.tables_bytes = (size_t)s.n_tris * sizeof(spt_tri_attr) + (size_t)s.n_surfaces * sizeof(spt_surface) +
                      (size_t)s.n_materials * sizeof(spt_material) + (size_t)s.n_lights * sizeof(spt_light) + 64;
}

// The trees the BLAS forms are made from: own binned-SAH BLAS per mesh (see build_sah_blas), or the ABI trees as they are
struct BlasSource {
    std::vector<spt_bvh_node> own_nodes;
    std::vector<uint32_t> roots;        // per mesh: its root in `nodes`
    std::vector<uint32_t> tri_order;    // slot -> ABI triangle index
    const spt_bvh_node* nodes = nullptr;
};

void blas_source(const spt_scene_desc& s, const BuildOptions& opt, SceneFixed& fx, BlasSource& src) {
    src.roots.assign(s.n_meshes, 0u);
    src.tri_order.resize(s.n_tris);
    for (uint32_t i = 0; i < s.n_tris; ++i) src.tri_order[i] = i;
    fx.mesh_depth.assign(s.n_meshes, 0u);
    for (uint32_t i = 0; i < s.n_meshes; ++i) {
        if (!fx.own_bvh) { src.roots[i] = s.meshes[i].root; continue; }
        src.roots[i] = (uint32_t)src.own_nodes.size();
        build_sah_blas(s.tri_pos + s.meshes[i].tri_first, s.meshes[i].tri_first, s.meshes[i].tri_count, opt, src.own_nodes, src.tri_order);
        fx.mesh_depth[i] = bvh_depth(src.own_nodes.data(), (uint32_t)src.own_nodes.size(), src.roots[i], s.n_tris, "device blas");
        fx.own_blas_depth = std::max(fx.own_blas_depth, fx.mesh_depth[i]);
    }
    src.nodes = fx.own_bvh ? src.own_nodes.data() : s.blas_nodes;
}

// triangles in leaf order of the tree that is walked, ABI index in the first vertex's pad lane
spt_tri_pos leaf_order_record(const spt_tri_pos& src, uint32_t abi_index) {
    spt_tri_pos dst = src;
    for (int k = 0; k < 3; ++k) { dst.p1[k] = src.p1[k] - src.p0[k]; dst.p2[k] = src.p2[k] - src.p0[k]; }   // e1, e2 of triangle.rs:125-126
    std::memcpy(&dst.pad0, &abi_index, 4);
    return dst;
}

std::vector<spt_tri_pos> leaf_order_triangles(const spt_scene_desc& s, const std::vector<uint32_t>& tri_order) {
    std::vector<spt_tri_pos> tri_blob(s.n_tris);
    for (uint32_t i = 0; i < s.n_tris; ++i) tri_blob[i] = leaf_order_record(s.tri_pos[tri_order[i]], tri_order[i]);
    return tri_blob;
}

// (root.lo, root ref) (root.hi, the mesh's range in the blob's triangle copy when it fits 16 + 16 bits: flat.h)
void set_mesh_record(SceneFixed& fx, uint32_t mesh, const float* lo, const float* hi, uint32_t root_ref) {
    const uint32_t first = fx.mesh_first[mesh], count = fx.mesh_tris[mesh];
    const uint32_t range = (first < 65536u && count < 65536u) ? (first | (count << 16)) : 0u;
    float rf, range_f;
    std::memcpy(&rf, &root_ref, 4);
    std::memcpy(&range_f, &range, 4);
    fx.mesh_rec[2 * mesh] = make_float4(lo[0], lo[1], lo[2], rf);
    fx.mesh_rec[2 * mesh + 1] = make_float4(hi[0], hi[1], hi[2], range_f);
}

// One mesh's nodes of the LDS-resident form, appended to `wblas`, with its range and its record (spt_scene_create per mesh;
// spt_scene_deform for the meshes it names)
void build_wide_mesh(const spt_bvh_node* nodes, uint32_t mesh_root, uint32_t mesh, SceneFixed& fx, std::vector<float4>& wblas,
                     std::vector<std::pair<uint32_t, uint32_t>>& blas_range) {
    const uint32_t first_node = (uint32_t)(wblas.size() / 4);
    const uint32_t sup = build_wide(nodes, mesh_root, wblas, 0u, "blas");
    uint32_t root_ref;
    std::memcpy(&root_ref, &wblas[(size_t)sup * 4].w, 4);
    blas_range.emplace_back(first_node, (uint32_t)(wblas.size() / 4));
    set_mesh_record(fx, mesh, nodes[mesh_root].bmin, nodes[mesh_root].bmax, root_ref);
}

// The BLAS nodes and the mesh records of one form.  BLAS: 2-wide full-precision nodes when the whole scene fits LDS, compressed
// 4-wide nodes otherwise
void build_blas(const spt_scene_desc& s, const BlasSource& src, bool n4, StaticBuild& sb) {
    SceneFixed& fx = sb.fixed;
    std::vector<float4>& wblas = sb.wblas;
    sb.blas_range.clear();
    wblas.clear();
    fx.mesh_rec.assign((size_t)s.n_meshes * 2, make_float4(0, 0, 0, 0));
    fx.max_blas_need = 0;
    fx.n4_nodes.clear();
    for (uint32_t i = 0; i < s.n_meshes; ++i) {
        const uint32_t mesh_root = src.roots[i];
        if (n4) {
            // (first node, nodes, height of the root node: what a refit of the mesh launches its kernels over - spt_scene_deform)
            uint32_t need = 0, height = 0;
            const uint32_t first_node = (uint32_t)(wblas.size() / 4);
            const uint32_t root_ref = build_n4(src.nodes, mesh_root, wblas, &need, "blas", 0u, &height);
            fx.max_blas_need = std::max(fx.max_blas_need, need);
            fx.n4_nodes.push_back({first_node, (uint32_t)(wblas.size() / 4) - first_node, height});
            set_mesh_record(fx, i, src.nodes[mesh_root].bmin, src.nodes[mesh_root].bmax, root_ref);
        } else {
            build_wide_mesh(src.nodes, mesh_root, i, fx, wblas, sb.blas_range);
        }
    }
    if (wblas.size() > 0x7fffffffull / 16) fail(SPT_ERR_UNSUPPORTED, "scene geometry larger than 32 GiB");
    fx.blas_f4 = (uint32_t)wblas.size();
    fx.n4 = n4;
}

// Which kernels the materials, surfaces and textures of the scene need (see spt_scene, spt_hip.hip), but for the lights' types,
// which an update may change
void classify(const spt_scene_desc& s, StaticBuild& sb) {
    // simple: Lambert + delta lights only, no emission / environment / media.  fused: ... and no recipe, normal map or emissive map
    bool simple = s.env.width == 0 && s.n_lights > 0, fused = simple;
    for (uint32_t i = 0; i < s.n_materials; ++i) {
        simple = simple && s.materials[i].bxdf == SPT_BXDF_LAMBERT;
        fused = fused && s.materials[i].bxdf == SPT_BXDF_LAMBERT && s.materials[i].recipe == 0;
    }
    for (uint32_t i = 0; i < s.n_surfaces; ++i) {
        const spt_surface& sf = s.surfaces[i];
        const bool plain = sf.inside_medium < 0 && !surface_emits(sf);
        simple = simple && plain;
        fused = fused && plain && sf.normal_map == 0 && sf.emissive_map == 0;
    }
    // image textures: only scenes that sample one per hit pay for the k_shade<2, .> variant
    bool textured = false;
    for (uint32_t i = 0; i < s.n_materials; ++i) textured = textured || s.materials[i].recipe != 0;
    for (uint32_t i = 0; i < s.n_surfaces; ++i) textured = textured || s.surfaces[i].normal_map != 0 || s.surfaces[i].emissive_map != 0;
    for (uint32_t i = 0; i < s.n_materials; ++i) sb.subsurface = sb.subsurface || s.materials[i].substrate == SPT_SUBSTRATE_SUBSURFACE;
    for (uint32_t i = 0; i < s.n_material_recipes; ++i) sb.subsurface = sb.subsurface || s.material_recipes[i].type == SPT_MAT_SUBSURFACE;
    sb.has_probe = sb.subsurface;
    if (s.n_pndfs != 0) {   // glints get a heavy variant of their own: their tree walks would cost k_shade<2> its registers
        sb.subsurface = true;
        sb.has_pndf = true;
    }
    if (sb.subsurface) textured = true;   // k_shade<3> is k_shade<2> + the probe: the texture tables (possibly empty) are uploaded too
    sb.textured = textured;
    sb.fixed.simple_fixed = simple && !textured;
    sb.fixed.fused_fixed = fused;
    for (uint32_t i = 0; i < s.n_bezier_patches; ++i) sb.bez_newton = sb.bez_newton || s.bezier_patches[i].cp[0][0][3] != 0.0f;
}

}  // namespace

StaticBuild build_static(const spt_scene_desc& s, const BuildOptions& opt) {
    StaticBuild sb;
    SceneFixed& fx = sb.fixed;
    fixed_of_desc(s, opt, fx);
    classify(s, sb);
    // one float4 blob for everything the traversal touches (see dyn_layout)
    BlasSource src;
    blas_source(s, opt, fx, src);
    sb.tri_blob = leaf_order_triangles(s, src.tri_order);
    build_blas(s, src, false, sb);
    {   // the LDS-resident form, if the blob it makes with the instances as they are now fits
        const DynView view = dyn_view(s, fx.surf_emissive.data());
        SceneDynamic trial;
        dyn_trees(fx, view, opt, false, trial);
        sb.lds_geo = lds_fits(dyn_layout(fx, trial, false, false)) && opt.lds_geo;
    }
    // patches: the streaming walkers of the large-scene path refill lanes whose patch test is over (measured,
    // t_bezier.json 512^2 @ 64 spp: 177 ms LDS-resident nested walkers, 147 ms here; SPT_BEZ_LDS=1 for the former)
    // (not under SPT_REFERENCE_BVH=1: only the exact 2-wide nodes in the reference's visit order reproduce which near
    //  misses of a patch the reference's own culling loses - see bezier_box_margin; the compressed 4-wide form of
    //  the caller's trees, which serves scenes beyond LDS in that mode, can differ from it in such a pixel)
    if (opt.with_bezier && fx.own_bvh && !opt.bez_lds) sb.lds_geo = false;
    if (!sb.lds_geo) {
        build_blas(s, src, true, sb);
        SceneDynamic none;   // where the sections an update rewrites start: behind the static ones, whatever the instances are
        dyn_layout(fx, none, true, false);
        fx.tail_first = none.tail_first;
    }
    if (sb.lds_geo) {   // (<= 32 KB: an update writes the whole blob again)
        auto section = [](std::vector<float4>& v, const void* src, size_t bytes) {
            v.assign((bytes + 15) / 16, make_float4(0, 0, 0, 0));
            if (bytes) std::memcpy(v.data(), src, bytes);
        };
        fx.wblas = sb.wblas;
        section(fx.tri_sec, sb.tri_blob.data(), (size_t)s.n_tris * sizeof(spt_tri_pos));
        section(fx.attr_sec, s.tri_attr, (size_t)s.n_tris * sizeof(spt_tri_attr));
        section(fx.surf_sec, s.surfaces, (size_t)s.n_surfaces * sizeof(spt_surface));
        section(fx.mat_sec, s.materials, (size_t)s.n_materials * sizeof(spt_material));
    }
    const size_t ne = (size_t)s.env.width * s.env.height;
    sb.env_px.resize(ne);
    sb.env_uk.resize(ne);
    for (size_t i = 0; i < ne; ++i) {
        sb.env_px[i] = make_float4(s.env.texels[3 * i], s.env.texels[3 * i + 1], s.env.texels[3 * i + 2], s.env.alias.props[i]);
        uint32_t ub;
        std::memcpy(&ub, &s.env.alias.u[i], 4);
        sb.env_uk[i] = make_uint2(ub, s.env.alias.k[i]);
    }
    if (sb.subsurface) {
        sb.ss_cdf.resize(SPT_SS_CDF_SIZE);
        for (uint32_t i = 0; i < SPT_SS_CDF_SIZE; ++i) {
            spt_ss_cdf_entry(i, &sb.ss_cdf[i].x, &sb.ss_cdf[i].y);
            if (i && !(sb.ss_cdf[i].y >= sb.ss_cdf[i - 1].y)) fail(SPT_ERR_UNSUPPORTED, "BSSRDF radius table is not monotonic");   // ss_sample_r bisects it
        }
    }
    if (sb.textured) sb.tex = compile_textures(s);
    return sb;
}

// ---- spt_scene_deform: the part of the static build that follows one mesh's vertices ---------------------------------------
namespace {

// the raw bounds of the new positions; the object-space box of the per-row spans goes into fx.mesh_box
RefitBox deformed_bounds(SceneFixed& fx, const spt_mesh_deform& e) {
    RefitBox raw = refit_empty();
    for (uint32_t t = 0; t < e.tri_count; ++t) refit_grow_tri(raw, e.tri_pos[t].p0, e.tri_pos[t].p1, e.tri_pos[t].p2);
    for (int k = 0; k < 3; ++k) { fx.mesh_box[e.mesh][k] = (double)raw.lo[k]; fx.mesh_box[e.mesh][3 + k] = (double)raw.hi[k]; }
    return raw;
}

}  // namespace

void validate_deform(const SceneFixed& fx, uint32_t n_meshes, const spt_mesh_deform* meshes) {
    if (n_meshes && !meshes) fail(SPT_ERR_INVALID_ARG, "scene_deform: null array");
    std::vector<uint8_t> named(fx.n_meshes, 0);
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const spt_mesh_deform& e = meshes[i];
        if (e.mesh >= fx.n_meshes) fail(SPT_ERR_INVALID_ARG, "scene_deform: mesh index out of range");
        if (named[e.mesh]++) fail(SPT_ERR_INVALID_ARG, "scene_deform: a mesh is named twice");
        // (a creation refuses a mesh without triangles; checked here too: the kernels' grids are sized by the count)
        if (e.tri_count == 0u || e.tri_count != fx.mesh_tris[e.mesh]) fail(SPT_ERR_INVALID_ARG, "scene_deform: tri_count differs from the mesh's (triangles cannot appear or vanish)");
        if (!e.tri_pos) fail(SPT_ERR_INVALID_ARG, "scene_deform: null array");
        for (uint32_t t = 0; t < e.tri_count; ++t)
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(e.tri_pos[t].p0[k]) || !std::isfinite(e.tri_pos[t].p1[k]) || !std::isfinite(e.tri_pos[t].p2[k]))
                    fail(SPT_ERR_INVALID_ARG, "scene_deform: a position is not finite");
    }
    if (n_meshes && !fx.own_bvh)
        fail(SPT_ERR_UNSUPPORTED, "scene_deform: the scene walks the caller's trees (SPT_REFERENCE_BVH): the library owns none to refit");
}

std::vector<RefitBox> deform_fixed_n4(SceneFixed& fx, uint32_t n_meshes, const spt_mesh_deform* meshes) {
    std::vector<RefitBox> roots(n_meshes);
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const RefitBox box = refit_padded(deformed_bounds(fx, meshes[i]));
        // every node's extent is at most the mesh's own (see scene_refit.h): the one refusal the refit kernels could meet
        for (int k = 0; k < 3; ++k)
            if (refit_exponent(box.hi[k] - box.lo[k]) > 120) fail(SPT_ERR_UNSUPPORTED, "scene_deform: node extent too large to quantise");
        uint32_t root_ref;
        std::memcpy(&root_ref, &fx.mesh_rec[2 * meshes[i].mesh].w, 4);
        set_mesh_record(fx, meshes[i].mesh, box.lo, box.hi, root_ref);
        roots[i] = box;
    }
    return roots;
}

std::vector<RefitBox> deform_fixed_n4_raw(SceneFixed& fx, uint32_t n_meshes, const uint32_t* mesh_ids, const RefitBox* raw) {
    std::vector<RefitBox> roots(n_meshes);
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const uint32_t mesh = mesh_ids[i];
        for (int k = 0; k < 3; ++k) { fx.mesh_box[mesh][k] = (double)raw[i].lo[k]; fx.mesh_box[mesh][3 + k] = (double)raw[i].hi[k]; }
        const RefitBox box = refit_padded(raw[i]);
        for (int k = 0; k < 3; ++k)
            if (refit_exponent(box.hi[k] - box.lo[k]) > 120) fail(SPT_ERR_UNSUPPORTED, "scene_deform_vertices: node extent too large to quantise");
        uint32_t root_ref;
        std::memcpy(&root_ref, &fx.mesh_rec[2 * mesh].w, 4);
        set_mesh_record(fx, mesh, box.lo, box.hi, root_ref);
        roots[i] = box;
    }
    return roots;
}

void deform_fixed_lds(SceneFixed& fx, std::vector<std::pair<uint32_t, uint32_t>>& blas_range, uint32_t n_meshes, const spt_mesh_deform* meshes,
                      const BuildOptions& opt) {
    if (blas_range.size() != fx.n_meshes) fail(SPT_ERR_UNSUPPORTED, "scene_deform: the scene keeps no node range per mesh");
    std::vector<const spt_mesh_deform*> edit(fx.n_meshes, nullptr);
    for (uint32_t i = 0; i < n_meshes; ++i) edit[meshes[i].mesh] = &meshes[i];
    std::vector<float4> wblas;
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    spt_tri_pos* tri_sec = reinterpret_cast<spt_tri_pos*>(fx.tri_sec.data());
    spt_tri_attr* attr_sec = reinterpret_cast<spt_tri_attr*>(fx.attr_sec.data());
    for (uint32_t m = 0; m < fx.n_meshes; ++m) {
        const uint32_t first = fx.mesh_first[m], count = fx.mesh_tris[m];
        if (!edit[m]) {
            // the nodes as they are, behind whatever the meshes before them take now: refs to nodes index the whole array
            const uint32_t old_first = blas_range[m].first, nodes = blas_range[m].second - old_first, new_first = (uint32_t)(wblas.size() / 4);
            const uint32_t delta = new_first - old_first;
            auto moved = [delta](float& w) {
                uint32_t ref;
                std::memcpy(&ref, &w, 4);
                if (!(ref & kLeaf)) { ref += delta; std::memcpy(&w, &ref, 4); }
            };
            wblas.insert(wblas.end(), fx.wblas.begin() + (size_t)old_first * 4, fx.wblas.begin() + (size_t)blas_range[m].second * 4);
            for (uint32_t j = 0; j < nodes; ++j) {
                float4* f = &wblas[((size_t)new_first + j) * 4];
                moved(f[0].w);
                if (j != 0u) moved(f[1].w);   // (the super-root has no right child: build_wide)
            }
            moved(fx.mesh_rec[2 * m].w);
            ranges.emplace_back(new_first, new_first + nodes);
            continue;
        }
        const spt_mesh_deform& e = *edit[m];
        std::vector<spt_bvh_node> nodes;
        std::vector<uint32_t> order((size_t)first + count, 0u);
        build_sah_blas(e.tri_pos, first, count, opt, nodes, order);
        fx.mesh_depth[m] = bvh_depth(nodes.data(), (uint32_t)nodes.size(), 0u, fx.n_tris, "device blas");
        build_wide_mesh(nodes.data(), 0u, m, fx, wblas, ranges);
        for (uint32_t slot = first; slot < first + count; ++slot) tri_sec[slot] = leaf_order_record(e.tri_pos[order[slot] - first], order[slot]);
        if (e.tri_attr) std::memcpy(static_cast<void*>(attr_sec + first), e.tri_attr, (size_t)count * sizeof(spt_tri_attr));
        deformed_bounds(fx, e);
    }
    fx.own_blas_depth = 0;
    for (uint32_t d : fx.mesh_depth) fx.own_blas_depth = std::max(fx.own_blas_depth, d);
    fx.wblas = std::move(wblas);
    fx.blas_f4 = (uint32_t)fx.wblas.size();
    blas_range = std::move(ranges);
}

}  // namespace scene_build
