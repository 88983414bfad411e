// vr_host_bvh.cpp -- the host's BVH builders in the reference's operation order, plain data in and
// out (no scene, no HIP): BoundingVolumeHierarchy::build (bounding_volume_hierarchy.rs:30-74), the
// binned-SAH traversal tree, and the collapse of either into the render kernel's 4-wide tree.
#define VR_HOST_NO_HIP
#include "vr_host.h"

#include <array>

namespace {
using namespace vrh;

struct Interval {  // util/interval.rs
    double min, max;
};
Interval iv_empty() { return {INFINITY, -INFINITY}; }
bool iv_is_empty(Interval a) { return a.min > a.max; }
Interval iv_union(Interval a, Interval b) {  // interval.rs:66-77 (f64::min/max ignore NaN)
    if (iv_is_empty(a)) return b;
    if (iv_is_empty(b)) return a;
    return {std::fmin(a.min, b.min), std::fmax(a.max, b.max)};
}
Interval iv_expand(Interval a, double v) {  // interval.rs:79-87
    if (iv_is_empty(a)) return {v, v};
    return {std::fmin(a.min, v), std::fmax(a.max, v)};
}
struct Box3 {
    Interval b[3];
};
Box3 box_empty() { return {{iv_empty(), iv_empty(), iv_empty()}}; }
Box3 box_union(const Box3& a, const Box3& b) {
    return {{iv_union(a.b[0], b.b[0]), iv_union(a.b[1], b.b[1]), iv_union(a.b[2], b.b[2])}};
}
int largest_dimension(const Box3& bb) {  // util/axis_aligned_bounding_box.rs:76-99
    int acc = 0;
    double acc_size = 0.0;
    for (int i = 0; i < 3; ++i) {
        double size = bb.b[i].min == bb.b[i].max ? -1.0 : bb.b[i].max - bb.b[i].min;
        if (size > acc_size) {
            acc = i;
            acc_size = size;
        }
    }
    return acc;
}
void box_to_layout(const Box3& bb, double out[6]) {
    for (int i = 0; i < 3; ++i) {
        out[2 * i] = bb.b[i].min;
        out[2 * i + 1] = bb.b[i].max;
    }
}

struct BuildPrim {
    Box3 box;
    double centre[3];
    uint64_t orig;
};

#ifndef VR_SAH_BINS  // bins per axis of the host's binned SAH (the device build uses 32)
#define VR_SAH_BINS 32
#endif
// Traversal tree (the default): a binned-SAH binary tree over the same triangles, leaf size 1.
// The reference's closest hit does not depend on its tree: a box test on a superset box passes
// whenever it passes on the subset (every rounding step of (bound - o) / d is monotonic in
// `bound`), so a triangle is reachable in the reference tree iff the exact line test passes on
// its OWN box -- which this tree tests too, as the leaf child's box -- and distance ties are
// broken by the reference in-order rank carried in TriVerts::rank.  Only the amount of work
// depends on the tree: SAH splits cut node visits against the median split.
// One top-down build over prims[lo, hi), leaf size 1: the reference's median split
// (bounding_volume_hierarchy.rs:38-74), or the binned-SAH split of the traversal tree
struct Builder {
    std::vector<BuildPrim>& prims;  // permuted in place into leaf order
    bool sah;
    int tri_base;
    std::vector<vr::Node> nodes;  // interior nodes, preorder
    int max_depth = 0;

    static double area(const Box3& b) {
        const double dx = b.b[0].max - b.b[0].min, dy = b.b[1].max - b.b[1].min, dz = b.b[2].max - b.b[2].min;
        if (!(dx >= 0.0) || !(dy >= 0.0) || !(dz >= 0.0)) return 0.0;
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    }

    uint64_t split_median(uint64_t lo, uint64_t hi, const Box3& bounds) {
        const int axis = largest_dimension(bounds);
        // sort_unstable_by(centre[axis].partial_cmp, NaN -> Equal); equal keys ordered by input
        // index so the permutation is unique (the oracle applies the same rule)
        std::sort(prims.begin() + lo, prims.begin() + hi, [axis](const BuildPrim& a, const BuildPrim& b) {
            double ca = a.centre[axis], cb = b.centre[axis];
            if (ca < cb) return true;
            if (ca > cb) return false;
            return a.orig < b.orig;
        });
        return lo + (hi - lo) / 2;
    }

    uint64_t split_sah(uint64_t lo, uint64_t hi, int level) {
        const uint64_t n = hi - lo;
        double cmin[3] = {INFINITY, INFINITY, INFINITY}, cmax[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint64_t i = lo; i < hi; ++i)
            for (int c = 0; c < 3; ++c) {
                cmin[c] = std::min(cmin[c], prims[i].centre[c]);
                cmax[c] = std::max(cmax[c], prims[i].centre[c]);
            }
        constexpr int kBins = VR_SAH_BINS;
        int best_axis = -1, best_bin = -1;
        double best_cost = INFINITY;
        // median splits where SAH would push the tree past the deepest traversal stack (48)
        const int need = n > 1 ? 64 - __builtin_clzll(n - 1) : 0;  // ceil(log2 n)
        if (level + need < 44) {
            for (int a = 0; a < 3; ++a) {
                const double ext = cmax[a] - cmin[a];
                if (!(ext > 0.0)) continue;
                Box3 bb[kBins];
                uint64_t cnt[kBins] = {};
                for (int k = 0; k < kBins; ++k) bb[k] = box_empty();
                const double scale = kBins / ext;
                for (uint64_t i = lo; i < hi; ++i) {
                    int k = (int)((prims[i].centre[a] - cmin[a]) * scale);
                    k = std::min(kBins - 1, std::max(0, k));
                    ++cnt[k];
                    bb[k] = box_union(bb[k], prims[i].box);
                }
                double right_area[kBins];
                uint64_t right_cnt[kBins];
                Box3 acc = box_empty();
                uint64_t c = 0;
                for (int k = kBins - 1; k > 0; --k) {
                    acc = box_union(acc, bb[k]);
                    c += cnt[k];
                    right_area[k] = area(acc);
                    right_cnt[k] = c;
                }
                acc = box_empty();
                c = 0;
                for (int k = 0; k < kBins - 1; ++k) {
                    acc = box_union(acc, bb[k]);
                    c += cnt[k];
                    if (c == 0 || right_cnt[k + 1] == 0) continue;
                    const double cost = area(acc) * (double)c + right_area[k + 1] * (double)right_cnt[k + 1];
                    if (cost < best_cost) {
                        best_cost = cost;
                        best_axis = a;
                        best_bin = k;
                    }
                }
            }
        }
        if (best_axis >= 0) {
            const double ext = cmax[best_axis] - cmin[best_axis], scale = kBins / ext;
            auto mid = std::partition(prims.begin() + lo, prims.begin() + hi, [&](const BuildPrim& p) {
                int k = (int)((p.centre[best_axis] - cmin[best_axis]) * scale);
                k = std::min(kBins - 1, std::max(0, k));
                return k <= best_bin;
            });
            const uint64_t m = (uint64_t)(mid - prims.begin());
            if (m > lo && m < hi) return m;
        }
        // median split on the widest centroid axis (ties by reference rank: deterministic)
        int a = 0;
        for (int c = 1; c < 3; ++c)
            if (cmax[c] - cmin[c] > cmax[a] - cmin[a]) a = c;
        const uint64_t m = lo + n / 2;
        std::nth_element(prims.begin() + lo, prims.begin() + m, prims.begin() + hi,
                         [a](const BuildPrim& x, const BuildPrim& y) {
                             if (x.centre[a] < y.centre[a]) return true;
                             if (x.centre[a] > y.centre[a]) return false;
                             return x.orig < y.orig;
                         });
        return m;
    }

    // Returns the child encoding of the subtree over prims[lo, hi): >= 0 interior node index,
    // < 0 leaf ~(tri_base + leaf position).  `bounds` receives the subtree's box.
    int32_t build(uint64_t lo, uint64_t hi, int level, Box3& bounds) {
        max_depth = std::max(max_depth, level + 1);
        bounds = box_empty();
        for (uint64_t i = lo; i < hi; ++i) bounds = box_union(bounds, prims[i].box);
        if (hi - lo <= 1) return ~(int32_t)(tri_base + lo);
        const uint64_t mid = sah ? split_sah(lo, hi, level) : split_median(lo, hi, bounds);
        const int32_t me = (int32_t)nodes.size();
        nodes.emplace_back();
        Box3 lb, rb;
        const int32_t l = build(lo, mid, level + 1, lb);
        const int32_t r = build(mid, hi, level + 1, rb);
        vr::Node& nd = nodes[me];
        std::memset(&nd, 0, sizeof nd);
        box_to_layout(lb, nd.box[0]);
        box_to_layout(rb, nd.box[1]);
        nd.child[0] = l;
        nd.child[1] = r;
        return me;
    }
};

// The render kernel's 4-wide tree, collapsed from a binary tree (the SAH traversal tree, or the
// reference's median-split tree): starting from a binary node's two children, the interior child
// with the largest surface area is replaced by its two children until there are four (or only
// leaves).  Leaf children keep the triangle's own box, so DESIGN.md section 5's argument carries
// over unchanged: interior boxes are unions (supersets), and a triangle is tested iff the exact
// line test passes on its own box.  `stack` is the deepest the kernel's traversal stack can get
// (a visit pushes all but one hit interior child): the maximum over root-to-node paths of the
// sum of (interior children - 1).
struct WideBuilder {
    const std::vector<vr::Node>& bin;
    std::vector<vr::Node4>& n4;
    int stack = 0;
    bool dp = false;  // the SAH-optimal DP collapse (else greedy by largest child area)
    WideBuilder(const std::vector<vr::Node>& b, std::vector<vr::Node4>& a, bool dp_ = false) : bin(b), n4(a), dp(dp_) {}

    static double area(const double* b) {
        const double dx = b[1] - b[0], dy = b[3] - b[2], dz = b[5] - b[4];
        if (!(dx >= 0.0) || !(dy >= 0.0) || !(dz >= 0.0)) return 0.0;
        return dx * dy + dy * dz + dz * dx;
    }

    // SAH-optimal collapse (the default; VR_SCENE_GREEDY_COLLAPSE builds the greedy one): a visit of a wide node costs one node step whatever its
    // children, and is entered with probability ~ its surface area, so the wide tree minimising
    // sum(SA(wide node)) is chosen by a bottom-up DP over the binary tree (as in Ylitie et al.'s
    // wide-BVH collapse, leaf size 1): F(x) = SA(x) + H(x, 4) is x as a wide node; C(x, k), the best
    // cost of x's subtree in at most k slots of its parent, = min(F(x), H(x, k)) for k >= 2 (x
    // dissolved into its children) and F(x) for k = 1; H(x, k) = min over a of C(l, a) + C(r, k - a),
    // a leaf costing 0.  split[x][k]: 0 keeps x as one slot, a > 0 gives its left child a slots.
    std::vector<std::array<double, 5>> C;
    std::vector<std::array<uint8_t, 5>> split;
    double H(int32_t x, int k, uint8_t& arg) const {
        double best = INFINITY;
        for (int a = 1; a < k; ++a) {
            const int32_t l = bin[x].child[0], r = bin[x].child[1];
            const double v = (l >= 0 ? C[l][a] : 0.0) + (r >= 0 ? C[r][k - a] : 0.0);
            if (v < best) {
                best = v;
                arg = (uint8_t)a;
            }
        }
        return best;
    }
    void plan(int32_t x, double sa) {  // x interior, sa: its surface area
        if (C.size() < bin.size()) {
            C.resize(bin.size());
            split.resize(bin.size());
        }
        for (int c = 0; c < 2; ++c)
            if (bin[x].child[c] >= 0) plan(bin[x].child[c], area(bin[x].box[c]));
        uint8_t a4 = 1;
        const double f = sa + H(x, 4, a4);
        C[x][1] = f;
        split[x][1] = 0;
        for (int k = 2; k <= 4; ++k) {
            uint8_t a = 1;
            const double h = H(x, k, a);
            C[x][k] = h < f ? h : f;
            split[x][k] = h < f ? a : 0;
        }
        split[x][0] = a4;  // the split of x's two children over a wide node's 4 slots
    }
    void plan_root(int32_t b) {  // before collapse(b, 0) of a BVH root
        double u[6];
        for (int j = 0; j < 6; ++j)
            u[j] = (j & 1) ? std::max(bin[b].box[0][j], bin[b].box[1][j]) : std::min(bin[b].box[0][j], bin[b].box[1][j]);
        plan(b, area(u));
    }
    void expand(int32_t x, const double* bx, int k, int32_t* code, const double** box, int& n) const {
        if (x < 0 || k == 1 || split[x][k] == 0) {
            code[n] = x;
            box[n] = bx;
            ++n;
            return;
        }
        expand(bin[x].child[0], bin[x].box[0], split[x][k], code, box, n);
        expand(bin[x].child[1], bin[x].box[1], k - split[x][k], code, box, n);
    }

    // the children of a wide node over binary node b: the DP's expansion or the greedy one
    int children(int32_t b, bool use_dp, int32_t* code, const double** box) const {
        int n = 0;
        if (use_dp) {
            const int a = split[b][0];
            expand(bin[b].child[0], bin[b].box[0], a, code, box, n);
            expand(bin[b].child[1], bin[b].box[1], 4 - a, code, box, n);
            return n;
        }
        for (int c = 0; c < 2; ++c) {
            code[c] = bin[b].child[c];
            box[c] = bin[b].box[c];
        }
        n = 2;
        while (n < 4) {
            int pick = -1;
            double best = -1.0;
            for (int k = 0; k < n; ++k)
                if (code[k] >= 0 && area(box[k]) > best) {
                    best = area(box[k]);
                    pick = k;
                }
            if (pick < 0) break;
            const vr::Node& c = bin[code[pick]];
            code[pick] = c.child[0];
            box[pick] = c.box[0];
            code[n] = c.child[1];
            box[n] = c.box[1];
            ++n;
        }
        return n;
    }
    // stack bound of the wide subtree over b when every node below uses the DP (or the greedy)
    // expansion: (interior children - 1) + the deepest child's (memoised)
    std::vector<int16_t> need_memo[2];
    int need(int32_t b, bool use_dp) {
        auto& m = need_memo[use_dp];
        if (m.size() < bin.size()) m.assign(bin.size(), -1);
        if (m[b] >= 0) return m[b];
        int32_t code[4];
        const double* box[4];
        const int n = children(b, use_dp, code, box);
        int interior = 0, deepest = 0;
        for (int k = 0; k < n; ++k)
            if (code[k] >= 0) {
                ++interior;
                deepest = std::max(deepest, need(code[k], use_dp));
            }
        return m[b] = (int16_t)(std::max(0, interior - 1) + deepest);
    }
    int limit = 1 << 30;  // dp: a node takes the DP expansion only if its DP subtree's stack fits

    // wide node over binary interior node `b`; `pushed`: stack entries held by its ancestors
    int32_t collapse(int32_t b, int pushed) {
        int32_t code[4];
        const double* box[4];
        // the DP expansion where its whole subtree's stack bound fits under `limit` from here (then
        // it fits at every node below too); else greedy here, and the children decide for themselves
        const int n = children(b, dp && pushed + need(b, true) <= limit, code, box);
        const int32_t me = (int32_t)n4.size();
        n4.emplace_back();
        int interior = 0;
        for (int k = 0; k < n; ++k) interior += code[k] >= 0;
        const int here = pushed + std::max(0, interior - 1);
        stack = std::max(stack, here);
        int32_t out[4];
        for (int k = 0; k < 4; ++k) out[k] = vr::kEmptyChild;
        for (int k = 0; k < n; ++k) out[k] = code[k] >= 0 ? collapse(code[k], here) : code[k];
        vr::Node4& w = n4[me];
        std::memset(&w, 0, sizeof w);
        for (int k = 0; k < 4; ++k) {
            w.child[k] = out[k];
            for (int j = 0; j < 6; ++j) {
                const double v = k < n ? box[k][j] : NAN;
                w.bound[j][k] = k < n ? ((j & 1) ? round_upper(v) : round_lower(v)) : NAN;
            }
        }
        return me;
    }
};

// The 4-wide tree over a device-built (median-split) binary tree, planned on the host from the
// triangle count alone: that tree's shape depends only on n (a node over n leaves splits n/2 :
// n - n/2; pre-order indices, the left subtree's m leaves take m - 1 indices), so no node has to
// come back from the device.  Parity collapse: one wide node per binary node at even depth, its
// children the binary node's children or, for interior ones, their two children.  desc: per wide
// node the four slots' box sources (binary node * 2 + child, -1 empty) then their child links;
// vr_build.hip's fill_wide_kernel gathers the boxes.
struct ShapeWide {
    std::vector<int32_t>& desc;
    int& stack;
    int32_t tri_base;
    struct Sub {
        uint64_t lo, hi;
        int32_t idx;  // global binary index when hi - lo >= 2
    };
    static void kids(const Sub& p, Sub out[2]) {
        const uint64_t mid = p.lo + (p.hi - p.lo) / 2;
        out[0] = {p.lo, mid, p.idx + 1};
        out[1] = {mid, p.hi, p.idx + (int32_t)(mid - p.lo)};
    }
    int32_t wide(const Sub& b, int pushed) {
        const int32_t me = (int32_t)(desc.size() / 8);
        desc.resize(desc.size() + 8, -1);
        int32_t src[4];
        Sub sub[4];
        int n = 0;
        Sub c[2];
        kids(b, c);
        for (int i = 0; i < 2; ++i) {
            if (c[i].hi - c[i].lo == 1) {
                src[n] = b.idx * 2 + i;
                sub[n++] = c[i];
            } else {
                Sub g[2];
                kids(c[i], g);
                for (int j = 0; j < 2; ++j) {
                    src[n] = c[i].idx * 2 + j;
                    sub[n++] = g[j];
                }
            }
        }
        int interior = 0;
        for (int k = 0; k < n; ++k) interior += sub[k].hi - sub[k].lo > 1;
        const int here = pushed + std::max(0, interior - 1);
        stack = std::max(stack, here);
        for (int k = 0; k < 4; ++k) {
            int32_t code = vr::kEmptyChild;
            if (k < n)
                code = sub[k].hi - sub[k].lo == 1 ? ~(tri_base + (int32_t)sub[k].lo) : wide(sub[k], here);
            desc[(size_t)me * 8 + k] = k < n ? src[k] : -1;
            desc[(size_t)me * 8 + 4 + k] = code;
        }
        return me;
    }
};


// BoundingBox::from_points(&vertices) (triangle.rs:101-105) of the triangle at v; raises extent to its max |coordinate|
Box3 tri_box(const double* v, double& extent) {
    Box3 bb = box_empty();
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) {
            bb.b[c] = iv_expand(bb.b[c], v[3 * k + c]);
            extent = std::max(extent, std::fabs(v[3 * k + c]));
        }
    return bb;
}

}  // namespace

namespace vrh {

// f32 copies of f64 box bounds, rounded outward (a lower bound down, an upper bound up), so an
// f32 box contains its f64 box
float round_lower(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafter(f, -INFINITY);
    return f;
}
float round_upper(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, INFINITY);
    return f;
}

void mesh_bounds(const double* vertices, uint64_t n, double root_box[6], double* extent) {
    Box3 rb = box_empty();
    *extent = 0.0;
    for (uint64_t t = 0; t < n; ++t) rb = box_union(rb, tri_box(vertices + 9 * t, *extent));
    box_to_layout(rb, root_box);
}

MeshTree build_mesh_tree(const double* vertices, uint64_t n, int32_t tri_base, int32_t node_base, bool sah) {
    MeshTree out;
    std::vector<BuildPrim> prims(n);
    for (uint64_t t = 0; t < n; ++t) {
        const Box3 bb = tri_box(vertices + 9 * t, out.extent);
        prims[t].box = bb;
        for (int c = 0; c < 3; ++c) prims[t].centre[c] = (bb.b[c].min + bb.b[c].max) / 2.0;  // centre()
        prims[t].orig = t;
    }
    out.rank.resize(n);
    out.order.resize(n);
    Box3 rb = box_empty(), trb;
    if (n) {
        Builder B{prims, false, tri_base};  // the reference's tree: its leaf order, its root box
        B.nodes.reserve(n);
        out.root = B.build(0, n, 0, rb);
        for (uint64_t i = 0; i < n; ++i) out.order[i] = prims[i].orig;
        for (uint64_t i = 0; i < n; ++i) out.rank[i] = prims[i].orig = i;
        Builder T{prims, true, tri_base};  // the traversal tree: SAH over the reference-ordered triangles (orig = rank)
        if (sah) {
            T.nodes.reserve(n);
            out.root = T.build(0, n, 0, trb);
            for (uint64_t i = 0; i < n; ++i) out.rank[i] = prims[i].orig;
        }
        out.nodes.swap(sah ? T.nodes : B.nodes);
        out.depth = sah ? T.max_depth : B.max_depth;
        // re-base interior node indices into the scene-wide node array
        for (auto& nd : out.nodes)
            for (int c = 0; c < 2; ++c)
                if (nd.child[c] >= 0) nd.child[c] += node_base;
        if (out.root >= 0) out.root += node_base;
    }
    box_to_layout(rb, out.root_box);
    return out;
}

WideTree collapse_wide(const std::vector<vr::Node>& nodes, const std::vector<vr::Bvh>& bvhs, bool greedy_only) {
    // greedy collapse; unless VR_SCENE_GREEDY_COLLAPSE, the SAH-optimal one instead wherever its (deeper) stack
    // bound keeps the kernel in the greedy tree's LDS stack class (24 / 32 / 48 entries; a larger
    // class would cost workgroups per CU): a node takes the DP expansion when its DP subtree fits
    auto class_limit = [](int st) { return st + 1 <= 24 ? 23 : (st + 1 <= 32 ? 31 : 47); };
    WideTree g, o;
    WideBuilder G(nodes, g.nodes4, false);
    g.roots.resize(bvhs.size());
    for (size_t i = 0; i < bvhs.size(); ++i) g.roots[i] = bvhs[i].root >= 0 ? G.collapse(bvhs[i].root, 0) : bvhs[i].root;
    g.stack = G.stack;
    bool use_dp = false;
    if (!greedy_only) {
        WideBuilder D(nodes, o.nodes4, true);
        D.limit = class_limit(G.stack);
        o.roots.resize(bvhs.size());
        for (size_t i = 0; i < bvhs.size(); ++i) {
            if (bvhs[i].root >= 0) D.plan_root(bvhs[i].root);
            o.roots[i] = bvhs[i].root >= 0 ? D.collapse(bvhs[i].root, 0) : bvhs[i].root;
        }
        o.stack = D.stack;
        use_dp = D.stack <= D.limit;  // (by construction)
    }
    WideTree& w4 = use_dp ? o : g;
    if (tuning_env("VR_WIDE_STATS")) {  // diagnostic: the collapse's SAH objective, sum SA(wide) / SA(root)
        double sum = 0.0, root = 0.0;
        for (const auto& w : w4.nodes4) {
            float u[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
            for (int k = 0; k < 4; ++k)
                if (w.child[k] != vr::kEmptyChild)
                    for (int j = 0; j < 6; ++j) u[j] = (j & 1) ? std::max(u[j], w.bound[j][k]) : std::min(u[j], w.bound[j][k]);
            const double a = (double)(u[1] - u[0]) * (u[3] - u[2]) + (double)(u[3] - u[2]) * (u[5] - u[4]) +
                             (double)(u[5] - u[4]) * (u[1] - u[0]);
            sum += a;
            if (&w == &w4.nodes4[0]) root = a;
        }
        std::fprintf(stderr, "vr wide tree: %zu nodes, stack %d, sum SA / SA(first root) %.4f (%s collapse)\n",
                     w4.nodes4.size(), w4.stack, sum / root, use_dp ? "DP" : "greedy");
    }
    return std::move(w4);
}

int32_t shape_wide(uint64_t n, int32_t node_base, int32_t tri_base, std::vector<int32_t>& desc, int& stack) {
    ShapeWide W{desc, stack, tri_base};
    return W.wide({0, n, node_base}, 0);
}

}  // namespace vrh
