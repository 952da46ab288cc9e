// bvh_build.cpp — the BVH builds, the node order and the stack rule of bvh_build.hpp.
#include "bvh_build.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rtb {

Item::Item(int id_, const double lo_[3], const double hi_[3], bool costly_, bool subtree_) : id(id_), subtree(subtree_), costly(costly_)
{
    for (int a = 0; a < 3; ++a) {
        lo[a] = lo_[a];
        hi[a] = hi_[a];
        c[a] = 0.5 * (lo[a] + hi[a]);
    }
}

SahParams sah_params(double c_isect, int max_leaf, int force_leaf, int root_leaf, int split_box_pairs,
                     int split_blas_pairs)
{
    SahParams p;
    if (c_isect > 0.0) p.c_isect = std::max(0.01, c_isect);
    if (max_leaf > 0) p.max_leaf = std::min(31, std::max(2, max_leaf));
    if (force_leaf > 0) p.force_leaf = std::min(31, std::max(1, force_leaf));
    if (root_leaf >= 0) p.root_leaf = std::min(31, root_leaf);
    if (split_box_pairs >= 0) p.split_box_pairs = split_box_pairs != 0;
    if (split_blas_pairs >= 0) p.split_blas_pairs = split_blas_pairs != 0;
    return p;
}

void to_f32_box(const double lo[3], const double hi[3], double pad_abs, float flo[3], float fhi[3])
{
    for (int a = 0; a < 3; ++a) {
        double mag = std::max(std::fabs(lo[a]), std::fabs(hi[a]));
        double pad = 1e-6 * (1.0 + mag) + pad_abs;
        double l = lo[a] - pad, h = hi[a] + pad;
        float fl = (float)l, fh = (float)h;
        if ((double)fl > l) fl = std::nextafter(fl, -INFINITY);
        if ((double)fh < h) fh = std::nextafter(fh, INFINITY);
        flo[a] = fl;
        fhi[a] = fh;
    }
}

namespace {

double area(const double lo[3], const double hi[3])
{
    double dx = std::max(0.0, hi[0] - lo[0]), dy = std::max(0.0, hi[1] - lo[1]), dz = std::max(0.0, hi[2] - lo[2]);
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

void bounds(const std::vector<Item>& items, int b, int e, double lo[3], double hi[3])
{
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int i = b; i < e; ++i)
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], items[i].lo[a]);
            hi[a] = std::max(hi[a], items[i].hi[a]);
        }
}

int make_leaf(const std::vector<Item>& items, int b, int e, std::vector<int32_t>& prim_refs)
{
    int first = (int)prim_refs.size();
    for (int i = b; i < e; ++i) prim_refs.push_back(items[i].id);
    return RT_LEAF_CODE(first, e - b);
}

void sort_by_centroid(std::vector<Item>& items, int b, int e, int axis)
{
    std::sort(items.begin() + b, items.begin() + e, [axis](const Item& x, const Item& y) {
        return x.c[axis] < y.c[axis] || (x.c[axis] == y.c[axis] && x.id < y.id);
    });
}

struct Sah {
    std::vector<Item>& items;
    const SahParams& p;
    const double pad_abs;
    const bool in_blas;
    std::vector<rt_bvh_node>& nodes;
    std::vector<int32_t>& prim_refs;

    int build_rec(int b, int e, int depth)
    {
        const int n = e - b;
        const double c_trav = 1.0;
        double plo[3], phi[3];
        bounds(items, b, e, plo, phi);
        double parea = area(plo, phi);
        const bool costly = p.split_box_pairs && std::any_of(items.begin() + b, items.begin() + e, [](const Item& it) { return it.costly; });
        const bool split_pair = costly || (p.split_blas_pairs && in_blas);
        if (n <= 1 || (n <= p.force_leaf && !split_pair) || (depth == 0 && n <= p.root_leaf)) return make_leaf(items, b, e, prim_refs);
        if (depth >= 20) {  // bound the traversal stack: median split on the widest centroid axis
            double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int i = b; i < e; ++i)
                for (int a = 0; a < 3; ++a) { clo[a] = std::min(clo[a], items[i].c[a]); chi[a] = std::max(chi[a], items[i].c[a]); }
            int ax = 0;
            for (int a = 1; a < 3; ++a) if (chi[a] - clo[a] > chi[ax] - clo[ax]) ax = a;
            return split_at(b, e, ax, n / 2, depth);
        }
        // full-sweep SAH over the three axes (centroid order; ties by prim index)
        double best_cost = INFINITY;
        int best_axis = -1, best_split = -1;
        std::vector<double> right_area(n);
        for (int axis = 0; axis < 3; ++axis) {
            sort_by_centroid(items, b, e, axis);
            double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int i = n - 1; i >= 1; --i) {
                for (int a = 0; a < 3; ++a) {
                    lo[a] = std::min(lo[a], items[b + i].lo[a]);
                    hi[a] = std::max(hi[a], items[b + i].hi[a]);
                }
                right_area[i] = area(lo, hi);
            }
            for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
            for (int i = 1; i < n; ++i) {
                for (int a = 0; a < 3; ++a) {
                    lo[a] = std::min(lo[a], items[b + i - 1].lo[a]);
                    hi[a] = std::max(hi[a], items[b + i - 1].hi[a]);
                }
                double cost = c_trav + p.c_isect * (area(lo, hi) * i + right_area[i] * (n - i)) / std::max(parea, 1e-300);
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = axis;
                    best_split = i;
                }
            }
        }
        double leaf_cost = p.c_isect * n;
        if (n <= p.max_leaf && leaf_cost <= best_cost) return make_leaf(items, b, e, prim_refs);
        if (best_axis < 0) best_axis = 0, best_split = n / 2;
        return split_at(b, e, best_axis, best_split, depth);
    }

    int split_at(int b, int e, int axis, int split, int depth)
    {
        sort_by_centroid(items, b, e, axis);
        int mid = b + split;
        int node = (int)nodes.size();
        nodes.emplace_back();
        double llo[3], lhi[3], rlo[3], rhi[3];
        bounds(items, b, mid, llo, lhi);
        bounds(items, mid, e, rlo, rhi);
        int lc = build_rec(b, mid, depth + 1);
        int rc = build_rec(mid, e, depth + 1);
        rt_bvh_node& nd = nodes[node];
        std::memset(&nd, 0, sizeof nd);
        to_f32_box(llo, lhi, pad_abs, nd.lo0, nd.hi0);
        to_f32_box(rlo, rhi, pad_abs, nd.lo1, nd.hi1);
        nd.child[0] = lc;
        nd.child[1] = rc;
        return node;
    }
};

}  // namespace

int build_sah(std::vector<Item>& items, const SahParams& p, double pad_abs, bool in_blas,
              std::vector<rt_bvh_node>& nodes, std::vector<int32_t>& prim_refs)
{
    if (items.empty()) return RT_LEAF_CODE((int)prim_refs.size(), 0);
    return Sah{items, p, pad_abs, in_blas, nodes, prim_refs}.build_rec(0, (int)items.size(), 0);
}

int build_chain(const std::vector<Item>& items, std::vector<rt_bvh_node>& nodes, std::vector<int32_t>& prim_refs)
{
    std::vector<int> segs;
    for (size_t i = 0; i < items.size();) {
        if (items[i].subtree) {
            segs.push_back(items[i].id);
            ++i;
            continue;
        }
        size_t j = i;
        while (j < items.size() && !items[j].subtree && j - i < 31) ++j;
        segs.push_back(make_leaf(items, (int)i, (int)j, prim_refs));
        i = j;
    }
    if (segs.empty()) return RT_LEAF_CODE((int)prim_refs.size(), 0);
    if (segs.size() == 1) return segs[0];
    const int base = (int)nodes.size(), n = (int)segs.size() - 1;
    nodes.resize(base + n);
    for (int k = 0; k < n; ++k) {
        rt_bvh_node& nd = nodes[base + k];
        std::memset(&nd, 0, sizeof nd);
        for (int a = 0; a < 3; ++a) {
            nd.lo0[a] = nd.lo1[a] = -INFINITY;
            nd.hi0[a] = nd.hi1[a] = INFINITY;
        }
        nd.child[0] = segs[k];
        nd.child[1] = k + 1 < n ? base + k + 1 : segs[n];
    }
    return base;
}

TlasFirst renumber_tlas_first(int root, std::vector<rt_bvh_node>& nodes, std::vector<rt_instance>& instances)
{
    if (root < 0) return TlasFirst{0, root};
    std::vector<int> order{root}, remap(nodes.size(), -1);
    remap[root] = 0;
    for (size_t i = 0; i < order.size(); ++i)
        for (int c : nodes[order[i]].child)
            if (c >= 0 && remap[c] < 0) {   // (a MEDIAN span-1 node names one child twice)
                remap[c] = (int)order.size();
                order.push_back(c);
            }
    const int n_tlas_nodes = (int)order.size();
    int next = n_tlas_nodes;
    for (size_t i = 0; i < nodes.size(); ++i)
        if (remap[i] < 0) remap[i] = next++;
    std::vector<rt_bvh_node> moved(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        rt_bvh_node nd = nodes[i];
        for (int& c : nd.child)
            if (c >= 0) c = remap[c];
        moved[remap[i]] = nd;
    }
    nodes.swap(moved);
    for (rt_instance& in : instances)
        if (in.child_kind == RT_CHILD_BVH && in.child >= 0) in.child = remap[in.child];
    return TlasFirst{n_tlas_nodes, remap[root]};
}

int stack_need(const rt_bvh_node* nodes, int ref, StackMemo& memo)
{
    if (ref < 0) return 0;
    std::vector<int>& need = memo.need;
    std::vector<uint8_t>& colour = memo.colour;
    std::vector<int> todo{ref};  // iterative post-order (a LINEAR chain can be long)
    while (!todo.empty()) {
        const int i = todo.back();
        if (colour[i] == 2) {
            todo.pop_back();
            continue;
        }
        const rt_bvh_node& nd = nodes[i];
        if (colour[i] == 0) {
            colour[i] = 1;
            for (int ch : nd.child) {
                if (ch < 0 || colour[ch] == 2) continue;
                if (colour[ch] == 1) return -1;  // back edge
                todo.push_back(ch);
            }
            continue;
        }
        todo.pop_back();  // both children done
        auto nc = [&](int ch) { return ch < 0 ? 0 : need[ch]; };
        const bool same = std::memcmp(nd.lo0, nd.lo1, 12) == 0 && std::memcmp(nd.hi0, nd.hi1, 12) == 0;
        need[i] = same ? std::max(1 + nc(nd.child[0]), nc(nd.child[1])) : 1 + std::max(nc(nd.child[0]), nc(nd.child[1]));
        colour[i] = 2;
    }
    return need[ref];
}

}  // namespace rtb
