// bvh_build_main.cpp — drives csrc/bvh_build.cpp (the BVH builds, the node order's stack rule: no
// HIP, no World) on the smallest inputs where each of its rules can go wrong, for
// tests/test_bvh_build.py. Links bvh_build.cpp alone. One JSON line per case: the root, the
// node count, the stack need, and what holds for every tree: each item's prim exactly once in
// the leaves under the root (prims_once), the largest leaf (max_leaf), and every f32 child box
// around the f64 boxes of all items below it (contained).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "bvh_build.hpp"

namespace {

using rtb::Item;

Item box_item(int id, double cx, double cy, double cz, double half, bool costly = false)
{
    const double lo[3] = {cx - half, cy - half, cz - half}, hi[3] = {cx + half, cy + half, cz + half};
    return Item(id, lo, hi, costly);
}

// n small boxes along x, staggered in y and z, prims first, first + 1, ...
std::vector<Item> row(int n, int first = 0)
{
    std::vector<Item> items;
    for (int i = 0; i < n; ++i) items.push_back(box_item(first + i, 1.0 * i, 0.5 * (i % 3), 0.25 * (i % 2), 0.3));
    return items;
}

// the boxes of tests/lower_dump.cpp's concentric_200: spheres at the origin, radii over 2^60
std::vector<Item> concentric(int n)
{
    std::vector<Item> items;
    for (int i = 0; i < n; ++i) items.push_back(box_item(i, 0.0, 0.0, 0.0, std::ldexp(1.0, i % 60) * (1 + i / 60)));
    return items;
}

struct Tree {
    std::vector<rt_bvh_node> nodes;
    std::vector<int32_t> prim_refs;
    std::map<int, Item> by_prim;   // every item the tree was built over
    void know(const std::vector<Item>& items)
    {
        for (const Item& it : items)
            if (!it.subtree) by_prim.emplace(it.id, it);
    }
};

struct Found {
    std::map<int, int> times;   // prim -> how often a leaf under the root holds it
    int max_leaf = 0;
    bool contained = true;
};

// the prims under ref, checking the child boxes of every node on the way
std::vector<int> below(const Tree& t, int ref, Found& f)
{
    std::vector<int> prims;
    if (ref < 0) {
        const int code = ~ref, first = code >> 5, count = code & 31;
        f.max_leaf = std::max(f.max_leaf, count);
        for (int j = first; j < first + count; ++j) {
            prims.push_back(t.prim_refs[(size_t)j]);
            f.times[t.prim_refs[(size_t)j]]++;
        }
        return prims;
    }
    const rt_bvh_node& nd = t.nodes[(size_t)ref];
    for (int c = 0; c < 2; ++c) {
        const float* lo = c ? nd.lo1 : nd.lo0;
        const float* hi = c ? nd.hi1 : nd.hi0;
        for (int p : below(t, nd.child[c], f)) {
            const Item& it = t.by_prim.at(p);
            for (int a = 0; a < 3; ++a) f.contained = f.contained && (double)lo[a] <= it.lo[a] && it.hi[a] <= (double)hi[a];
            prims.push_back(p);
        }
    }
    return prims;
}

void report(const char* name, const Tree& t, int root, const std::string& extra = "")
{
    Found f;
    below(t, root, f);
    bool once = f.times.size() == t.by_prim.size();
    for (const auto& kv : f.times) once = once && kv.second == 1 && t.by_prim.count(kv.first);
    rtb::StackMemo memo;
    memo.resize(t.nodes.size());
    std::printf("{\"case\": \"%s\", \"root\": %d, \"root_leaf_count\": %d, \"n_nodes\": %zu, \"n_prim_refs\": %zu, \"need\": %d, "
                "\"prims_once\": %s, \"max_leaf\": %d, \"contained\": %s%s}\n",
                name, root, root < 0 ? (~root) & 31 : -1, t.nodes.size(), t.prim_refs.size(),
                rtb::stack_need(t.nodes.data(), root, memo), once ? "true" : "false", f.max_leaf,
                f.contained ? "true" : "false", extra.c_str());
}

// root_leaf 0: no whole-BVH leaf, so the rules for small sets decide at the root too
void sah(const char* name, std::vector<Item> items, bool in_blas = false, int root_leaf = rtb::SahParams().root_leaf)
{
    Tree t;
    t.know(items);
    rtb::SahParams p;
    p.root_leaf = root_leaf;
    const int root = rtb::build_sah(items, p, 0x1.0p-18 * 8.0, in_blas, t.nodes, t.prim_refs);
    report(name, t, root);
}

// the chain's segments in list order: "leaf:COUNT" or "node:INDEX", and whether every box is unbounded
void chain(const char* name, const std::vector<Item>& items, Tree t = Tree())
{
    const size_t before = t.nodes.size();
    t.know(items);
    const int root = rtb::build_chain(items, t.nodes, t.prim_refs);
    auto seg = [](int ref) { return ref < 0 ? "\"leaf:" + std::to_string((~ref) & 31) + "\"" : "\"node:" + std::to_string(ref) + "\""; };
    std::string segs;
    bool unbounded = true;
    int ref = root;
    while (ref >= (int)before) {   // the chain's own nodes
        const rt_bvh_node& nd = t.nodes[(size_t)ref];
        for (int a = 0; a < 3; ++a)
            unbounded = unbounded && nd.lo0[a] == -INFINITY && nd.lo1[a] == -INFINITY && nd.hi0[a] == INFINITY && nd.hi1[a] == INFINITY;
        segs += seg(nd.child[0]) + ", ";
        ref = nd.child[1];
    }
    segs += seg(ref);
    report(name, t, root, ", \"chain_nodes\": " + std::to_string(t.nodes.size() - before) + ", \"segments\": [" + segs +
                              "], \"unbounded\": " + (unbounded ? "true" : "false"));
}

// a node over two children with differing or bit-identical child boxes
rt_bvh_node node(int c0, int c1, bool same)
{
    rt_bvh_node nd;
    std::memset(&nd, 0, sizeof nd);
    for (int a = 0; a < 3; ++a) {
        nd.lo0[a] = -1.0f, nd.hi0[a] = 1.0f;
        nd.lo1[a] = -1.0f, nd.hi1[a] = same ? 1.0f : 2.0f;
    }
    nd.child[0] = c0;
    nd.child[1] = c1;
    return nd;
}

void stack_rule()
{
    const int L = RT_LEAF_CODE(0, 1);
    // 0: a leaf pair (need 1); 1: a node over it (need 2); then the nodes under test, each over a
    // child of need n0 and one of need n1
    std::vector<rt_bvh_node> nodes = {node(L, L, false), node(0, L, false)};
    struct Case {
        const char* name;
        int c0, c1;
        bool same;
    };
    const Case cases[6] = {{"differ_1_2", 0, 1, false}, {"differ_2_1", 1, 0, false}, {"same_1_2", 0, 1, true},
                           {"same_2_1", 1, 0, true},    {"same_0_0", L, L, true},    {"differ_0_0", L, L, false}};
    for (const Case& c : cases) nodes.push_back(node(c.c0, c.c1, c.same));
    rtb::StackMemo memo;
    memo.resize(nodes.size());
    std::printf("{\"case\": \"stack_rule\", \"leaf\": %d", rtb::stack_need(nodes.data(), L, memo));
    for (int pass = 0; pass < 2; ++pass)   // the second pass reads the shared memo
        for (int i = 0; i < 6; ++i)
            std::printf(", \"%s%s\": %d", cases[i].name, pass ? "_again" : "", rtb::stack_need(nodes.data(), 2 + i, memo));
    // nodes appended later, over a subtree already walked: the memo grows
    nodes.push_back(node(2, 3, false));
    memo.resize(nodes.size());
    std::printf(", \"appended\": %d", rtb::stack_need(nodes.data(), (int)nodes.size() - 1, memo));
    // a two-node cycle
    std::vector<rt_bvh_node> loop = {node(1, L, false), node(0, L, false)};
    rtb::StackMemo fresh;
    fresh.resize(loop.size());
    std::printf(", \"cycle\": %d}\n", rtb::stack_need(loop.data(), 0, fresh));
}

}  // namespace

int main()
{
    sah("sah_0", {});
    sah("sah_1", row(1));
    sah("sah_2_plain", row(2), false, 0);
    {
        std::vector<Item> two = row(2);
        two[1].costly = true;
        sah("sah_2_costly", two, false, 0);
        sah("sah_2_costly_whole_bvh", two);   // root_leaf 8 comes first
    }
    sah("sah_2_in_blas", row(2), /*in_blas=*/true, 0);
    sah("sah_8", row(8));
    sah("sah_9", row(9));
    sah("sah_100", row(100));
    sah("sah_concentric_200", concentric(200));

    chain("chain_0", {});
    chain("chain_31", row(31));
    chain("chain_32", row(32));
    {   // a prebuilt subtree (its root a node) between two runs of primitives
        Tree t;
        std::vector<Item> sub = row(9, 100);
        t.know(sub);
        const int sub_root = rtb::build_sah(sub, rtb::SahParams(), 0.0, false, t.nodes, t.prim_refs);
        std::vector<Item> items = row(3);
        const double lo[3] = {-1.0, -1.0, -1.0}, hi[3] = {9.0, 2.0, 1.0};
        items.push_back(Item(sub_root, lo, hi, false, /*subtree=*/true));
        for (const Item& it : row(2, 50)) items.push_back(it);
        chain("chain_subtree", items, t);
    }
    stack_rule();

    {   // TLAS first: a BLAS node built before the TLAS, whose root names one child twice (a MEDIAN span-1 node)
        const int L = RT_LEAF_CODE(0, 1);
        std::vector<rt_bvh_node> nodes = {node(L, L, false), node(2, 2, true), node(L, L, false)};
        std::vector<rt_instance> instances(2);
        std::memset(instances.data(), 0, 2 * sizeof(rt_instance));
        instances[0].child_kind = RT_CHILD_BVH, instances[0].child = 0;
        instances[1].child_kind = RT_CHILD_PRIM, instances[1].child = 0;
        const rtb::TlasFirst t = rtb::renumber_tlas_first(1, nodes, instances);
        std::printf("{\"case\": \"renumber\", \"n_tlas_nodes\": %d, \"root\": %d, \"n_nodes\": %zu, \"root_children\": [%d, %d], "
                    "\"blas_root\": %d, \"prim_child\": %d, \"leaf_root\": %d}\n",
                    t.n_tlas_nodes, t.root, nodes.size(), nodes[0].child[0], nodes[0].child[1], instances[0].child,
                    instances[1].child, rtb::renumber_tlas_first(L, nodes, instances).root == L);
    }
    // the clamps of the build options
    const rtb::SahParams d = rtb::sah_params(0.0, 0, 0, -1, -1, -1), c = rtb::sah_params(1e-9, 1, 99, 99, 0, 5);
    std::printf("{\"case\": \"params\", \"default\": [%g, %d, %d, %d, %d, %d], \"clamped\": [%g, %d, %d, %d, %d, %d]}\n", d.c_isect,
                d.max_leaf, d.force_leaf, d.root_leaf, (int)d.split_box_pairs, (int)d.split_blas_pairs, c.c_isect, c.max_leaf,
                c.force_leaf, c.root_leaf, (int)c.split_box_pairs, (int)c.split_blas_pairs);
    return 0;
}
