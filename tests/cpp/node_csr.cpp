// build_node_csr (csrc/node_csr.hpp) against a per-node list built the slow way: for every node, every entry that names it, in the
// order the entries were given.  Stand-alone: includes node_csr.hpp alone, exits 0 when every case agrees.
#include "node_csr.hpp"

#include <cstdio>
#include <vector>

using namespace admm_lib;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("  FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the caller's entries: batch order, then local element order, then corner order; batch b's value of (element el, corner c) lies at
// base + 3 c n_local + el with stride n_local, as abi_gradient.inc lays its corner forces out
struct BatchCase { int nodes_per_elem; std::vector<int> idx; long long base; };

static std::vector<NodeCsrEntry> entries_of(const std::vector<BatchCase> &batches) {
    std::vector<NodeCsrEntry> out;
    for (const BatchCase &b : batches) {
        const int n_local = (int)b.idx.size() / b.nodes_per_elem;
        for (int el = 0; el < n_local; ++el) for (int c = 0; c < b.nodes_per_elem; ++c)
            out.push_back({b.idx[(size_t)el * b.nodes_per_elem + c], b.base + 3ll * c * n_local + el, n_local});
    }
    return out;
}

static void check_case(const char *name, int n_nodes, const std::vector<BatchCase> &batches) {
    std::printf("%s\n", name);
    const std::vector<NodeCsrEntry> entries = entries_of(batches);
    const NodeCsrHost h = build_node_csr(n_nodes, entries);
    CHECK(h.ptr.size() == (size_t)n_nodes + 1);
    CHECK(h.ptr[0] == 0 && h.ptr[n_nodes] == (int)entries.size());
    CHECK(h.off.size() == (entries.empty() ? 1 : entries.size()) && h.stride.size() == h.off.size());      // never empty: an empty list still uploads
    if (entries.empty()) CHECK(h.off[0] == 0 && h.stride[0] == 0);
    for (int i = 0; i < n_nodes; ++i) {
        std::vector<NodeCsrEntry> want;      // brute force
        for (const NodeCsrEntry &e : entries) if (e.node == i) want.push_back(e);
        CHECK(h.ptr[i + 1] - h.ptr[i] == (int)want.size());
        if (h.ptr[i + 1] - h.ptr[i] != (int)want.size()) continue;
        for (size_t k = 0; k < want.size(); ++k) CHECK(h.off[h.ptr[i] + k] == want[k].off && h.stride[h.ptr[i] + k] == want[k].stride);
    }
}

int main() {
    // 5 nodes, two batches (four tets-like elements of 4 nodes, three springs): node 3 is named by no element
    check_case("5 nodes, two batches, node 3 unnamed", 5, {{4, {0, 1, 2, 4, 4, 2, 1, 0, 0, 1, 2, 4, 1, 2, 4, 0}, 0}, {2, {0, 1, 4, 2, 1, 4}, 48}});
    {
        const NodeCsrHost h = build_node_csr(5, entries_of({{4, {0, 1, 2, 4}, 0}}));
        CHECK(h.ptr[3] == h.ptr[4]);      // the unnamed node's list is empty
    }
    // a degenerate element names node 1 twice: both entries, in corner order
    check_case("one node named twice by one element", 3, {{3, {1, 0, 1, 2, 1, 0}, 0}});
    {
        const NodeCsrHost h = build_node_csr(3, entries_of({{3, {1, 0, 1}, 7}}));
        CHECK(h.ptr[1] == 1 && h.ptr[2] == 3 && h.off[1] == 7 + 0 && h.off[2] == 7 + 6 && h.stride[1] == 1);
    }
    // an empty batch (n_local = 0 on this rank) between two others, and one alone
    check_case("an empty batch between two others", 4, {{2, {0, 1, 2, 3}, 0}, {3, {}, 12}, {1, {3, 0, 3}, 12}});
    check_case("only an empty batch", 4, {{3, {}, 0}});
    check_case("no batch", 2, {});
    check_case("n_nodes = 0", 0, {});
    check_case("n_nodes = 0 with an empty batch", 0, {{4, {}, 0}});
    if (failures) { std::printf("node_csr: %d check(s) FAILED\n", failures); return 1; }
    std::printf("node_csr: ok\n");
    return 0;
}
