// node_csr.hpp -- the per-node lists that gradient_gather_kernel (kernels_gradient.hpp) and reaction_gather_kernel (kernels_reaction.hpp)
// walk, as a CSR over the caller's nodes.  Free of HIP: build_node_csr is a pure function (tests/cpp/node_csr.cpp); the device's copy is
// three pointers (NodeCsr), filled by upload_node_csr (abi_gradient.inc).
// An entry names a node and where its value lies: row r at buf[off + r * stride].  The callers list their entries in batch order, then
// local element order, then their own corner order; build_node_csr keeps that order inside every node (a counting sort): node i owns
// off[ptr[i] .. ptr[i + 1]) and stride likewise.  off and stride hold at least one element, so that an empty list still uploads.
#pragma once
#include <algorithm>
#include <vector>

namespace admm_lib {

struct NodeCsrEntry { int node; long long off; int stride; };
struct NodeCsrHost { std::vector<int> ptr; std::vector<long long> off; std::vector<int> stride; };
struct NodeCsr { int *ptr = nullptr; long long *off = nullptr; int *stride = nullptr; };      // the device's copy

inline NodeCsrHost build_node_csr(int n_nodes, const std::vector<NodeCsrEntry> &entries) {
    NodeCsrHost h;
    h.ptr.assign((size_t)n_nodes + 1, 0);
    for (const NodeCsrEntry &e : entries) h.ptr[(size_t)e.node + 1]++;
    for (int i = 0; i < n_nodes; ++i) h.ptr[i + 1] += h.ptr[i];
    std::vector<int> pos(h.ptr.begin(), h.ptr.end() - 1);
    h.off.assign(std::max<size_t>(entries.size(), 1), 0);
    h.stride.assign(h.off.size(), 0);
    for (const NodeCsrEntry &e : entries) { const int k = pos[e.node]++; h.off[k] = e.off; h.stride[k] = e.stride; }
    return h;
}

} // namespace admm_lib
