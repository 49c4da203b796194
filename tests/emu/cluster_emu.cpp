// tests/emu/cluster_emu.cpp — TEST INFRASTRUCTURE ONLY: the host part of limo-velo_amd/csrc/lv_cluster.hpp (the union-find by
// minimum id, the ordering key, the size rules) compiled with g++ against tests/emu/hip/hip_runtime.h, whose atomics are
// sequential.  It links a given edge list in the given order and prints the canonical labels, as the kernels of lv_cluster.hip
// produce them from the same functions.
//
// stdin (text):  n min_size max_size n_edges
//                n bytes-as-integers: the mask (0 = excluded)
//                n_edges pairs a b, in the order they are to be linked
// stdout:        C, then the n labels, then the C sizes
#define LV_CLUSTER_HOST_ONLY 1
#include "lv_cluster.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

int main() {
    unsigned n = 0, min_size = 1, max_size = 0, n_edges = 0;
    if (scanf("%u %u %u %u", &n, &min_size, &max_size, &n_edges) != 4) return 2;
    std::vector<uint32_t> parent(n), size(n, 0u);
    for (unsigned i = 0; i < n; ++i) {
        unsigned in = 0;
        if (scanf("%u", &in) != 1) return 2;
        parent[i] = in ? i : lv::CL_NONE;   // cluster_init_kernel
    }
    for (unsigned e = 0; e < n_edges; ++e) {   // cluster_link_kernel: a hit counts only between included points
        unsigned a = 0, b = 0;
        if (scanf("%u %u", &a, &b) != 2 || a >= n || b >= n) return 2;
        if (parent[a] == lv::CL_NONE || parent[b] == lv::CL_NONE) continue;
        lv::cl_link(parent.data(), a, b);
    }
    for (unsigned i = 0; i < n; ++i) {   // cluster_flatten_kernel
        if (parent[i] == lv::CL_NONE) continue;
        const uint32_t root = lv::cl_root(parent.data(), i);
        lv::cl_store(&parent[i], root);
        atomicAdd(&size[root], 1u);
    }
    std::vector<uint64_t> keys;   // cluster_flag_kernel / cluster_key_kernel / the sort
    for (unsigned i = 0; i < n; ++i)
        if (parent[i] == i && lv::cl_reported(size[i], min_size, max_size)) keys.push_back(lv::cl_order_key(size[i], i));
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> lab(n, -1);   // cluster_number_kernel
    for (size_t j = 0; j < keys.size(); ++j) lab[lv::cl_key_root(keys[j])] = (int32_t)j;
    printf("%zu\n", keys.size());
    for (unsigned i = 0; i < n; ++i) printf("%d\n", parent[i] == lv::CL_NONE ? -1 : lab[parent[i]]);   // cluster_scatter_kernel
    for (uint64_t k : keys) printf("%u\n", lv::cl_key_size(k));
    // the removal rule, both modes, on a few sizes (checked by the test against its own statement)
    for (uint32_t s : {1u, 4u, 5u, 9u, 10u, 11u})
        printf("%d %d %d\n", (int)lv::cl_removed(s, 5, 10, false, false), (int)lv::cl_removed(s, 5, 10, true, true), (int)lv::cl_removed(s, 5, 10, true, false));
    return 0;
}
