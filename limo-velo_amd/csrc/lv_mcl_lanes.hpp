// lv_mcl_lanes.hpp — the group of G lanes that serves one particle in mcl_particle (lv_mcl.hpp) on the device: what mcl_kernel of
// lv_mcl.hip and mclf_weigh_kernel of lv_mcl_filter.hip share.  hipcc only.
#pragma once

#include "lv_mcl.hpp"

namespace lv {

template <int G>
struct MclLanes {
    int g;
    __device__ int first() const { return g; }
    __device__ int stride() const { return G; }
    __device__ void beam(const float* beams, int b, float& ex, float& ey, float& ez) const {
        ex = beams[3 * b];
        ey = beams[3 * b + 1];
        ez = beams[3 * b + 2];
    }
    __device__ uint32_t cost(const uint32_t* table, uint32_t idx) const { return table[idx]; }
    __device__ uint64_t sum(uint64_t v) const {
        return (uint64_t)group_fold<G>((unsigned long long)v, [](unsigned long long a, unsigned long long b) { return a + b; });
    }
    __device__ uint32_t count(uint32_t v) const {
        return group_fold<G>(v, [](uint32_t a, uint32_t b) { return a + b; });
    }
};

}  // namespace lv
