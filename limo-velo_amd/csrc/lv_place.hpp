// lv_place.hpp — place recognition: a database of Scan Context descriptors on the device and their brute-force retrieval
// (include/limovelo_hip.h "Place recognition"; kernels and host side in lv_place.hip).
#pragma once
#include "lv_host.hpp"
#include "lv_rules.hpp"   // PLACE_MAX_*

namespace lv {

constexpr int PLACE_TOPK_CHUNK = 4096;                      // keys per workgroup of the top-k selection (256 lanes x 16)

// The rule as the kernels take it: ring_w = (rmax - rmin) / n_rings and sector_w = 2 pi / n_sectors in f32
struct PlaceRule {
    int n_rings, n_sectors, n_bins;
    float rmin, rmax, z_offset, ring_w, sector_w;
};

// M = R_x R_off of a query state, rounded to f32 (row-major)
struct PlaceFrame {
    float M[9];
};

// The database: descriptors (ring-major, n_bins floats each) on the device, centres on the host.  Grown on demand, kept until
// configure / clear shrink the count; released by lv_destroy.
struct PlaceStore {
    lv_place_params prm{20, 60, 0.f, 80.f, 2.f};
    size_t n = 0;                      // places held
    std::vector<double> centres;       // 3 n
    DevBuf<float> d_desc;              // room for d_desc.cap / n_bins places
    DevBuf<uint32_t> d_q;              // the query descriptor (f32 bits), PLACE_MAX_BINS
    DevBuf<uint64_t> d_keys;           // one retrieval key per place: (distance bits << 32) | (id << 6) | shift
    DevBuf<uint64_t> d_top[2];         // the top-k stages, ping-pong
    DevBuf<float4> d_cent;             // lv_place_add_map: the call's centres in f32 and their 2-D grid (CSR)
    DevBuf<uint32_t> d_cstart;         // cells + 1 starts, then the call's items
    uint32_t* d_citems = nullptr;      // (inside d_cstart)

    PlaceRule rule() const;
    int bins() const { return prm.n_rings * prm.n_sectors; }
    // room for `want` places (keeps the first n)
    int reserve(hipStream_t stream, size_t want);
    // the descriptor of `scan` in frame f, accumulated (u32 atomicMax) into out (n_bins zeroed dwords on the device)
    int describe(const ScanStore& scan, hipStream_t stream, const PlaceFrame& f, uint32_t* out);
    int add_scan(const ScanStore& scan, hipStream_t stream, const PlaceFrame& f, const double centre[3], uint32_t* id);
    int add_map(const MapStore& map, hipStream_t stream, const double* cs, size_t k, uint32_t* first_id);
    // the k (<= n) nearest places to the descriptor in d_q: ids, shifts, distances in retrieval order.  Synchronises the stream.
    int query(hipStream_t stream, int k, uint32_t* ids, int32_t* shifts, float* dist);
    int load(hipStream_t stream, const float* desc, const double* cs, size_t k);
    int fetch(hipStream_t stream, float* desc, double* cs) const;
    void clear() { n = 0; centres.clear(); }
    void release();
};

// x -> (M = R_x R_off in f64 rounded to f32, centre = R_x t_off + x.pos in f64)
void place_frame(const lv_state& x, PlaceFrame* f, double centre[3]);

}  // namespace lv
