// lv_host.hpp — host-side state behind the C-ABI (include/limovelo_hip.h).
#pragma once
#include "lv_note.hpp"

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/limovelo_hip.h"
#include "lv_device.hpp"
#include "lv_common.hpp"
#include "lv_buffers.hpp"
#include "lv_exchange.hpp"
#include "lv_update.hpp"
#include "lv_mapinc.hpp"
#include "lv_stores.hpp"

namespace lv {

// Map queries (lv_query.hip): batched k-NN / radius / box searches of arbitrary points against the active store.  Owns its staging
// and result buffers (grown on demand, freed by release); nothing here is shared with the update or the background rebuild.
struct QueryStore {
    PointStage pts;                // queries, packed xyz (doubling from QUERY_FLOOR floats)
    DevBuf<uint32_t> d_idx;        // k-NN: n x k results; radius: the ids found; box: the ranks found
    DevBuf<float> d_d2;            // k-NN / radius: their distances; box: their xyz
    DevBuf<int32_t> d_found;
    DevBuf<uint32_t> d_idx2;       // radius: the segmented sort's output
    DevBuf<float> d_d22;
    DevBuf<uint32_t> d_off;        // box: positions (n_ids + 1)
    DevBuf<uint32_t> d_cnt;        // box: flags by id
    DevBuf<uint64_t> d_roff;       // radius: per-query counts -> exclusive offsets of the queries' segments (n + 1), 64-bit
    DevBuf<uint64_t> d_rcnt;
    DevBuf<void> d_tmp;            // hipcub scratch
    DevBuf<uint32_t> d_rank;       // rank among the living by id, valid for the map whose stamp is rank_gen
    DevBuf<uint32_t> d_flag;
    uint64_t rank_gen = 0;
    PinBuf<uint32_t> h_word;       // a total read back by the host
    int stage_queries(hipStream_t stream, const void* q, size_t stride, size_t n);
    // nullptr when ranks equal ids (no dead id); else d_rank, rebuilt when the map's stamp moved
    int ensure_rank(const MapStore& map, hipStream_t stream, const uint32_t** rank);
    int knn(const MapStore& map, hipStream_t stream, const void* q, size_t stride, size_t n, int k, float max_dist, uint32_t* idx, float* d2,
            int32_t* found);
    int radius(const MapStore& map, hipStream_t stream, const void* q, size_t stride, size_t n, float radius, size_t* offsets, uint32_t* idx,
               float* d2, size_t capacity, size_t* total);
    int box(const MapStore& map, hipStream_t stream, const float lo[3], const float hi[3], uint32_t* idx, float* xyz, size_t capacity,
            size_t* n_out);
    void release();
};

// Multi-hypothesis passes and updates of the current scan (lv_batch.hip: lv_iterate_batch / lv_update_batch).  Its own
// buffers, grown on demand and kept: the hypothesis records (all M), the hand-over records and block partials of one chunk of
// hypotheses, and a KfDev that only knn_search's counters write (the context's kf is never touched by a batch).
struct BatchHyp;
// bytes of hand-over records (qrec_slots(K) x 16 B per point and hypothesis: 128 B for K = 5) one chunk may use; a batch with
// more is processed chunk after chunk (results do not depend on the chunking)
constexpr size_t BATCH_RECORD_BUDGET = (size_t)256 << 20;
struct BatchStore {
    DevBuf<BatchHyp> d_hyp;
    PinBuf<BatchHyp> h_hyp;
    DevBuf<float4> d_qrec;
    DevBuf<double> d_part;
    DevBuf<KfDev> d_sink;
    int chunk_hyp = 0;             // lv_set_option "batch_chunk_hypotheses": at most this many hypotheses per chunk (0: the budget alone)
    size_t chunk_size(uint32_t n, int num_match) const;
    // m hypotheses xs (prior covariance P) against the map and the scan (n sorted points): solve = false runs one pass without
    // a solve (lv_iterate_batch).  Outputs (each optional): final states, posterior covariances (m x 529), passes, the record
    // of each hypothesis' last pass (m x SUMS_LEN).  Returns once the host arrays are written.
    int run(const lv_params& prm, int max_blocks, const MapView& map, const float4* scan, uint32_t n, hipStream_t stream, const lv_state* xs,
            size_t m, const double* P, bool solve, lv_state* x_out, double* P_out, int* passes, double* recs);
    void release();
};

// (the launches of the update, their parameter structs and the driver that issues them: lv_update.hpp)
// lv_predict.hip
int launch_filter_to_kf(hipStream_t stream, const FilterDev* f, KfDev* kf);
// (the map, the scan and the LiDAR buffer, with the growth of their memory: lv_stores.hpp)

}  // namespace lv
