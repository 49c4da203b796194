// lv_common.hpp — host declarations shared by lv_host.hpp, lv_rebuild.hpp, lv_filter.hpp, lv_exchange.hpp and lv_buffers.hpp (the
// last four must build without lv_host.hpp: their host tests compile them against a HIP stand-in, tests/emu/hip/hip_runtime.h; so
// do lv_occupancy.hpp, lv_distance.hpp and lv_plan.hpp, which include lv_buffers.hpp; lv_rules.hpp needs no HIP header at all and
// declares set_error itself).  set_error keeps the message lv_last_error returns
// (include/limovelo_hip.h), LV_HIP turns a failed HIP call into LV_EHIP.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/limovelo_hip.h"

namespace lv {

void set_error(const char* fmt, ...);

#define LV_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            ::lv::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return LV_EHIP;                                                                       \
        }                                                                                         \
    } while (0)

// Leaves the function with the code of a failed step (an int expression: LV_OK or an error whose message is set)
#define LV_TRY(expr)            \
    do {                        \
        const int _rc = (expr); \
        if (_rc) return _rc;    \
    } while (0)

// Leaves the function with `code` and the message unless cond holds
#define LV_REQUIRE(cond, code, msg) \
    do {                            \
        if (!(cond)) {              \
            ::lv::set_error(msg);   \
            return code;            \
        }                           \
    } while (0)

struct KfDev; struct FilterDev;
// lv_predict.hip: n <= PREDICT_BATCH steps {dt, acc[3], gyro[3]} with one Q in one launch, from kf->x / P_post if src != nullptr
constexpr int PREDICT_BATCH = 8;   // (== PREDICT_BATCH_MAX of lv_predict.hip)
int launch_predict(hipStream_t stream, FilterDev* f, const KfDev* src, const double* Q, int n, const double (*steps)[7]);
int launch_kf_to_filter(hipStream_t stream, const KfDev* kf, FilterDev* f);
// lv_observe.hip: n <= LV_OBSERVE_BATCH checked observations applied to f one after the other in one launch; d_results (device)
// receives one record each
int launch_observe(hipStream_t stream, FilterDev* f, const lv_observation* obs, int n, lv_observe_result* d_results);

void set_slice_pause_us(uint32_t us);   // lv_map.hip: the calling THREAD's sliced launches are spaced by that many microseconds (0: back to back)

}  // namespace lv
