// lv_common.hpp — host declarations shared by lv_host.hpp and lv_rebuild.hpp (which must build without lv_host.hpp: the host test
// compiles it against a HIP stand-in).  set_error keeps the message lv_last_error returns (include/limovelo_hip.h), LV_HIP turns a
// failed HIP call into LV_EHIP.
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

void set_slice_pause_us(uint32_t us);   // lv_map.hip: the calling THREAD's sliced launches are spaced by that many microseconds (0: back to back)

}  // namespace lv
