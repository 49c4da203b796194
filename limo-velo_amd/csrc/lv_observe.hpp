// lv_observe.hpp — the argument rules of lv_observe (include/limovelo_hip.h "Aiding observations"): what an observation is
// refused for (LV_EINVAL and the message; the first refusal wins, nothing is enqueued) and lv_default_observation's values.  Pure
// host arithmetic, no HIP header: plain g++ compiles it (tests/test_observe_host.py).
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/limovelo_hip.h"

namespace lv {

void set_error(const char* fmt, ...);

constexpr double OBS_QUAT_TOL = 1e-6;   // ATTITUDE: | |z| - 1 | beyond this is refused (the kernel does not normalise z)

inline void default_observation(lv_observation* o, int kind) {
    if (!o) return;
    o->kind = kind;
    o->mask = 7;
    for (int i = 0; i < 4; ++i) o->z[i] = 0.0;
    if (kind == LV_OBS_ATTITUDE) o->z[3] = 1.0;
    for (int i = 0; i < 9; ++i) o->R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) o->lever[i] = 0.0;
    o->gate = 0.0;
}

inline int observation_ok(const lv_observation& o, size_t at) {
    if (o.kind < LV_OBS_POSITION || o.kind > LV_OBS_ATTITUDE) { set_error("lv_observe: observation %zu: unknown kind %d", at, o.kind); return LV_EINVAL; }
    if (o.mask < 1 || o.mask > 7) { set_error("lv_observe: observation %zu: mask %d outside 1..7", at, o.mask); return LV_EINVAL; }
    const int nz = o.kind == LV_OBS_ATTITUDE ? 4 : 3;
    for (int i = 0; i < nz; ++i) if (!std::isfinite(o.z[i])) { set_error("lv_observe: observation %zu: non-finite z", at); return LV_EINVAL; }
    for (int i = 0; i < 9; ++i) if (!std::isfinite(o.R[i])) { set_error("lv_observe: observation %zu: non-finite R", at); return LV_EINVAL; }
    for (int i = 0; i < 3; ++i) if (!std::isfinite(o.lever[i])) { set_error("lv_observe: observation %zu: non-finite lever", at); return LV_EINVAL; }
    if (o.kind != LV_OBS_POSITION && (o.lever[0] != 0.0 || o.lever[1] != 0.0 || o.lever[2] != 0.0)) {
        set_error("lv_observe: observation %zu: a lever arm goes with LV_OBS_POSITION only", at);
        return LV_EINVAL;
    }
    if (!(o.gate >= 0.0) || !std::isfinite(o.gate)) { set_error("lv_observe: observation %zu: gate must be finite and >= 0", at); return LV_EINVAL; }
    if (o.kind == LV_OBS_ATTITUDE) {
        const double nrm = std::sqrt(o.z[0] * o.z[0] + o.z[1] * o.z[1] + o.z[2] * o.z[2] + o.z[3] * o.z[3]);
        if (!(std::fabs(nrm - 1.0) <= OBS_QUAT_TOL)) { set_error("lv_observe: observation %zu: z is not a unit quaternion (|z| = %.9g)", at, nrm); return LV_EINVAL; }
    }
    return LV_OK;
}

// the whole call: obs, n and every observation
inline int observations_ok(const lv_observation* obs, size_t n) {
    if (!obs) { set_error("lv_observe: null observations"); return LV_EINVAL; }
    if (n < 1 || n > LV_OBSERVE_BATCH) { set_error("lv_observe: %zu observations: one call takes 1..%d", n, LV_OBSERVE_BATCH); return LV_EINVAL; }
    for (size_t i = 0; i < n; ++i)
        if (int r = observation_ok(obs[i], i)) return r;
    return LV_OK;
}

}  // namespace lv
