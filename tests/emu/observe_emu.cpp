// tests/emu/observe_emu.cpp — HOST test of ResidentFilter::observe (limo-velo_amd/csrc/lv_filter.hpp) and of the argument rules
// of lv_observe (limo-velo_amd/csrc/lv_observe.hpp).
// TEST INFRASTRUCTURE ONLY: built by tests/test_observe_host.py into tests/emu/_build/ (once plain, once with AddressSanitizer +
// UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own ResidentFilter against the stand-in hip_runtime.h
// next to this file, with fake launches that apply toy arithmetic to the buffer they are told to use (a wrong source or a wrong
// order gives a wrong value); the HIP stand-in logs every call, so a scenario asserts what each step enqueued and where the
// filter is afterwards.  Usage: observe_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <limits>
#include <memory>

#include "../../limo-velo_amd/csrc/lv_filter.hpp"

using namespace lv;
using Where = ResidentFilter::Where;
using Source = ResidentFilter::Source;

static char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// (variadic: a braced list of calls inside the condition carries commas)
#define CHECK(...)                                                                                                  \
    do {                                                                                                            \
        if (!(__VA_ARGS__)) {                                                                                       \
            fprintf(stderr, "CHECK FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #__VA_ARGS__, g_err); \
            std::_Exit(1);                                                                                          \
        }                                                                                                           \
    } while (0)

namespace {

// ---- toy arithmetic: deterministic, not commutative between the three kinds of step
void toy_step(double* x, double* P, const double* Q, const double* st) {
    for (int j = 0; j < NX; ++j) x[j] = x[j] * 0.75 + st[0] * (j + 1) + st[1 + j % 6] * 0.125;
    for (int k = 0; k < NS * NS; ++k) P[k] = P[k] * 0.5 + Q[k % 144] * st[0];
}
void toy_update(double* x, double* P) {
    for (int j = 0; j < NX; ++j) x[j] = x[j] * 0.5 + 1.0 / (j + 1);
    for (int k = 0; k < NS * NS; ++k) P[k] = P[k] * 0.25 + 0.01;
}
void toy_observe(double* x, double* P, const lv_observation& o) {
    for (int j = 0; j < NX; ++j) x[j] = x[j] * 0.875 + o.z[j % 3] * 0.25 + o.kind;
    for (int k = 0; k < NS * NS; ++k) P[k] = P[k] * 0.625 + o.R[k % 9] * o.mask;
}

struct ObserveLaunch { int n; const FilterDev* f; };
std::vector<ObserveLaunch> g_observes;
std::vector<int> g_predict_n;
std::vector<bool> g_predict_from_kf;

}  // namespace

// ---- the fakes of lv_predict.hip and lv_observe.hip
int lv::launch_predict(hipStream_t s, FilterDev* f, const KfDev* src, const double* Q, int n, const double (*steps)[7]) {
    emu_hip::call("launch_predict", s);
    g_predict_n.push_back(n);
    g_predict_from_kf.push_back(src != nullptr);
    FilterDev t;
    std::memcpy(t.x, src ? src->x : f->x, sizeof(t.x));
    std::memcpy(t.P, src ? src->P_post : f->P, sizeof(t.P));
    for (int i = 0; i < n; ++i) toy_step(t.x, t.P, Q, steps[i]);
    *f = t;
    return LV_OK;
}
int lv::launch_kf_to_filter(hipStream_t s, const KfDev* kf, FilterDev* f) {
    emu_hip::call("launch_kf_to_filter", s);
    std::memcpy(f->x, kf->x, sizeof(f->x));
    std::memcpy(f->P, kf->P_post, sizeof(f->P));
    return LV_OK;
}
int lv::launch_observe(hipStream_t s, FilterDev* f, const lv_observation* obs, int n, lv_observe_result* d_results) {
    emu_hip::call("launch_observe", s);
    g_observes.push_back({n, f});
    for (int i = 0; i < n; ++i) {
        toy_observe(f->x, f->P, obs[i]);
        d_results[i].status = 0;
        d_results[i].rows = __builtin_popcount((unsigned)obs[i].mask);
    }
    return LV_OK;
}

namespace {

using Calls = std::vector<std::string>;
Calls calls(size_t from) {
    Calls v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i) v.push_back(log[i].call);
    return v;
}
size_t mark() { return emu_hip::state().log.size(); }
const Calls UPLOAD = {"hipMemcpyAsync", "hipEventCreateWithFlags", "hipEventRecord"};
Calls operator+(Calls a, const Calls& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

struct Logical { double x[NX], P[NS * NS]; };
Logical seed(double v) {
    Logical m;
    for (int j = 0; j < NX; ++j) m.x[j] = v + j;
    for (int k = 0; k < NS * NS; ++k) m.P[k] = (k % (NS + 1) == 0) ? v : 0.001 * k;
    return m;
}

double g_Q[144];
const double g_acc[3] = {0.1, -0.2, 9.81}, g_gyro[3] = {0.01, 0.02, -0.03};
void model_predict(Logical& m, double dt) {
    const double st[7] = {dt, g_acc[0], g_acc[1], g_acc[2], g_gyro[0], g_gyro[1], g_gyro[2]};
    toy_step(m.x, m.P, g_Q, st);
}

lv_observation good(int kind, double z0 = 0.5) {
    lv_observation o;
    default_observation(&o, kind);
    if (kind != LV_OBS_ATTITUDE) { o.z[0] = z0; o.z[1] = -2.0 * z0; o.z[2] = 0.25; }
    o.R[0] = 0.04; o.R[4] = 0.09; o.R[8] = 0.01; o.R[1] = o.R[3] = 0.002;
    return o;
}

// a context as lv_api.hip holds it
struct Ctx {
    ResidentFilter f;
    std::unique_ptr<KfDev> kf{new KfDev()};
    KfHostIO io{};
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    lv_observe_result res[LV_OBSERVE_BATCH] = {};
    long resyncs = 0;
    Ctx() { CHECK(f.alloc() == LV_OK); }
    ~Ctx() { f.release(); }
    int set(const Logical& m) { return f.set(reinterpret_cast<const lv_state*>(m.x), m.P); }
    int predict(double dt) { return f.predict(s, kf.get(), dt, g_Q, g_acc, g_gyro); }
    int observe(const lv_observation* o, size_t n) { return f.observe(s, kf.get(), o, n, res); }
    // lv_correct as lv_api.hip drives the filter; the fake passes leave the posterior of the prior in kf
    int correct(Logical* m) {
        if (int r = f.need("lv_correct")) return r;
        if (int r = f.flush(s, kf.get())) return r;
        f.latest = Source::Filter;
        const ResidentFilter::Prior pr = f.prior();
        if (int r = f.begin_update(s, kf.get(), pr.dev != nullptr)) return r;
        if (pr.host) {
            std::memcpy(kf->x, pr.host, sizeof(kf->x));
            std::memcpy(kf->P_post, pr.host + NX, sizeof(kf->P_post));
        } else if (!pr.dev_in_kf) {
            std::memcpy(kf->x, pr.dev->x, sizeof(kf->x));
            std::memcpy(kf->P_post, pr.dev->P, sizeof(kf->P_post));
        }
        emu_hip::call("update", s);
        toy_update(kf->x, kf->P_post);
        if (m) toy_update(m->x, m->P);
        f.correct_done();
        return LV_OK;
    }
    void expect_device(const Logical& m) {   // the filter is d's, and holds m
        CHECK(f.where == Where::Device && f.latest == Source::Filter && f.n == 0 && !f.in_mailbox());
        CHECK(std::memcmp(f.d->x, m.x, sizeof(m.x)) == 0 && std::memcmp(f.d->P, m.P, sizeof(m.P)) == 0);
        CHECK(f.scan_x(kf.get()) == f.d->x);                        // lv_map_add_scan transforms with the observed state
        const ResidentFilter::Prior pr = f.prior();                 // a following lv_correct finds its prior in d
        CHECK(pr.host == nullptr && pr.dev == f.d && pr.dev_in_kf == 0);
        lv_state x;
        double P[NS * NS];
        const size_t t = mark();
        CHECK(f.get(s, kf.get(), &io, 0, true, &resyncs, &x, P) == LV_OK);   // ... and lv_filter_get copies it (not the mailbox)
        CHECK((calls(t) == Calls{"hipMemcpyAsync", "hipStreamSynchronize"}));
        CHECK(std::memcmp(&x, m.x, sizeof(m.x)) == 0 && std::memcmp(P, m.P, sizeof(m.P)) == 0);
    }
};

// ---- scenarios: one per place the filter can be
void from_host() {
    Ctx c;
    Logical m = seed(1.0);
    CHECK(c.set(m) == LV_OK);
    const lv_observation o[2] = {good(LV_OBS_POSITION), good(LV_OBS_VELOCITY_BODY, 1.5)};
    const size_t t = mark();
    CHECK(c.observe(o, 2) == LV_OK);
    CHECK(calls(t) == UPLOAD + Calls{"launch_observe"});
    CHECK(g_observes.size() == 1 && g_observes[0].n == 2 && g_observes[0].f == c.f.d);
    toy_observe(m.x, m.P, o[0]);
    toy_observe(m.x, m.P, o[1]);
    CHECK(c.res[0].rows == 3 && c.res[1].rows == 3);
    c.expect_device(m);
}
void from_device_queued() {
    Ctx c;
    Logical m = seed(2.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.predict(0.01) == LV_OK);
    CHECK(c.f.flush(c.s, c.kf.get()) == LV_OK);   // (the filter is on the device, nothing queued)
    model_predict(m, 0.01);
    g_predict_n.clear();
    size_t t = mark();
    for (int i = 0; i < 3; ++i) { CHECK(c.predict(0.002 * (i + 1)) == LV_OK); model_predict(m, 0.002 * (i + 1)); }
    CHECK(calls(t).empty());
    const lv_observation o = good(LV_OBS_VELOCITY_WORLD);
    CHECK(c.observe(&o, 1) == LV_OK);
    CHECK((calls(t) == Calls{"launch_predict", "launch_observe"}));
    CHECK(g_predict_n == std::vector<int>{3} && !g_predict_from_kf.back());
    toy_observe(m.x, m.P, o);
    c.expect_device(m);
}
void from_kf() {
    Ctx c;
    Logical m = seed(3.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.correct(&m) == LV_OK);
    CHECK(c.f.where == Where::Kf);
    const lv_observation o = good(LV_OBS_ATTITUDE);
    const size_t t = mark();
    CHECK(c.observe(&o, 1) == LV_OK);
    CHECK((calls(t) == Calls{"launch_kf_to_filter", "launch_observe"}));
    toy_observe(m.x, m.P, o);
    c.expect_device(m);
}
void from_kf_queued() {   // predictions queued behind a correct read kf; the observation follows them in d
    Ctx c;
    Logical m = seed(3.5);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.correct(&m) == LV_OK);
    CHECK(c.predict(0.004) == LV_OK);
    model_predict(m, 0.004);
    const lv_observation o = good(LV_OBS_POSITION);
    const size_t t = mark();
    CHECK(c.observe(&o, 1) == LV_OK);
    CHECK((calls(t) == Calls{"launch_predict", "launch_observe"}));
    CHECK(g_predict_from_kf.back());
    toy_observe(m.x, m.P, o);
    c.expect_device(m);
}
void from_copied() {
    Ctx c;
    Logical m = seed(4.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.correct(&m) == LV_OK);
    CHECK(c.f.materialise(c.s, c.kf.get()) == LV_OK);
    CHECK(c.f.where == Where::Copied && c.f.in_mailbox());
    const lv_observation o = good(LV_OBS_POSITION);
    const size_t t = mark();
    CHECK(c.observe(&o, 1) == LV_OK);
    CHECK(calls(t) == Calls{"launch_observe"});
    toy_observe(m.x, m.P, o);
    c.expect_device(m);
}
void unset() {
    Ctx c;
    const lv_observation o = good(LV_OBS_POSITION);
    size_t t = mark();
    CHECK(c.observe(&o, 1) == LV_ESTATE && std::strstr(g_err, "lv_observe before lv_filter_set"));
    CHECK(calls(t).empty() && g_observes.empty() && c.f.where == Where::Unset);
    Logical m = seed(5.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.correct(&m) == LV_OK);
    c.f.drop();   // (a failed correct or exchange)
    t = mark();
    CHECK(c.observe(&o, 1) == LV_ESTATE);
    CHECK(calls(t).empty() && g_observes.empty());
}
void observe_predict_observe() {
    Ctx c;
    Logical m = seed(6.0);
    CHECK(c.set(m) == LV_OK);
    const lv_observation a = good(LV_OBS_POSITION), b = good(LV_OBS_VELOCITY_BODY, -0.75);
    size_t t = mark();
    CHECK(c.observe(&a, 1) == LV_OK);
    toy_observe(m.x, m.P, a);
    CHECK(c.predict(0.005) == LV_OK);
    model_predict(m, 0.005);
    CHECK(calls(t) == UPLOAD + Calls{"launch_observe"});   // (the prediction waits in the queue)
    CHECK(c.observe(&b, 1) == LV_OK);
    toy_observe(m.x, m.P, b);
    CHECK(calls(t) == UPLOAD + Calls{"launch_observe", "launch_predict", "launch_observe"});
    c.expect_device(m);
    // ... and with one launch per prediction the same sequence of launches, the prediction's at its own call
    Ctx e;
    Logical k = seed(6.0);
    e.f.batch_predict = false;
    CHECK(e.set(k) == LV_OK);
    t = mark();
    CHECK(e.observe(&a, 1) == LV_OK && e.predict(0.005) == LV_OK);
    CHECK(calls(t) == UPLOAD + Calls{"launch_observe", "launch_predict"});
    CHECK(e.observe(&b, 1) == LV_OK);
    CHECK(calls(t) == UPLOAD + Calls{"launch_observe", "launch_predict", "launch_observe"});
    e.expect_device(m);
}
void then_correct() {   // the LiDAR update after an observation starts from d, and its posterior is the mailbox's again
    Ctx c;
    Logical m = seed(7.0);
    CHECK(c.set(m) == LV_OK);
    const lv_observation o = good(LV_OBS_POSITION);
    CHECK(c.observe(&o, 1) == LV_OK);
    toy_observe(m.x, m.P, o);
    const size_t t = mark();
    CHECK(c.correct(&m) == LV_OK);
    CHECK(calls(t) == Calls{"update"});
    CHECK(c.f.where == Where::Kf && std::memcmp(c.kf->x, m.x, sizeof(m.x)) == 0 && std::memcmp(c.kf->P_post, m.P, sizeof(m.P)) == 0);
}
void rejections() {
    struct Bad { const char* what; void (*spoil)(lv_observation&); int kind; };
    const Bad bad[] = {
        {"unknown kind", [](lv_observation& o) { o.kind = 0; }, LV_OBS_POSITION},
        {"unknown kind", [](lv_observation& o) { o.kind = 5; }, LV_OBS_POSITION},
        {"unknown kind", [](lv_observation& o) { o.kind = -1; }, LV_OBS_POSITION},
        {"mask", [](lv_observation& o) { o.mask = 0; }, LV_OBS_VELOCITY_WORLD},
        {"mask", [](lv_observation& o) { o.mask = 8; }, LV_OBS_VELOCITY_WORLD},
        {"mask", [](lv_observation& o) { o.mask = -3; }, LV_OBS_VELOCITY_WORLD},
        {"non-finite z", [](lv_observation& o) { o.z[1] = std::numeric_limits<double>::quiet_NaN(); }, LV_OBS_POSITION},
        {"non-finite z", [](lv_observation& o) { o.z[2] = std::numeric_limits<double>::infinity(); }, LV_OBS_VELOCITY_BODY},
        {"non-finite z", [](lv_observation& o) { o.z[3] = std::numeric_limits<double>::quiet_NaN(); }, LV_OBS_ATTITUDE},
        {"non-finite R", [](lv_observation& o) { o.R[5] = std::numeric_limits<double>::quiet_NaN(); }, LV_OBS_POSITION},
        {"non-finite R", [](lv_observation& o) { o.R[0] = -std::numeric_limits<double>::infinity(); }, LV_OBS_ATTITUDE},
        {"non-finite lever", [](lv_observation& o) { o.lever[2] = std::numeric_limits<double>::quiet_NaN(); }, LV_OBS_POSITION},
        {"non-finite lever", [](lv_observation& o) { o.lever[0] = std::numeric_limits<double>::infinity(); }, LV_OBS_VELOCITY_WORLD},
        {"lever arm goes with LV_OBS_POSITION", [](lv_observation& o) { o.lever[1] = 0.1; }, LV_OBS_VELOCITY_WORLD},
        {"lever arm goes with LV_OBS_POSITION", [](lv_observation& o) { o.lever[0] = -0.1; }, LV_OBS_VELOCITY_BODY},
        {"lever arm goes with LV_OBS_POSITION", [](lv_observation& o) { o.lever[2] = 1e-300; }, LV_OBS_ATTITUDE},
        {"gate", [](lv_observation& o) { o.gate = -1e-9; }, LV_OBS_POSITION},
        {"gate", [](lv_observation& o) { o.gate = std::numeric_limits<double>::quiet_NaN(); }, LV_OBS_POSITION},
        {"gate", [](lv_observation& o) { o.gate = std::numeric_limits<double>::infinity(); }, LV_OBS_POSITION},
        {"unit quaternion", [](lv_observation& o) { o.z[3] = 1.0 + 2e-6; }, LV_OBS_ATTITUDE},
        {"unit quaternion", [](lv_observation& o) { o.z[3] = 1.0 - 2e-6; }, LV_OBS_ATTITUDE},
        {"unit quaternion", [](lv_observation& o) { o.z[3] = 0.0; }, LV_OBS_ATTITUDE},
    };
    Ctx c;
    const Logical m = seed(8.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.predict(0.01) == LV_OK);   // (one queued prediction: a refusal must leave it queued)
    const size_t t = mark();
    for (const Bad& b : bad) {
        lv_observation o[3] = {good(LV_OBS_POSITION), good(b.kind), good(LV_OBS_VELOCITY_WORLD)};
        CHECK(observations_ok(o, 3) == LV_OK);
        b.spoil(o[1]);
        g_err[0] = 0;
        CHECK(c.observe(o, 3) == LV_EINVAL);
        CHECK(std::strstr(g_err, b.what) && std::strstr(g_err, "observation 1") && std::strstr(g_err, "lv_observe: ") == g_err);
        CHECK(observation_ok(o[1], 1) == LV_EINVAL && observations_ok(o, 1) == LV_OK);
    }
    lv_observation nine[LV_OBSERVE_BATCH + 1];
    for (auto& o : nine) o = good(LV_OBS_POSITION);
    CHECK(c.observe(nine, 0) == LV_EINVAL && std::strstr(g_err, "0 observations"));
    CHECK(c.observe(nine, LV_OBSERVE_BATCH + 1) == LV_EINVAL && std::strstr(g_err, "9 observations"));
    CHECK(c.observe(nullptr, 1) == LV_EINVAL && std::strstr(g_err, "null observations"));
    // nothing enqueued, the filter where it was, the prediction still queued
    CHECK(calls(t).empty() && g_observes.empty() && c.f.where == Where::Host && c.f.n == 1);
    // what is allowed: the bound of the quaternion norm, a zero gate, R = 0, a lever with POSITION, z[3] ignored outside ATTITUDE
    lv_observation q = good(LV_OBS_ATTITUDE);
    q.z[3] = 1.0 + 0.9e-6;
    CHECK(observation_ok(q, 0) == LV_OK);
    lv_observation p = good(LV_OBS_POSITION);
    p.lever[0] = 0.3; p.gate = 0.0; p.z[3] = std::numeric_limits<double>::quiet_NaN();
    for (double& r : p.R) r = 0.0;
    CHECK(observation_ok(p, 0) == LV_OK);
    CHECK(c.observe(nine, LV_OBSERVE_BATCH) == LV_OK && g_observes.size() == 1 && g_observes[0].n == LV_OBSERVE_BATCH);
}
void defaults() {
    for (int kind = 1; kind <= 4; ++kind) {
        lv_observation o;
        std::memset(&o, 0xff, sizeof(o));
        default_observation(&o, kind);
        CHECK(o.kind == kind && o.mask == 7 && o.gate == 0.0);
        for (int i = 0; i < 3; ++i) CHECK(o.z[i] == 0.0 && o.lever[i] == 0.0);
        CHECK(o.z[3] == (kind == LV_OBS_ATTITUDE ? 1.0 : 0.0));
        for (int i = 0; i < 9; ++i) CHECK(o.R[i] == (i % 4 == 0 ? 1.0 : 0.0));
        CHECK(observation_ok(o, 0) == LV_OK);
    }
    default_observation(nullptr, 1);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: observe_emu <scenario>\n"); return 2; }
    for (int k = 0; k < 144; ++k) g_Q[k] = 1e-3 * (k + 1);
    const std::string s = argv[1];
    if (s == "from_host") from_host();
    else if (s == "from_device_queued") from_device_queued();
    else if (s == "from_kf") from_kf();
    else if (s == "from_kf_queued") from_kf_queued();
    else if (s == "from_copied") from_copied();
    else if (s == "unset") unset();
    else if (s == "observe_predict_observe") observe_predict_observe();
    else if (s == "then_correct") then_correct();
    else if (s == "rejections") rejections();
    else if (s == "defaults") defaults();
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees && st.events_created == st.events_destroyed);
    printf("ok %s\n", s.c_str());
    return 0;
}
