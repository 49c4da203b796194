// tests/emu/filter_emu.cpp — HOST test of the resident filter (limo-velo_amd/csrc/lv_filter.hpp).
// TEST INFRASTRUCTURE ONLY: built by tests/test_filter_host.py into tests/emu/_build/ (once plain, once with AddressSanitizer +
// UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own ResidentFilter against the stand-in hip_runtime.h
// next to this file, with fake launches: launch_predict applies a toy step to whichever buffer it is told to read (so a wrong
// source gives a wrong value), launch_kf_to_filter copies, and a fake update writes a posterior derived from its prior into kf
// and the mailbox with a correct seqcheck.  The drivers below call the class exactly as the update driver (lv_update.hpp) and the entry points of lv_api.hip do; the
// HIP stand-in logs every call, so a scenario asserts what each step enqueued.  Usage: filter_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <memory>
#include <random>

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

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            std::_Exit(1);                                                              \
        }                                                                               \
    } while (0)

namespace {

// ---- toy arithmetic: deterministic, element-wise (in place is fine), different for every input
void toy_step(double* x, double* P, const double* Q, const double* st) {
    for (int j = 0; j < NX; ++j) x[j] = x[j] * 0.75 + st[0] * (j + 1) + st[1 + j % 6] * 0.125;
    for (int k = 0; k < NS * NS; ++k) P[k] = P[k] * 0.5 + Q[k % 144] * st[0];
}
void toy_update(double* x, double* P) {
    for (int j = 0; j < NX; ++j) x[j] = x[j] * 0.5 + 1.0 / (j + 1);
    for (int k = 0; k < NS * NS; ++k) P[k] = P[k] * 0.25 + 0.01;
}

struct PredictLaunch { bool from_kf; int n; };
std::vector<PredictLaunch> g_predicts;
std::function<void(const char*)> g_hook;   // runs at every logged HIP call (the mailbox scenarios complete a late arrival there)

}  // namespace

// ---- the fakes of lv_predict.hip
int lv::launch_predict(hipStream_t s, FilterDev* f, const KfDev* src, const double* Q, int n, const double (*steps)[7]) {
    emu_hip::call("launch_predict", s);
    g_predicts.push_back({src != nullptr, n});
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

namespace {

std::vector<std::string> calls(size_t from) {
    std::vector<std::string> v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i) v.push_back(log[i].call);
    return v;
}
size_t mark() { return emu_hip::state().log.size(); }
using Calls = std::vector<std::string>;

struct Logical {   // the reference model: the filter as the caller sees it
    bool set = false;
    double x[NX], P[NS * NS];
};

// a context as lv_api.hip and its update driver hold it: the filter, kf, the mailbox, the stream and the update number
struct Ctx {
    ResidentFilter f;
    std::unique_ptr<KfDev> kf{new KfDev()};
    KfHostIO io{};
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    int seq = 0;
    long resyncs = 0;
    Ctx() { CHECK(f.alloc() == LV_OK); }
    ~Ctx() { f.release(); }

    // the fake passes of an update: the posterior of what kf holds, in kf and (checksummed) in the mailbox
    void passes() {
        emu_hip::call("update", s);
        toy_update(kf->x, kf->P_post);
        std::memcpy(io.x, kf->x, sizeof(io.x));
        std::memcpy(io.P_post, kf->P_post, sizeof(io.P_post));
        io.passes = 3;
        uint32_t chk = 0;
        for (int i = 0; i < NS * NS; ++i) chk ^= mailbox_mix(io.P_post[i], (uint32_t)i);
        for (int i = 0; i < NX; ++i) chk ^= mailbox_mix(io.x[i], 1000u + (uint32_t)i);
        chk ^= mailbox_mix((double)io.passes, 2000u);
        if (chk == MAILBOX_UNCHECKED) chk = 0u;
        io.seqcheck = ((unsigned long long)chk << 32) | (uint32_t)seq;
    }
    // begin_device: the filter's part, then the begin (deferred or kf_begin_kernel) installs the prior in kf
    int begin(const double* x_host, const ResidentFilter::Prior& pr = {}) {
        if (int r = f.begin_update(s, kf.get(), pr.dev != nullptr)) return r;
        if (x_host) {
            std::memcpy(kf->x, x_host, sizeof(kf->x));
            std::memcpy(kf->P_post, x_host + NX, sizeof(kf->P_post));
        } else if (pr.dev && !pr.dev_in_kf) {
            std::memcpy(kf->x, pr.dev->x, sizeof(kf->x));
            std::memcpy(kf->P_post, pr.dev->P, sizeof(kf->P_post));
        }
        return LV_OK;
    }
    // ---- the entry points (a map is always present; a peer exchange never is, except through drop())
    int set(const Logical& m) { return f.set(reinterpret_cast<const lv_state*>(m.x), m.P); }
    int predict(double dt, const double* Q, const double* acc, const double* gyro) { return f.predict(s, kf.get(), dt, Q, acc, gyro); }
    int correct(bool fail = false) {
        if (int r = f.need("lv_correct")) return r;
        if (int r = f.flush(s, kf.get())) return r;
        f.latest = Source::Filter;
        seq = (seq + 1) & 0x3fffffff;
        const ResidentFilter::Prior pr = f.prior();
        if (int r = begin(pr.host, pr)) return r;
        if (fail) { f.drop(); return LV_EHIP; }
        passes();
        f.correct_done();
        return LV_OK;
    }
    int get(lv_state* x, double* P) { return f.get(s, kf.get(), &io, seq, true, &resyncs, x, P); }
    // lv_update with a map (by value: x_in followed by P_in) / lv_iterate (kf->x := x, no mailbox) / lv_update without a map
    int update_by_value(const double* xP) {
        f.latest = Source::ByValue;
        seq = (seq + 1) & 0x3fffffff;
        if (int r = begin(xP)) return r;
        passes();
        return LV_OK;
    }
    int iterate(const double* xP) {
        seq = (seq + 1) & 0x3fffffff;
        return begin(xP);
    }
    int update_no_map(const double* x) {
        f.latest = Source::ByValue;
        if (int r = f.flush(s, kf.get())) return r;
        if (int r = f.materialise(s, kf.get())) return r;
        CHECK(hipStreamSynchronize(s) == hipSuccess);
        CHECK(hipMemcpyAsync(kf->x, x, sizeof(double) * NX, hipMemcpyHostToDevice, s) == hipSuccess);
        return LV_OK;
    }
    int synchronize() { return f.flush(s, kf.get()); }   // (lv_synchronize, lv_set_stream)
    const double* map_add() {   // the state lv_map_add_scan transforms the scan with
        CHECK(f.flush(s, kf.get()) == LV_OK);
        CHECK(f.upload(s) == LV_OK);
        return f.scan_x(kf.get());
    }
};

double g_Q[2][144];
const double g_acc[3] = {0.1, -0.2, 9.81}, g_gyro[3] = {0.01, 0.02, -0.03};

Logical seed(double v) {
    Logical m;
    m.set = true;
    for (int j = 0; j < NX; ++j) m.x[j] = v + j;
    for (int k = 0; k < NS * NS; ++k) m.P[k] = (k % (NS + 1) == 0) ? v : 0.001 * k;
    return m;
}
void model_predict(Logical& m, double dt, const double* Q) {
    const double st[7] = {dt, g_acc[0], g_acc[1], g_acc[2], g_gyro[0], g_gyro[1], g_gyro[2]};
    toy_step(m.x, m.P, Q, st);
}
void model_correct(Logical& m) { toy_update(m.x, m.P); }
void expect_get(Ctx& c, const Logical& m) {
    lv_state x;
    double P[NS * NS];
    CHECK(c.get(&x, P) == LV_OK);
    CHECK(std::memcmp(&x, m.x, sizeof(m.x)) == 0);
    CHECK(std::memcmp(P, m.P, sizeof(m.P)) == 0);
}
int count(const Calls& v, const char* name) { return (int)std::count(v.begin(), v.end(), std::string(name)); }

// ---- scenarios
void cycle() {
    Ctx c;
    Logical m = seed(1.0);
    for (int it = 0; it < 3; ++it) {
        size_t t = mark();
        CHECK(c.set(m) == LV_OK);
        CHECK(calls(t).empty());
        t = mark();
        CHECK(c.correct() == LV_OK);
        CHECK(calls(t) == Calls{"update"});   // (the filter's side of the correct: nothing)
        model_correct(m);
        t = mark();
        expect_get(c, m);
        CHECK(calls(t).empty());              // (the mailbox: no copy, no synchronise)
        CHECK(c.f.where == Where::Kf);
    }
    CHECK(c.resyncs == 0);
}
void set_get() {
    Ctx c;
    const Logical m = seed(2.0);
    const size_t t = mark();
    CHECK(c.set(m) == LV_OK);
    expect_get(c, m);
    CHECK(calls(t).empty());
}
void set_predict3_get() {
    Ctx c;
    Logical m = seed(3.0);
    CHECK(c.set(m) == LV_OK);
    const size_t t = mark();
    for (int i = 0; i < 3; ++i) {
        CHECK(c.predict(0.01 * (i + 1), g_Q[0], g_acc, g_gyro) == LV_OK);
        model_predict(m, 0.01 * (i + 1), g_Q[0]);
    }
    CHECK(calls(t).empty());   // (queued)
    expect_get(c, m);
    CHECK((calls(t) == Calls{"hipMemcpyAsync", "hipEventCreateWithFlags", "hipEventRecord", "launch_predict", "hipMemcpyAsync",
                             "hipStreamSynchronize"}));
    CHECK(g_predicts.size() == 1 && g_predicts[0].n == 3 && !g_predicts[0].from_kf);
}
void queue_splits() {
    Ctx c;
    Logical m = seed(4.0);
    CHECK(c.set(m) == LV_OK);
    for (int i = 0; i < 2; ++i) { CHECK(c.predict(0.01, g_Q[0], g_acc, g_gyro) == LV_OK); model_predict(m, 0.01, g_Q[0]); }
    CHECK(g_predicts.empty());
    CHECK(c.predict(0.01, g_Q[1], g_acc, g_gyro) == LV_OK);   // a new Q: the two queued steps launch
    model_predict(m, 0.01, g_Q[1]);
    CHECK(g_predicts.size() == 1 && g_predicts[0].n == 2);
    CHECK(c.synchronize() == LV_OK);
    CHECK(g_predicts.size() == 2 && g_predicts[1].n == 1);
    g_predicts.clear();
    for (int i = 0; i < 9; ++i) { CHECK(c.predict(0.002, g_Q[0], g_acc, g_gyro) == LV_OK); model_predict(m, 0.002, g_Q[0]); }
    expect_get(c, m);
    CHECK(g_predicts.size() == 2 && g_predicts[0].n == PREDICT_BATCH && g_predicts[1].n == 1);
    g_predicts.clear();
    CHECK(c.synchronize() == LV_OK);
    c.f.batch_predict = false;
    for (int i = 0; i < 3; ++i) {
        CHECK(c.predict(0.003, g_Q[0], g_acc, g_gyro) == LV_OK);
        model_predict(m, 0.003, g_Q[0]);
        CHECK((int)g_predicts.size() == i + 1 && g_predicts[i].n == 1);
    }
    expect_get(c, m);
}
void correct_predict_correct() {
    Ctx c;
    Logical m = seed(5.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.correct() == LV_OK);
    model_correct(m);
    size_t t = mark();
    CHECK(c.predict(0.01, g_Q[0], g_acc, g_gyro) == LV_OK);
    model_predict(m, 0.01, g_Q[0]);
    expect_get(c, m);   // (not from the mailbox: the prediction has moved the filter on)
    CHECK((calls(t) == Calls{"launch_predict", "hipMemcpyAsync", "hipStreamSynchronize"}));
    CHECK(g_predicts.size() == 1 && g_predicts[0].from_kf);
    CHECK(c.correct() == LV_OK);
    model_correct(m);
    CHECK(c.predict(0.02, g_Q[0], g_acc, g_gyro) == LV_OK);
    model_predict(m, 0.02, g_Q[0]);
    t = mark();
    CHECK(c.correct() == LV_OK);
    model_correct(m);
    CHECK((calls(t) == Calls{"launch_predict", "update"}));
    CHECK(g_predicts.size() == 2 && g_predicts[1].from_kf);
    expect_get(c, m);
    CHECK(count(calls(0), "launch_kf_to_filter") == 0);
}
void correct_update_predict_get() {
    Ctx c;
    Logical m = seed(6.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.correct() == LV_OK);
    model_correct(m);
    const Logical other = seed(60.0);
    size_t t = mark();
    CHECK(c.update_by_value(other.x) == LV_OK);   // (other.x is followed by other.P: the layout of x_in / P_in)
    CHECK((calls(t) == Calls{"launch_kf_to_filter", "update"}));
    CHECK(c.f.where == Where::Device);
    CHECK(c.predict(0.01, g_Q[0], g_acc, g_gyro) == LV_OK);
    model_predict(m, 0.01, g_Q[0]);
    expect_get(c, m);
    CHECK(g_predicts.size() == 1 && !g_predicts[0].from_kf);
}
void set_predict_set() {
    Ctx c;
    Logical m = seed(7.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.predict(0.01, g_Q[0], g_acc, g_gyro) == LV_OK);
    CHECK(c.synchronize() == LV_OK);   // (the upload out of h is enqueued here)
    m = seed(8.0);
    size_t t = mark();
    CHECK(c.set(m) == LV_OK);
    CHECK(calls(t) == Calls{"hipEventSynchronize"});
    t = mark();
    CHECK(c.set(m) == LV_OK);          // (nothing uploaded since)
    CHECK(calls(t).empty());
    expect_get(c, m);
}
void mailbox(int kind) {   // 0: checksum mismatch, 1: MAILBOX_UNCHECKED, 2: the fault bit
    Ctx c;
    Logical m = seed(9.0);
    CHECK(c.set(m) == LV_OK);
    CHECK(c.correct() == LV_OK);
    model_correct(m);
    const double good = c.io.x[0];
    if (kind == 0) {
        c.io.x[0] = -1.0;   // a result that has not arrived when the word has: it does once the stream is synchronised
        g_hook = [&](const char* call) { if (!std::strcmp(call, "hipStreamSynchronize")) c.io.x[0] = good; };
    } else if (kind == 1) {
        c.io.seqcheck = ((unsigned long long)MAILBOX_UNCHECKED << 32) | (uint32_t)c.seq;
    } else {
        c.io.fallback_queries = (int)KF_FAULT_BIT | 7;
    }
    const size_t t = mark();
    if (kind == 2) {
        lv_state x;
        CHECK(c.get(&x, nullptr) == ((int)KF_FAULT_BIT | 7));
        return;
    }
    expect_get(c, m);
    g_hook = nullptr;
    CHECK(calls(t) == Calls{"hipStreamSynchronize"});
    CHECK(c.resyncs == (kind == 0 ? 1 : 0));
}
void failures() {
    for (int how = 0; how < 2; ++how) {   // a failed correct, a failed peer exchange
        Ctx c;
        Logical m = seed(10.0);
        CHECK(c.set(m) == LV_OK);
        if (how == 0) {
            CHECK(c.correct(true) == LV_EHIP);
        } else {
            CHECK(c.correct() == LV_OK);
            c.f.drop();
        }
        CHECK(c.f.where == Where::Unset);
        lv_state x;
        CHECK(c.get(&x, nullptr) == LV_ESTATE && std::strstr(g_err, "lv_filter_get before lv_filter_set"));
        CHECK(c.predict(0.01, g_Q[0], g_acc, g_gyro) == LV_ESTATE && std::strstr(g_err, "lv_predict before lv_filter_set"));
        CHECK(c.correct() == LV_ESTATE && std::strstr(g_err, "lv_correct before lv_filter_set"));
        CHECK(c.map_add() == c.kf->x);
        CHECK(c.set(m) == LV_OK);   // (re-seeded)
        expect_get(c, m);
    }
}
void map_add_source() {
    Ctx c;
    CHECK(c.map_add() == c.kf->x);   // (nothing set yet)
    Logical m = seed(11.0);
    CHECK(c.set(m) == LV_OK);
    size_t t = mark();
    const double* x = c.map_add();   // set: uploaded, d
    CHECK(x == c.f.d->x && std::memcmp(x, m.x, sizeof(m.x)) == 0);
    CHECK((calls(t) == Calls{"hipMemcpyAsync", "hipEventCreateWithFlags", "hipEventRecord"}));
    CHECK(c.correct() == LV_OK);
    model_correct(m);
    x = c.map_add();                 // correct: kf
    CHECK(x == c.kf->x && std::memcmp(x, m.x, sizeof(m.x)) == 0);
    CHECK(c.predict(0.01, g_Q[0], g_acc, g_gyro) == LV_OK);
    model_predict(m, 0.01, g_Q[0]);
    x = c.map_add();                 // predict: d
    CHECK(x == c.f.d->x && std::memcmp(x, m.x, sizeof(m.x)) == 0);
    const Logical other = seed(110.0);
    CHECK(c.update_by_value(other.x) == LV_OK);
    CHECK(c.map_add() == c.kf->x);   // update by value: kf, even after a correct
    CHECK(c.correct() == LV_OK);
    model_correct(m);
    CHECK(c.update_no_map(other.x) == LV_OK);
    x = c.map_add();                 // update without a map: the state the caller handed over
    CHECK(x == c.kf->x && std::memcmp(x, other.x, sizeof(other.x)) == 0);
    CHECK(c.f.where == Where::Copied);
    t = mark();
    expect_get(c, m);                // (the mailbox still holds the correct's posterior)
    CHECK(calls(t).empty());
    CHECK(c.set(m) == LV_OK);
    CHECK(c.iterate(other.x) == LV_OK);
    x = c.map_add();                 // lv_iterate does not mark its state: the filter's
    CHECK(x == c.f.d->x && std::memcmp(x, m.x, sizeof(m.x)) == 0);
}
// seeded random sequences against the reference model: every get equals it, every map add reads the latest state
void random_sequence(unsigned seed_value) {
    std::mt19937 rng(seed_value);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    Ctx c;
    Logical m;
    bool by_value = false;
    int gets = 0;
    for (int op = 0; op < 2000; ++op) {
        const int r = pick(100);
        const Logical other = seed(100.0 + op);
        if (r < 8 || (!m.set && r < 40)) {
            m = seed(op * 0.5);
            CHECK(c.set(m) == LV_OK);
            by_value = false;
        } else if (r < 40) {
            const double dt = 0.001 * (1 + pick(5));
            const double* Q = g_Q[pick(8) == 0];
            const int rc = c.predict(dt, Q, g_acc, g_gyro);
            CHECK(rc == (m.set ? LV_OK : LV_ESTATE));
            if (m.set) { model_predict(m, dt, Q); by_value = false; }
        } else if (r < 55) {
            const bool fail = pick(40) == 0;
            const int rc = c.correct(fail);
            CHECK(rc == (!m.set ? LV_ESTATE : fail ? LV_EHIP : LV_OK));
            if (m.set) by_value = false;
            if (m.set && fail) m.set = false;
            if (m.set) model_correct(m);
        } else if (r < 75) {
            lv_state x;
            double P[NS * NS];
            const int rc = c.get(&x, P);
            CHECK(rc == (m.set ? LV_OK : LV_ESTATE));
            if (m.set) {
                CHECK(std::memcmp(&x, m.x, sizeof(m.x)) == 0 && std::memcmp(P, m.P, sizeof(m.P)) == 0);
                ++gets;
            }
        } else if (r < 80) {
            CHECK(c.update_by_value(other.x) == LV_OK);
            by_value = true;
        } else if (r < 83) {
            CHECK(c.iterate(other.x) == LV_OK);
        } else if (r < 85) {
            CHECK(c.update_no_map(other.x) == LV_OK);
            by_value = true;
        } else if (r < 92) {
            const double* x = c.map_add();
            if (by_value || !m.set) CHECK(x == c.kf->x);
            else CHECK(std::memcmp(x, m.x, sizeof(m.x)) == 0);
        } else if (r < 94) {
            CHECK(c.synchronize() == LV_OK);
            c.f.batch_predict = pick(2);
        } else if (r < 96) {
            c.f.mail_filter = pick(2);
        } else if (r < 97) {
            c.f.drop();   // (a failed peer exchange)
            m.set = false;
        } else {
            CHECK(c.synchronize() == LV_OK);
        }
        CHECK((c.f.where == Where::Unset) == !m.set);
    }
    CHECK(gets > 100);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: filter_emu <scenario>\n"); return 2; }
    for (int k = 0; k < 144; ++k) { g_Q[0][k] = 1e-3 * (k + 1); g_Q[1][k] = 2e-3 * (144 - k); }
    emu_hip::state().fail = [](const char* call) { if (g_hook) g_hook(call); return false; };
    const std::string s = argv[1];
    if (s == "cycle") cycle();
    else if (s == "set_get") set_get();
    else if (s == "set_predict3_get") set_predict3_get();
    else if (s == "queue_splits") queue_splits();
    else if (s == "correct_predict_correct") correct_predict_correct();
    else if (s == "correct_update_predict_get") correct_update_predict_get();
    else if (s == "set_predict_set") set_predict_set();
    else if (s == "mailbox_resync") mailbox(0);
    else if (s == "mailbox_unchecked") mailbox(1);
    else if (s == "mailbox_fault") mailbox(2);
    else if (s == "failures") failures();
    else if (s == "map_add_source") map_add_source();
    else if (s.rfind("random", 0) == 0) random_sequence((unsigned)std::stoul(s.substr(6)));
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees && st.events_created == st.events_destroyed);
    printf("ok %s\n", s.c_str());
    return 0;
}
