// lv_knobs.hpp — the run-time knobs of a context, once: lv_set_option's name, the environment variable lv_create reads, how an int
// becomes the value, where it lands.  A row without a name is fixed at creation (it sizes buffers).  Ctx is lv_ctx (lv_api.hip);
// tests/emu/update_emu.cpp walks the table over a stand-in with members of the same names.
#pragma once
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "lv_common.hpp"

namespace lv {

enum class KnobKind { Bool /* v != 0 */, Count /* v > 0 ? v : 0 */, Int /* as given */ };

template <class Ctx>
struct Knobs {
    struct Knob {
        const char *option, *env;    // lv_set_option's name / the environment variable, or nullptr
        KnobKind kind;
        int (*set)(Ctx& c, int v);   // v: already of its kind
    };
    static const std::initializer_list<Knob>& table() {
#define LV_KNOB(option, env, kind, ...) {option, env, KnobKind::kind, [](Ctx& c, int v) -> int { __VA_ARGS__; return LV_OK; }}
        static const std::initializer_list<Knob> rows = {
            // ---- the update's routes (lv_update.hpp)
            LV_KNOB("fused_pass", "LV_FUSED_PASS", Bool, c.upd.fused_pass = v),   // off: the three-kernel pass also where pass_kernel applies
            LV_KNOB("fused_ext", "LV_FUSED_EXT", Bool, c.upd.fused_ext = v),       // off: the three-kernel pass with estimate_extrinsics
            LV_KNOB("fast_fit", nullptr, Bool, c.upd.fast_fit = v),   // the approximate plane fit of pass_kernel (v_rcp / v_sqrt + Newton; NOT bit-exact)
            LV_KNOB("multi_overlap", "LV_MULTI_OVERLAP", Bool, c.upd.multi_overlap = v),   // A/B: 0 = every round's fits between two barriers
            LV_KNOB("fused_multi_round", "LV_FUSED_MULTI", Bool, c.upd.fused_multi_round = v),   // tri-state: 1 any number of rounds, 0 up to three (-1, the default, is nobody's to set)
            LV_KNOB("keeper_by_cost", "LV_KEEPER_BY_COST", Bool, c.upd.keeper_by_cost = v),   // off: the last searching workgroup always keeps the books (A/B)
            LV_KNOB("tile_lpt", "LV_TILE_LPT", Bool, c.upd.tile_lpt = v),                     // off: the search tiles in plain order, not farthest-first (A/B)
            LV_KNOB("spin_wait", "LV_SPIN_WAIT", Bool, c.upd.spin_wait = v),                  // off: the end synchronises the stream without polling the mailbox
            LV_KNOB(nullptr, "LV_BLOCKS_PER_CU", Count, c.upd.blocks_per_cu = v),   // fit blocks per CU (0: the default, four)
            LV_KNOB(nullptr, "LV_PASS_WG", Count, c.upd.pass_max_wg = v),           // pass_kernel's workgroup limit (0: one per CU)
            LV_KNOB(nullptr, "LV_PASS_CLK", Bool, c.upd.pass_clk = v),              // phase stamps of pass_kernel (lv_get_pass_clocks)
            // ---- the exchange and the filter
            LV_KNOB("comm_fused", "LV_COMM_FUSED", Bool, c.ranks.fused = v),
            LV_KNOB("mail_filter", "LV_MAIL_FILTER", Bool, c.filter.mail_filter = v),
            LV_KNOB("batch_predict", "LV_BATCH_PREDICT", Bool,   // (the queue, filled under the other rule, is flushed first; lv_create: it is empty, kf not looked at)
                    if (int rp = c.filter.flush(c.stream, c.upd.d_kf)) return rp; c.filter.batch_predict = v),
            // ---- the background re-linearisation (lv_rebuild.hpp)
            LV_KNOB("async_relinearise", "LV_ASYNC_RELINEARISE", Bool, c.rebuild.opt.async = v),
            LV_KNOB("async_relinearise_min", nullptr, Count, c.rebuild.opt.async_min = (size_t)v),
            LV_KNOB("async_relinearise_pause_us", "LV_RELIN_PAUSE_US", Count, c.rebuild.opt.pause_us = (uint32_t)v),
            LV_KNOB("async_relinearise_slice_wgs", "LV_RELIN_SLICE_WGS", Count, c.rebuild.opt.slice_wgs = (uint32_t)v),   // 0: whole grids
            LV_KNOB("async_relinearise_journal_max", nullptr, Count, c.rebuild.opt.journal_max = v ? (size_t)v : 1),
            LV_KNOB("async_relinearise_test_delay_ms", nullptr, Int, c.rebuild.opt.test_delay_ms = v),
            LV_KNOB("async_relinearise_test_race", nullptr, Bool, c.rebuild.opt.test_race = v),
            // ---- the map, the scan, the batch
            LV_KNOB("overlap_insert", "LV_OVERLAP_INSERT", Bool, c.overlap_insert = v),
            LV_KNOB("merged_insert", "LV_MERGED_INSERT", Bool, c.map.merged_back = v),
            LV_KNOB("sweep_evict", "LV_SWEEP_EVICT", Bool, c.map.sweep_evict = v),
            LV_KNOB("small_insert", "LV_SMALL_INSERT", Bool, c.map.small_front = v),
            LV_KNOB("survivor_list", "LV_SURV_LIST", Bool, c.map.surv_list = v),
            LV_KNOB("small_window", "LV_SMALL_WINDOW", Bool, c.scan.small_enabled = v),
            LV_KNOB("large_window", "LV_LARGE_WINDOW", Bool, c.scan.large_enabled = v),
            LV_KNOB("batch_chunk_hypotheses", nullptr, Count, c.batch.chunk_hyp = v),
        };
#undef LV_KNOB
        return rows;
    }
    static int of_kind(KnobKind k, int v) { return k == KnobKind::Bool ? (v != 0) : k == KnobKind::Count ? (v > 0 ? v : 0) : v; }
    // lv_set_option
    static int set_option(Ctx& c, const char* name, int value) {
        for (const Knob& k : table())
            if (k.option && !std::strcmp(name, k.option)) return k.set(c, of_kind(k.kind, value));
        set_error("lv_set_option: unknown option '%s'", name);
        return LV_EINVAL;
    }
    // lv_create: every variable that is set
    static int read_environment(Ctx& c) {
        for (const Knob& k : table())
            if (const char* e = k.env ? getenv(k.env) : nullptr)
                if (int rc = k.set(c, of_kind(k.kind, atoi(e)))) return rc;
        return LV_OK;
    }
};

}  // namespace lv
