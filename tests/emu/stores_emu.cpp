// tests/emu/stores_emu.cpp — the reserve paths of MapStore, ScanStore and CloudStore (limo-velo_amd/csrc/lv_stores.hpp) run on the
// host (TEST INFRASTRUCTURE ONLY; g++ through tests/emu/hip/hip_runtime.h).  argv[1] names a case; the case prints one
// "name value..." line per fact and tests/test_stores_host.py asserts the values.  The stand-in's call log, its mallocs / frees
// counters and its fail hook are the instruments; "device" memory is host memory here, so contents are written and read directly.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "lv_stores.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace lv {
static std::string g_error;
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
// the scratch sizes: any fixed formulas
int sort_pairs_scratch_u64(size_t n, int, size_t* bytes) { *bytes = 16 * n + 256; return LV_OK; }
int sort_pairs_scratch_u32(size_t n, int, size_t* bytes) { *bytes = 8 * n + 256; return LV_OK; }
int exclusive_sum_scratch(size_t n, size_t* bytes) { *bytes = n / 8 + 64; return LV_OK; }
int select_flagged_scratch(size_t n, size_t* bytes) { *bytes = n + 128; return LV_OK; }
void MapStore::refresh_view() { view.orig = d_orig; ++gen; }
}  // namespace lv

using namespace lv;

static emu_hip::State& st() { return emu_hip::state(); }
static hipStream_t g_s1 = nullptr;

struct Stores {
    MapStore map;
    ScanStore scan;
    CloudStore cloud;
};

// ---- what a store holds: every buffer as (name, cap, has a block), every field that speaks for buffers as a group -----------------
struct Item { std::string name; size_t cap; bool there; };
struct Group { std::string field; size_t value; std::vector<std::pair<Item, size_t>> members; };   // value * scale <= member.cap
template <class B> static Item item(const char* name, const B& b) { return {name, b.cap, b.p != nullptr}; }
#define IT(s, b) item(#b, (s).b)

static std::vector<Item> items(const Stores& S) {
    const MapStore& m = S.map;
    const ScanStore& s = S.scan;
    const CloudStore& c = S.cloud;
    std::vector<Item> v = {IT(m, d_orig), IT(m, d_orig2), IT(m, d_sorted), IT(m, d_keys), IT(m, d_keys_sorted), IT(m, d_idx), IT(m, d_idx_sorted),
                           IT(m, d_sort_tmp), IT(m, d_counts), IT(m, d_cellpos), IT(m, d_biglist), IT(m, d_gtable), IT(m, d_gext), IT(m, d_goff),
                           IT(m, d_broken), IT(m, d_regroup), IT(m, d_cell_slots), IT(m, d_bcount), IT(m, d_bcap), IT(m, d_boff), IT(m, d_flags),
                           IT(m, d_scan_tmp), IT(m, d_caux), IT(m, d_cell4), IT(m, d_cnt), IT(m, h_cnt), IT(m, d_new), IT(m, d_nkeys),
                           IT(m, d_nkeys_sorted), IT(m, d_nidx), IT(m, d_nidx_sorted), IT(m, d_nalive), IT(m, d_napos), IT(m, d_nsurv),
                           IT(m, d_nsflag), IT(m, d_nspos), IT(m, d_ntmp), IT(m, d_gcnt), IT(m, d_dead), IT(m, d_alive), IT(m, d_apos),
                           IT(m, d_ascan_tmp), IT(m, d_box), IT(m, d_box_next)};
    for (int l = 0; l < N_OCC; ++l) v.push_back(IT(m, d_tables[l]));
    for (int l = 0; l < BUCKET_LEVELS; ++l) {
        const Item per[] = {IT(m, d_btable[l]), IT(m, d_baux[l]), IT(m, d_bxyz[l]), IT(m, d_bidx[l]), IT(m, d_backpos[l]), IT(m, d_comp[l]),
                            IT(m, d_cstage[l]), IT(m, d_cnew[l]), IT(m, d_rank[l]), IT(m, d_gtab[l]), IT(m, d_prank[l]), IT(m, d_pslot[l]),
                            IT(m, d_gbase[l]), IT(m, d_gslot[l]), IT(m, d_gdst[l]), IT(m, d_reloc[l])};
        for (Item i : per) { i.name += std::to_string(l); v.push_back(i); }
    }
    const Item rest[] = {IT(s, d_raw), IT(s, d_sorted), IT(s, d_keys), IT(s, d_keys_sorted), IT(s, d_idx), IT(s, d_idx_sorted), IT(s, d_sort_tmp),
                         IT(s, d_tile_order), IT(s, d_in), IT(s, d_times), IT(s, d_desk), IT(s, d_states), IT(s, d_vkeys), IT(s, d_vkeys_sorted),
                         IT(s, d_vidx), IT(s, d_vidx_sorted), IT(s, d_heads), IT(s, d_hpos), IT(s, d_bounds), IT(s, d_vsort_tmp),
                         IT(s, d_vscan_tmp), IT(s, d_tail_clk), IT(c, d_buf), IT(c, d_rawmsg), IT(c, h_rawmsg), IT(c, h_rawmsg2),
                         IT(c, d_decoded), IT(c, d_kept), IT(c, d_keep), IT(c, d_keys), IT(c, d_keys_sorted), IT(c, d_ids), IT(c, d_ids_sorted),
                         IT(c, d_tmp), IT(c, d_count), IT(c, h_count)};
    for (const Item& i : rest) v.push_back(i);
    // the group fields themselves, as items of their own
    const std::pair<const char*, size_t> fields[] = {{"map.capacity", m.capacity}, {"map.batch_cap", m.batch_cap}, {"map.gtab_size", m.gtab_size},
                                                     {"map.reloc_cap", m.reloc_cap}, {"map.broken_cap", m.broken_cap}, {"map.comp_cap", m.comp_cap},
                                                     {"map.cstage_cap", m.cstage_cap}, {"map.box_size", m.box_size}, {"scan.capacity", s.capacity},
                                                     {"scan.raw_cap", s.raw_cap}, {"cloud.raw_cap", c.raw_cap}, {"cloud.msg_cap", c.msg_cap},
                                                     {"cloud.notes", (size_t)(c.notes.h != nullptr) + (size_t)(c.notes.d != nullptr)},
                                                     {"cloud.events", (size_t)(c.ev_stage[0] != nullptr) + (size_t)(c.ev_stage[1] != nullptr)}};
    for (const auto& f : fields) v.push_back({f.first, f.second, f.second != 0});
    return v;
}

static std::vector<Group> groups(const Stores& S) {
    const MapStore& m = S.map;
    const ScanStore& s = S.scan;
    const CloudStore& c = S.cloud;
    std::vector<Group> g;
    Group ids{"map.capacity", m.capacity, {{IT(m, d_orig), 1}, {IT(m, d_orig2), 1}, {IT(m, d_sorted), 1}, {IT(m, d_keys), 1}, {IT(m, d_keys_sorted), 1},
                                           {IT(m, d_idx), 1}, {IT(m, d_idx_sorted), 1}, {IT(m, d_sort_tmp), 0}, {IT(m, d_dead), 1}}};
    if (m.d_box_next.p) ids.members.push_back({IT(m, d_box_next), 1});   // (by id once they exist)
    if (m.d_cellpos.p) {
        ids.members.push_back({IT(m, d_cellpos), 1});
        for (int l = 0; l < BUCKET_LEVELS; ++l) ids.members.push_back({IT(m, d_backpos[l]), 27});
    }
    g.push_back(ids);
    Group batch{"map.batch_cap", m.batch_cap, {{IT(m, d_new), 1}, {IT(m, d_nkeys), 1}, {IT(m, d_nkeys_sorted), 1}, {IT(m, d_nidx), 1},
                                               {IT(m, d_nidx_sorted), 1}, {IT(m, d_nalive), 1}, {IT(m, d_napos), 1}, {IT(m, d_nsurv), 1},
                                               {IT(m, d_nsflag), 1}, {IT(m, d_nspos), 1}, {IT(m, d_ntmp), 0}, {IT(m, d_gcnt), 0}}};
    Group gtab{"map.gtab_size", m.gtab_size, {}}, reloc{"map.reloc_cap", m.reloc_cap, {}}, comp{"map.comp_cap", m.comp_cap, {}},
        cstage{"map.cstage_cap", m.cstage_cap, {}};
    for (int l = 0; l < BUCKET_LEVELS; ++l) {
        batch.members.push_back({IT(m, d_rank[l]), 27 * SORTED_LEVELS});
        batch.members.push_back({IT(m, d_prank[l]), REPL_LEVELS});
        batch.members.push_back({IT(m, d_pslot[l]), REPL_LEVELS});
        gtab.members.push_back({IT(m, d_gtab[l]), 1});
        gtab.members.push_back({IT(m, d_gbase[l]), GROUP_TARGETS});
        gtab.members.push_back({IT(m, d_gslot[l]), GROUP_TARGETS});
        gtab.members.push_back({IT(m, d_gdst[l]), GROUP_TARGETS});
        reloc.members.push_back({IT(m, d_reloc[l]), 1});
        comp.members.push_back({IT(m, d_comp[l]), 1});
        cstage.members.push_back({IT(m, d_cstage[l]), 1});
        cstage.members.push_back({IT(m, d_cnew[l]), 1});
    }
    g.push_back(batch); g.push_back(gtab); g.push_back(reloc); g.push_back(comp); g.push_back(cstage);
    g.push_back({"map.broken_cap", m.broken_cap, {{IT(m, d_broken), 1}, {IT(m, d_regroup), 1}}});
    g.push_back({"map.box_size", m.box_size, {{IT(m, d_box), 1}}});
    g.push_back({"scan.capacity", s.capacity, {{IT(s, d_raw), 1}, {IT(s, d_sorted), 1}, {IT(s, d_keys), 1}, {IT(s, d_keys_sorted), 1}, {IT(s, d_idx), 1},
                                               {IT(s, d_idx_sorted), 1}, {IT(s, d_sort_tmp), 0}}});
    g.push_back({"scan.raw_cap", s.raw_cap, {{IT(s, d_in), 1}, {IT(s, d_times), 1}, {IT(s, d_desk), 1}, {IT(s, d_vkeys), 1}, {IT(s, d_vkeys_sorted), 1},
                                             {IT(s, d_vidx), 1}, {IT(s, d_vidx_sorted), 1}, {IT(s, d_heads), 1}, {IT(s, d_hpos), 1},
                                             {IT(s, d_vsort_tmp), 0}, {IT(s, d_vscan_tmp), 0}}});
    g.push_back({"cloud.raw_cap", c.raw_cap, {{IT(c, d_rawmsg), 1}, {IT(c, h_rawmsg), 1}, {IT(c, h_rawmsg2), 1}}});
    g.push_back({"cloud.msg_cap", c.msg_cap, {{IT(c, d_decoded), 1}, {IT(c, d_kept), 1}, {IT(c, d_keep), 1}, {IT(c, d_keys), 1}, {IT(c, d_keys_sorted), 1},
                                              {IT(c, d_ids), 1}, {IT(c, d_ids_sorted), 1}, {IT(c, d_tmp), 0}}});
    return g;
}
// no field exceeds the cap of a member of its group (scale 0: the member only has to be there); a buffer with a block has room, one
// without has none
static bool sound(const Stores& S, std::string* why) {
    for (const Group& g : groups(S))
        for (const auto& mb : g.members)
            if (g.value && (!mb.first.there || g.value * mb.second > mb.first.cap)) { *why = g.field + " over " + mb.first.name; return false; }
    for (const Item& i : items(S))
        if (i.name.find('.') == std::string::npos && i.there != (i.cap != 0)) { *why = i.name + " block and cap disagree"; return false; }
    return true;
}
static bool same(const std::vector<Item>& x, const std::vector<Item>& y, std::string* why) {
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].cap != y[i].cap || x[i].there != y[i].there) { *why = x[i].name; return false; }
    return true;
}
static void release(Stores& S) { S.map.release(); S.scan.release(); S.cloud.release(); }

// ---- the reserve paths: a state to start from (reached without failures) and the request under test -----------------------------------
struct Path {
    const char* name;
    std::function<int(Stores&)> setup, request;
};
static std::vector<Path> paths() {
    return {
        {"map_reserve_first", [](Stores&) { return 0; }, [](Stores& S) { return S.map.reserve(3000); }},
        {"map_reserve_grow",   // (with the chains and the positions by id in place, as after a build and a down-sampling add)
         [](Stores& S) {
             int rc = S.map.reserve(3000);
             S.map.n_ids = 3000;
             rc = rc ? rc : S.map.reserve_boxes();
             for (int l = 0; l < BUCKET_LEVELS && !rc; ++l) rc = S.map.d_backpos[l].resize(S.map.capacity * 27);
             return rc ? rc : S.map.d_cellpos.resize(S.map.capacity);
         },
         [](Stores& S) { return S.map.reserve(4097); }},
        {"map_reserve_batch_first", [](Stores&) { return 0; }, [](Stores& S) { return S.map.reserve_batch(600); }},
        {"map_reserve_batch_grow", [](Stores& S) { return S.map.reserve_batch(600); }, [](Stores& S) { return S.map.reserve_batch(4100); }},
        {"map_alive_scratch_first", [](Stores& S) { return S.map.reserve(3000); }, [](Stores& S) { return S.map.ensure_alive_scratch(); }},
        {"map_alive_scratch_grow",
         [](Stores& S) {
             int rc = S.map.reserve(3000);
             rc = rc ? rc : S.map.ensure_alive_scratch();
             return rc ? rc : S.map.reserve(5000);
         },
         [](Stores& S) { return S.map.ensure_alive_scratch(); }},
        {"map_counters", [](Stores&) { return 0; }, [](Stores& S) { return S.map.ensure_counters(); }},
        {"map_boxes_first", [](Stores& S) { return S.map.reserve(3000); }, [](Stores& S) { return S.map.reserve_boxes(); }},
        {"map_boxes_grow",
         [](Stores& S) {
             int rc = S.map.reserve(3000);
             rc = rc ? rc : S.map.reserve_boxes();
             return rc ? rc : S.map.reserve(9000);
         },
         [](Stores& S) { return S.map.reserve_boxes(); }},
        {"scan_reserve_first", [](Stores&) { return 0; }, [](Stores& S) { return S.scan.reserve(4000); }},
        {"scan_reserve_grow", [](Stores& S) { return S.scan.reserve(4000); }, [](Stores& S) { return S.scan.reserve(4100); }},
        {"scan_raw_first", [](Stores&) { return 0; }, [](Stores& S) { return S.scan.reserve_raw(4000, 2); }},
        {"scan_raw_grow", [](Stores& S) { return S.scan.reserve_raw(4000, 2); }, [](Stores& S) { return S.scan.reserve_raw(4100, 70); }},
        {"scan_tiles_first", [](Stores&) { return 0; }, [](Stores& S) { return S.scan.reserve_tiles(100); }},
        {"scan_tiles_grow", [](Stores& S) { return S.scan.reserve_tiles(100); }, [](Stores& S) { return S.scan.reserve_tiles(1025); }},
        {"cloud_init", [](Stores&) { return 0; }, [](Stores& S) { return S.cloud.init(); }},
        {"cloud_msg_first", [](Stores&) { return 0; }, [](Stores& S) { return S.cloud.reserve_msg(1000, 48000); }},
        {"cloud_msg_grow", [](Stores& S) { return S.cloud.reserve_msg(1000, 48000); }, [](Stores& S) { return S.cloud.reserve_msg(70000, 70000 * 48); }},
        {"cloud_buffer_first", [](Stores&) { return 0; }, [](Stores& S) { return S.cloud.reserve_buffer(g_s1, 1000); }},
        {"cloud_buffer_grow",
         [](Stores& S) {
             const int rc = S.cloud.reserve_buffer(g_s1, 1000);
             S.cloud.size = 200000;
             S.cloud.head = 10000;
             return rc;
         },
         [](Stores& S) { return S.cloud.reserve_buffer(g_s1, (size_t)S.cloud.size + 70000); }},
        {"cloud_buffer_move",
         [](Stores& S) {
             const int rc = S.cloud.reserve_buffer(g_s1, 1000);
             S.cloud.size = 200000;
             S.cloud.head = 150000;
             return rc;
         },
         [](Stores& S) { return S.cloud.reserve_buffer(g_s1, (size_t)S.cloud.size + 70000); }},
    };
}

// every path: the calls of a clean run; then call k failing, for every k
static int failures() {
    for (const Path& p : paths()) {
        Stores clean;
        if (p.setup(clean)) return 2;
        size_t mark = st().log.size();
        if (p.request(clean)) return 2;
        const long n_calls = (long)(st().log.size() - mark);
        const std::vector<Item> clean_items = items(clean);
        mark = st().log.size();
        const int again = p.request(clean);   // (what now fits: no call at all)
        const long n_again = (long)(st().log.size() - mark);
        long n_ehip = 0, n_sound = 0, n_retry = 0, n_same = 0;
        std::string why, first_bad;
        for (long k = 0; k < n_calls; ++k) {
            Stores S;
            if (p.setup(S)) return 2;
            long seen = 0;
            st().fail = [&seen, k](const char*) { return seen++ == k; };
            const int rc = p.request(S);
            st().fail = nullptr;
            const bool e = rc == LV_EHIP, s = sound(S, &why);
            if (!s && first_bad.empty()) first_bad = "k=" + std::to_string(k) + ":" + why;
            const bool r = p.request(S) == LV_OK, q = same(items(S), clean_items, &why);
            if (r && !q && first_bad.empty()) first_bad = "k=" + std::to_string(k) + ":differs:" + why;
            n_ehip += e; n_sound += s; n_retry += r; n_same += q;
            release(S);
        }
        release(clean);
        printf("path %s %ld %d %ld %ld %ld %ld %ld %s\n", p.name, n_calls, again, n_again, n_ehip, n_sound, n_retry, n_same,
               first_bad.empty() ? "-" : first_bad.c_str());
    }
    Stores fresh, used;
    std::string why;
    for (const Path& p : paths()) {   // every path on ONE set of stores, then release: nothing left, the stores as new
        if (std::string(p.name).find("_first") == std::string::npos && std::string(p.name) != "cloud_init" && std::string(p.name) != "map_counters") continue;
        if (p.request(used)) return 2;
    }
    release(used);
    printf("released %ld %ld %d %ld %ld\n", (long)st().mallocs, (long)st().frees, same(items(used), items(fresh), &why), (long)st().events_created,
           (long)st().events_destroyed);
    return 0;
}

// capacities after requests at the floor, at floor + 1 and at 5 x floor
static int growth() {
    Stores S;
    const size_t f = 4096;
    for (size_t n : {f, f + 1, 5 * f}) {
        int rc = S.map.reserve(n);
        printf("map_reserve %d %zu %zu %zu %zu %zu\n", rc, S.map.capacity, S.map.d_orig.cap, S.map.d_idx_sorted.cap, S.map.d_dead.cap, S.map.d_sort_tmp.cap);
        rc = S.map.ensure_alive_scratch();
        printf("map_alive %d %zu %zu %zu\n", rc, S.map.d_alive.cap, S.map.d_apos.cap, S.map.d_ascan_tmp.cap);
        rc = S.map.reserve_boxes();
        printf("map_boxes %d %u %zu %zu\n", rc, S.map.box_size, S.map.d_box.cap, S.map.d_box_next.cap);
        rc = S.map.reserve_batch(n);
        printf("map_batch %d %zu %u %u %u %u %u %zu %zu %zu %zu %zu %zu\n", rc, S.map.batch_cap, S.map.gtab_size, S.map.reloc_cap, S.map.broken_cap,
               S.map.comp_cap, S.map.cstage_cap, S.map.d_rank[1].cap, S.map.d_gbase[0].cap, S.map.d_reloc[1].cap, S.map.d_regroup.cap,
               S.map.d_cstage[0].cap, S.map.d_ntmp.cap);
        rc = S.scan.reserve(n);
        printf("scan_reserve %d %zu %zu %zu\n", rc, S.scan.capacity, S.scan.d_raw.cap, S.scan.d_sort_tmp.cap);
        rc = S.scan.reserve_raw(n, n == f ? 2 : 70);
        printf("scan_raw %d %zu %zu %zu %zu %zu %zu\n", rc, S.scan.raw_cap, S.scan.d_times.cap, S.scan.d_vsort_tmp.cap, S.scan.d_vscan_tmp.cap,
               S.scan.d_states.cap, S.scan.d_bounds.cap);
    }
    for (uint32_t nt : {0u, 1u, 1024u, 1025u, 5000u}) {
        const int rc = S.scan.reserve_tiles(nt);
        printf("scan_tiles %d %zu %ld\n", rc, S.scan.d_tile_order.cap, (long)st().mallocs);
    }
    for (size_t n : {(size_t)65536, (size_t)65537, (size_t)5 * 65536}) {
        const int rc = S.cloud.reserve_msg(n, n * 16);   // (1 MiB, 1 MiB + 16, 5 MiB)
        printf("cloud_msg %d %zu %zu %zu %zu %zu %zu\n", rc, S.cloud.msg_cap, S.cloud.raw_cap, S.cloud.d_kept.cap, S.cloud.d_tmp.cap, S.cloud.d_rawmsg.cap,
               S.cloud.h_rawmsg2.cap);
    }
    for (size_t n : {(size_t)1 << 18, ((size_t)1 << 18) + 1, (size_t)5 << 18}) {
        const int rc = S.cloud.reserve_buffer(g_s1, n);
        printf("cloud_buffer %d %zu\n", rc, S.cloud.d_buf.cap);
    }
    // the wait before the pinned stagings go
    const size_t mark = st().log.size();
    int rc = S.cloud.reserve_msg(10, (size_t)16 << 20);
    printf("cloud_msg_log %d", rc);
    for (size_t i = mark; i < st().log.size(); ++i) printf(" %s", st().log[i].call.c_str());
    printf("\n");
    release(S);
    printf("released %ld %ld\n", (long)st().mallocs, (long)st().frees);
    return 0;
}

// what a growth keeps
static int contents() {
    Stores S;
    MapStore& m = S.map;
    int rc = m.reserve(3000);
    m.n_ids = 3000;
    rc = rc ? rc : m.reserve(4000);   // (fits: nothing moves)
    const float4* before = m.d_orig.p;
    for (uint32_t i = 0; i < m.n_ids; ++i) m.d_orig[i] = make_float4((float)i, 1.f, 2.f, 3.f);
    rc = rc ? rc : m.reserve(4097);
    bool kept = true;
    for (uint32_t i = 0; i < m.n_ids; ++i) kept = kept && m.d_orig[i].x == (float)i && m.d_orig[i].w == 3.f;
    printf("orig_alone %d %zu %d %d %d %d\n", rc, m.capacity, kept, m.d_orig.p != before, m.d_box_next.p == nullptr, m.d_cellpos.p == nullptr);
    // ... with the chains and the positions by id
    rc = m.reserve_boxes();
    for (int l = 0; l < BUCKET_LEVELS && !rc; ++l) rc = m.d_backpos[l].resize(m.capacity * 27);
    rc = rc ? rc : m.d_cellpos.resize(m.capacity);
    m.n_ids = 8000;
    for (uint32_t i = 0; i < m.n_ids; ++i) {
        m.d_orig[i] = make_float4((float)i, 0.f, 0.f, 7.f);
        m.d_box_next[i] = i ^ 0x5555u;
        m.d_cellpos[i] = i * 3u;
        for (int l = 0; l < BUCKET_LEVELS; ++l)
            for (int c = 0; c < 27; ++c) m.d_backpos[l][(size_t)i * 27 + c] = (uint16_t)(i * 31u + (uint32_t)c + (uint32_t)l);
    }
    const size_t mark = st().log.size();
    rc = rc ? rc : m.reserve(8193);
    bool k_orig = true, k_next = true, k_cell = true, k_back = true;
    for (uint32_t i = 0; i < m.n_ids; ++i) {
        k_orig = k_orig && m.d_orig[i].x == (float)i && m.d_orig[i].w == 7.f;
        k_next = k_next && m.d_box_next[i] == (i ^ 0x5555u);
        k_cell = k_cell && m.d_cellpos[i] == i * 3u;
        for (int l = 0; l < BUCKET_LEVELS; ++l)
            for (int c = 0; c < 27; ++c) k_back = k_back && m.d_backpos[l][(size_t)i * 27 + c] == (uint16_t)(i * 31u + (uint32_t)c + (uint32_t)l);
    }
    printf("by_id %d %zu %d %d %d %d %zu %zu %zu\n", rc, m.capacity, k_orig, k_next, k_cell, k_back, m.d_box_next.cap, m.d_cellpos.cap, m.d_backpos[1].cap);
    printf("orig_log");
    for (size_t i = mark; i < mark + 5 && i < st().log.size(); ++i) printf(" %s", st().log[i].call.c_str());
    printf("\n");
    // the LiDAR buffer: the living range [head, size) on both branches
    CloudStore& c = S.cloud;
    for (int branch = 0; branch < 2; ++branch) {
        rc = c.reserve_buffer(g_s1, 1000);
        for (uint32_t i = 0; i < 200000; ++i) { c.d_buf[i] = CloudPoint{}; c.d_buf[i].time = (double)i; c.d_buf[i].x = (float)branch; }
        c.size = 200000;
        c.head = branch == 0 ? 150000 : 10000;
        const uint32_t head = c.head, live = c.size - c.head;
        const size_t cap0 = c.d_buf.cap, mk = st().log.size();
        const long mallocs0 = (long)st().mallocs;
        rc = rc ? rc : c.reserve_buffer(g_s1, 270000);
        bool ok_live = c.size == live && c.head == 0;
        for (uint32_t j = 0; j < live; ++j) ok_live = ok_live && c.d_buf[j].time == (double)(head + j) && c.d_buf[j].x == (float)branch;
        printf("cloud_%s %d %zu %zu %d %ld", branch == 0 ? "move" : "grow", rc, cap0, c.d_buf.cap, ok_live, (long)st().mallocs - mallocs0);
        for (size_t i = mk; i < st().log.size(); ++i) printf(" %s%s", st().log[i].call.c_str(), st().log[i].stream == g_s1 ? "@1" : "");
        printf("\n");
        c.release();
    }
    release(S);
    printf("released %ld %ld\n", (long)st().mallocs, (long)st().frees);
    return 0;
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    if (hipStreamCreateWithFlags(&g_s1, hipStreamNonBlocking) != hipSuccess) return 2;
    if (which == "failures") return failures();
    if (which == "growth") return growth();
    if (which == "contents") return contents();
    return 2;
}
