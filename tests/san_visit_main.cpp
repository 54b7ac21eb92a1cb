// san_visit_main.cpp — a stand-alone driver of the visit map's HOST rules (rcw_visit_cell, the plan of kFeatVisits) for AddressSanitizer +
// UndefinedBehaviorSanitizer.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_visit_map_spec.py compiles this file TOGETHER with csrc/rcw_rules.hip (it includes it: one
// translation unit, host side only) under -fsanitize=address,undefined and runs the program on the CPU: nothing loads a sanitizer's runtime
// into Python.  The inputs are the hostile ones: positions that are huge, negative, not finite, exactly on a tile's edge; the largest map
// with eight sectors (the cell index just below 2^31 / 4096); sectors and directions out of range; and the plan of shapes whose table,
// cells * (1 + rows) * 4 bytes, would pass 32 bits — the rows rule must answer 0 rows without a wrapped product.  Every result is held to
// the definition.  Exits 0 if nothing was reported and the checks hold.
#include "../raycastworlds.jl_amd/csrc/rcw_rules.hip"

#include <cstdarg>
#include <cstdio>
#include <limits>

// what the unit takes from the other units of the library (tests/san_frontier_main.cpp): none of which these rules reach
int (fail)(int code, const char*, ...) { return code; }
#ifdef RCW_DEV_SWITCHES
int fail_at(const char*, int, int code, const char*, ...) { return code; }
#endif
const char* hip_failure(hipError_t) { return ""; }
int hip_code(hipError_t) { return RCW_ERR_HIP; }
size_t rcw_step_lds_bytes(const RcwDev&) { return 0; }
size_t rcw_top_view_lds_bytes(const RcwDev&) { return 0; }
int rcw_top_split_unit(const RcwPlan&) { return 0; }
int rcw_top_flat_cols(const RcwPlan&) { return 0; }
int32_t rcw_top_plane_words(const RcwDev&) { return 0; }
int rcw_fill_flat_cols(const RcwDev&) { return 0; }
int rcw_fill_takes_256(const RcwPlan&, long long) { return 0; }
int rcw_fill_window_columns(const RcwPlan&, long long) { return 0; }
size_t rcw_top_plane_bytes(const RcwDev&) { return 0; }
size_t rcw_top_codes_bytes(const RcwDev&) { return 0; }
int rcw_top_draw_per_cu(const RcwDev&, int, int, int) { return 0; }
int rcw_step_spec_eligible(const RcwPlan&) { return 0; }
size_t rcw_step_spec_slot_bytes(const RcwDev&) { return 0; }
int rcw_fill_draw_fusable(const RcwPlan&) { return 0; }
int rcw_view_full_eligible(const RcwDev&, int, int) { return 0; }
size_t rcw_goal_distance_lds_bytes(const RcwDev&) { return 0; }
size_t rcw_seen_map_lds_bytes(const RcwDev&) { return 0; }
size_t rcw_local_map_lds_bytes(const RcwDev&, int32_t, bool) { return 0; }

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "san_visit_main: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static int cell_of(int H, int W, int nd, int sectors, double x, double y, int bits, int d, int32_t* out)
{
    *out = -7;
    return rcw_visit_cell(H, W, nd, sectors, x, y, bits, d, out);
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int32_t c = 0;
    // every (direction, sectors) of three tables on the largest map a handle takes and on the largest the export takes: the cell lies in
    // [0, sectors * H * W) and is the definition's
    const int maps[][2] = {{5, 7}, {255, 254}, {16384, 16383}, {1, 268435455}, {268435455, 1}};
    for (const auto& hw : maps) {
        const int H = hw[0], W = hw[1];
        for (int nd : {8, 16, 130})
            for (int sectors = 1; sectors <= 8; ++sectors)
                for (int d = 0; d < nd; ++d)
                    for (int bits : {32, 64}) {
                        const double x = H - 1 + 0.5, y = W - 1 + 0.25;     // the last tile (Float32 rounds the large ones: the rule must still stay on the map or say -1)
                        CHECK(cell_of(H, W, nd, sectors, x, y, bits, d, &c) == RCW_OK);
                        const long long s = ((long long)d * sectors) / nd, cells = (long long)sectors * H * W;
                        CHECK(c == -1 || (c >= 0 && c < cells && c / ((long long)H * W) == s));
                        if (bits == 64) CHECK(c == s * (long long)H * W + (H - 1) + (long long)H * (W - 1));
                    }
    }
    // positions no kernel may index with
    const double hostile[] = {nan, inf, -inf, -1e300, 1e300, -1.0, -0.5, -1e-30, 5.0, 7.0, 1e9, 4294967296.0, 9223372036854775808.0, -2147483649.0};
    for (double v : hostile)
        for (int bits : {32, 64}) {
            CHECK(cell_of(5, 5, 8, 2, v, 1.5, bits, 7, &c) == RCW_OK && c == -1);
            CHECK(cell_of(5, 5, 8, 2, 1.5, v, bits, 7, &c) == RCW_OK && c == -1);
        }
    for (int bits : {32, 64}) {
        CHECK(cell_of(5, 7, 8, 1, -0.0, 0.0, bits, 0, &c) == RCW_OK && c == 0);
        CHECK(cell_of(5, 7, 8, 1, 3.0, 2.0, bits, 0, &c) == RCW_OK && c == 3 + 5 * 2);
        CHECK(cell_of(5, 7, 8, 1, 4.999, 6.999, bits, 0, &c) == RCW_OK && c == 4 + 5 * 6);
    }
    CHECK(cell_of(5, 7, 8, 1, 4.99999999, 0.5, 64, 0, &c) == RCW_OK && c == 4);
    CHECK(cell_of(5, 7, 8, 1, 4.99999999, 0.5, 32, 0, &c) == RCW_OK && c == -1);        // (Float32 rounds it to 5: off the map)
    // refused
    CHECK(rcw_visit_cell(5, 5, 8, 1, 1.5, 1.5, 32, 0, nullptr) == RCW_ERR_INVALID_ARGUMENT);
    const int bad[][6] = {{0, 5, 8, 1, 32, 0}, {5, 0, 8, 1, 32, 0}, {-1, 5, 8, 1, 32, 0}, {5, 5, 0, 1, 32, 0}, {5, 5, 8, 0, 32, 0}, {5, 5, 8, 9, 32, 0},
                          {5, 5, 4, 5, 32, 0}, {5, 5, 8, -1, 32, 0}, {5, 5, 8, 1, 16, 0}, {5, 5, 8, 1, 32, -1}, {5, 5, 8, 1, 32, 8},
                          {16384, 16384, 8, 1, 32, 0}, {2147483647, 2147483647, 8, 1, 64, 0}, {5, 5, 2147483647, 8, 32, 2147483647}};
    for (const auto& b : bad) CHECK(cell_of(b[0], b[1], b[2], b[3], 1.5, 1.5, b[4], b[5], &c) == RCW_ERR_INVALID_ARGUMENT && c == -7);
    CHECK(cell_of(5, 5, 2147483647, 8, 1.5, 1.5, 32, 2147483646, &c) == RCW_OK && c == 7 * 25 + 1 + 5);   // (d * sectors passes 32 bits)

    // the plan: the parts, and the table's rows under the byte cap
    SnapshotShape sh;
    sh.H = 255; sh.W = 254; sh.nd = 128; sh.N = 8; sh.Hc = 8;
    AgentArrays a;
    agent_arrays(sh, kFeatVisits, &a);
    CHECK(a.n == 0 && a.head == 0);                                                    // off: no parts, no head
    sh.visit_sectors = 8;
    agent_arrays(sh, kFeatVisits, &a);
    CHECK(a.n == 6 && a.head == 0 && a.part[5].bytes == 2u * 8u * 255u * 254u && a.part[5].tag == 8);
    for (int k = 0; k < a.n; ++k) CHECK(a.part[k].archived);
    sh.visit_flags = RCW_VISIT_TABLE;
    int32_t rows = -1, first = -1;
    const uint64_t cells = 8ull * 255 * 254;
    struct Case { int kind, layouts, levels, first_level; int32_t rows, first; };
    const Case cases[] = {
        {kLayoutNone, 0, 0, 0, 0, 0},
        {kLayoutBank, 3, 0, 0, 3, 0},
        {kLayoutBank, 129, 0, 0, 129, 0},                  // 130 rows of 2,072,640 bytes = 269,443,200: past the cap by a hair, so 0 rows (taken below)
        {kLayoutBank, 2072, 0, 0, 0, 0},                   // cells * (1 + rows) * 4 = 2^32 + ...: the product must not wrap into the cap
        {kLayoutMazes, 0, 65536, 5, 0, 0},                 // 65537 rows: far past 32 bits
        {kLayoutMazes, 0, 100, 2147483000, 100, 2147483000},
        {kLayoutMazes, 0, 65537, 3, 0, 0},                 // the statistics' own bound
        {kLayoutCaves, 0, 0, 7, 0, 0},
    };
    for (const Case& k : cases) {
        sh.source_kind = k.kind; sh.layouts = k.layouts; sh.levels = k.levels; sh.first_level = k.first_level;
        plan_visit_table_rows(sh, &rows, &first);
        int32_t want_rows = k.rows, want_first = k.first;
        if (cells * (1 + (uint64_t)want_rows) * 4 > RCW_VISIT_TABLE_MAX_BYTES) { want_rows = 0; want_first = 0; }
        CHECK(rows == want_rows && first == want_first);
        agent_arrays(sh, kFeatVisits, &a);
        CHECK(a.head == 4 * cells * (1 + (uint64_t)rows) && a.head <= RCW_VISIT_TABLE_MAX_BYTES);
        const AgentCarve carve = carve_agent_arrays(a.head, a.part, a.n, 1u << 20);     // a million agents: 64-bit offsets
        CHECK(carve.total >= a.head + (2 * cells + 20) * (1ull << 20));
        SnapshotPlan plan;
        plan_snapshot(sh, &plan);
        CHECK(plan.n == 15 + (k.kind ? 2 : 0) && plan.seg[plan.n - 1].field == kSnapVisitMap && plan.row_bytes < (1ull << 32));
    }
    // the wrap itself: 4 * cells * 2073 = 2^32 + 1,615,424 — in 32 bits that is 1.6 MB, under the cap
    CHECK((uint32_t)(4 * cells * 2073) < RCW_VISIT_TABLE_MAX_BYTES && 4 * cells * 2073 > RCW_VISIT_TABLE_MAX_BYTES);
    // a small map takes every row the statistics take
    sh.H = 5; sh.W = 5; sh.visit_sectors = 1; sh.source_kind = kLayoutMazes; sh.layouts = 0; sh.levels = 65536; sh.first_level = -9;
    plan_visit_table_rows(sh, &rows, &first);
    CHECK(rows == 65536 && first == -9);
    std::puts("san_visit_main: ok");
    return 0;
}
