// san_snapshot_main.cpp — a stand-alone driver of the state archive's HOST rules for AddressSanitizer + UndefinedBehaviorSanitizer.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_snapshot_spec.py compiles this file TOGETHER with csrc/rcw_rules.hip (it includes it: one translation
// unit, host side only) under -fsanitize=address,undefined and runs the program on the CPU: nothing loads a sanitizer's runtime into Python.
// It plans the record of three shapes (plan_snapshot, snapshot_plan_differs) and puts a valid exported row and every single corruption
// rcw_snapshot_rows_load refuses through validate_snapshot_row — each row in a heap block of exactly row_bytes, so a read past a row's end
// is reported —, carves every feature's per-agent arrays (agent_arrays, carve_agent_arrays) into heap blocks of exactly the carve's total, and
// exits 0 if nothing was reported and the checks below hold.
#include "../raycastworlds.jl_amd/csrc/rcw_rules.hip"

#include <cstdarg>
#include <cstdio>
#include <memory>

// what the unit takes from the other units of the library: the failure text (rcw_api.hip) and the kernel units' geometry rules — none of
// which the archive's rules reach
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

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "san_snapshot_main: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static SnapshotShape shape(int H, int W, bool real64, bool everything)
{
    SnapshotShape s;
    s.H = H; s.W = W; s.nd = 8; s.N = 64; s.Hc = 64; s.real64 = real64;
    if (everything) {
        s.goal = s.seen = s.stats = 1;
        s.view_fmt = RCW_VIEW_GRAY8; s.view_C = 1; s.view_h = 7; s.view_w = 9; s.view_frames = 3;
        s.local_source = RCW_LOCAL_SEEN; s.local_size = 5; s.local_cells = 1;
        s.source_kind = kLayoutBank; s.layouts = 3;
    }
    return s;
}

template <typename T>
static void put(uint8_t* row, const SnapshotPlan& p, SnapshotField f, T v, int index = 0)
{
    std::memcpy(row + p.offset(p.find(f)) + sizeof(T) * (size_t)index, &v, sizeof v);
}

static int run(const SnapshotShape& sh)
{
    SnapshotPlan plan;
    plan_snapshot(sh, &plan);
    uint64_t sum = 0;
    for (int k = 0; k < plan.n; ++k) sum += plan.seg[k].bytes;
    CHECK(plan.n > 0 && plan.n <= kSnapshotMaxSegments && sum == plan.row_bytes && plan.key != 0);
    CHECK(snapshot_plan_differs(plan, plan) == nullptr);
    const size_t nb = (size_t)plan.row_bytes;
    const int H = sh.H, W = sh.W;
    const auto fresh = [&] {                                                    // exactly row_bytes on the heap: a read past the end is reported
        std::unique_ptr<uint8_t[]> r(new uint8_t[nb]);
        std::memset(r.get(), 0, nb);
        if (sh.real64) { put<double>(r.get(), plan, kSnapPos, 1.5); put<double>(r.get(), plan, kSnapPos, 2.25, 1); }
        else { put<float>(r.get(), plan, kSnapPos, 1.5f); put<float>(r.get(), plan, kSnapPos, 2.25f, 1); }
        put<int32_t>(r.get(), plan, kSnapDir, sh.nd - 1);
        put<int32_t>(r.get(), plan, kSnapGoal, 2); put<int32_t>(r.get(), plan, kSnapGoal, W - 1, 1);
        uint8_t* const map = r.get() + plan.offset(plan.find(kSnapTileMap));
        for (int j = 0; j < W; ++j)
            for (int i = 0; i < H; ++i)
                if (i == 0 || i == H - 1 || j == 0 || j == W - 1) { const unsigned b = 2u * (unsigned)(i + H * j); map[b >> 3] |= (uint8_t)(1u << (b & 7u)); }
        if (sh.source_kind) put<int32_t>(r.get(), plan, kSnapSourceLayout, sh.layouts - 1);
        return r;
    };
    char msg[256];
    { auto r = fresh(); CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_OK); }
    { auto r = fresh(); put<int32_t>(r.get(), plan, kSnapGoal, 1); CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT && !std::strncmp(msg, "goal:", 5)); }
    { auto r = fresh(); put<int32_t>(r.get(), plan, kSnapDir, sh.nd); CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT && !std::strncmp(msg, "dir:", 4)); }
    { auto r = fresh(); put<int32_t>(r.get(), plan, kSnapDir, INT32_MIN); CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT); }
    {
        auto r = fresh();
        if (sh.real64) put<double>(r.get(), plan, kSnapPos, std::nan("")); else put<float>(r.get(), plan, kSnapPos, std::nanf(""));
        CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT && !std::strncmp(msg, "pos", 3));
    }
    { auto r = fresh(); r[plan.offset(plan.find(kSnapTileMap))] ^= 1; CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT && !std::strncmp(msg, "tile_map:", 9)); }
    if (2u * (unsigned)(H * W) < 8u * plan.seg[plan.find(kSnapTileMap)].bytes)                                      // (the map's last bit is padding)
    { auto r = fresh(); r[plan.offset(plan.find(kSnapTileMap)) + plan.seg[plan.find(kSnapTileMap)].bytes - 1] |= 0x80; CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT && !std::strncmp(msg, "tile_map:", 9)); }
    if (sh.source_kind) {
        auto r = fresh();
        put<int32_t>(r.get(), plan, kSnapSourceLayout, sh.layouts);
        CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT && !std::strncmp(msg, "layout_source.layout:", 21));
        put<int32_t>(r.get(), plan, kSnapSourceLayout, INT32_MAX);
        CHECK(validate_snapshot_row(sh, plan, r.get(), msg, sizeof msg) == RCW_ERR_INVALID_ARGUMENT);
    }
    { auto r = fresh(); char tiny[8]; put<int32_t>(r.get(), plan, kSnapGoal, INT32_MIN); CHECK(validate_snapshot_row(sh, plan, r.get(), tiny, sizeof tiny) == RCW_ERR_INVALID_ARGUMENT && std::strlen(tiny) < sizeof tiny); }
    return 0;
}

// The carve of every feature of a shape for B agents, as a setter uses it: a heap block of exactly `total` bytes, the head written at its start,
// every part's [B] array written at its offset with a byte of its own — a write past the block is reported —, and then every byte still holds
// what its part wrote: no two parts, and no part and the head, share one.  The archived parts, feature by feature, are the record's segments.
static int carve(const SnapshotShape& sh, int B)
{
    SnapshotPlan plan;
    plan_snapshot(sh, &plan);
    int seg = 0;
    for (int f = 0; f < kFeatCount; ++f) {
        AgentArrays a;
        agent_arrays(sh, f, &a);
        CHECK(a.n >= 0 && a.n <= kAgentMaxParts && (a.n > 0 || a.head == 0));
        const AgentCarve c = carve_agent_arrays(a.head, a.part, a.n, (uint64_t)B);
        CHECK(c.total >= a.head && c.total % 16 == 0);
        if (c.total == 0) continue;                                             // (a feature that is off carves nothing)
        std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)c.total]);
        std::memset(buf.get(), 0xEE, (size_t)c.total);
        std::memset(buf.get(), 0xAA, (size_t)a.head);
        for (int k = 0; k < a.n; ++k) {
            CHECK(c.off[k] % 16 == 0 && a.part[k].id >= kFeatureFirstId[f] && a.part[k].id < kFeatureFirstId[f + 1] && (k == 0 || a.part[k].id > a.part[k - 1].id));
            std::memset(buf.get() + c.off[k], k + 1, (size_t)B * a.part[k].bytes);
            if (a.part[k].archived) { CHECK(seg < plan.n && plan.seg[seg].field == a.part[k].id && plan.seg[seg].bytes == a.part[k].bytes); ++seg; }
        }
        for (uint64_t i = 0; i < a.head; ++i) CHECK(buf[i] == 0xAA);
        for (int k = 0; k < a.n; ++k)
            for (uint64_t i = 0; i < (uint64_t)B * a.part[k].bytes; ++i) CHECK(buf[c.off[k] + i] == k + 1);
    }
    CHECK(seg == plan.n);
    return 0;
}

int main()
{
    const SnapshotShape shapes[] = {shape(8, 8, false, false), shape(4, 4, false, true), shape(5, 5, true, true), shape(5, 7, true, false)};
    for (const SnapshotShape& s : shapes)
        if (run(s)) return 1;
    SnapshotShape f64_5x5 = shape(5, 5, true, false);                           // (tests/test_agent_arrays_spec.py's shapes and batches)
    f64_5x5.goal = f64_5x5.seen = f64_5x5.stats = 1;
    for (const SnapshotShape& s : {shape(4, 4, false, true), f64_5x5, shape(7, 9, false, true)})
        for (int B : {1, 3, 5, 63, 64, 65, 257})
            if (carve(s, B)) return 1;
    SnapshotPlan a, b;
    plan_snapshot(shapes[1], &a);
    SnapshotShape other = shapes[1];
    other.view_h = 9; other.view_w = 7;
    plan_snapshot(other, &b);
    CHECK(a.row_bytes == b.row_bytes && a.key != b.key && !std::strcmp(snapshot_plan_differs(a, b), "learner_view.stack"));
    plan_snapshot(shape(4, 4, false, false), &b);
    CHECK(!std::strcmp(snapshot_plan_differs(a, b), "goal_distance.field"));
    plan_snapshot(shapes[0], &b);
    CHECK(!std::strcmp(snapshot_plan_differs(a, b), "tile_map"));
    std::puts("san_snapshot_main: ok");
    return 0;
}
