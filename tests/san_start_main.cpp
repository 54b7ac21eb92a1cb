// san_start_main.cpp — a stand-alone driver of the start rule's HOST restatement (rcw_start_rule) for AddressSanitizer + UndefinedBehaviorSanitizer.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_start_distance_san.py compiles this file TOGETHER with csrc/rcw_rules.hip (it includes it: one
// translation unit, host side only) under -fsanitize=address,undefined and runs the program on the CPU: nothing loads a sanitizer's runtime
// into Python.  Every map lies in a heap block of exactly its size, so a read past either end is reported.  The maps are the hand-made ones
// of tests/start_distance_ref.py — the 5 x 70 corridor, the 7 x 7 of isolated cells, the two sealed rooms on 9 x 12 — and the hostile ones:
// maps WITHOUT a wall ring (a flood that reaches every edge and corner), of one tile, one row, one column, all wall, all free; goals on the
// corners, inside walls and off the map; every band edge and every refused argument.  Exits 0 if nothing was reported and the checks hold.
#include "../raycastworlds.jl_amd/csrc/rcw_rules.hip"

#include <cstdarg>
#include <cstdio>
#include <memory>

// what the unit takes from the other units of the library (tests/san_guide_main.cpp): none of which the start rule reaches
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

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "san_start_main: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

// a map of exactly H W bytes; wall(i, j), 0-based
template <typename Wall>
static std::unique_ptr<uint8_t[]> make(int H, int W, Wall wall)
{
    std::unique_ptr<uint8_t[]> m(new uint8_t[(size_t)H * W]);
    for (int j = 0; j < W; ++j)
        for (int i = 0; i < H; ++i) m[(size_t)i + (size_t)H * j] = wall(i, j) ? 1 : 0;
    return m;
}

int main()
{
    int32_t tile = 0, outcome = 0;
    const int32_t MAX = RCW_START_DISTANCE_MAX;
    // (a) the corridor: band (60, 65) from an end, the clamp from the middle
    {
        const auto m = make(5, 70, [](int i, int j) { return i != 2 || j == 0 || j == 69; });
        for (uint64_t key = 0; key < 64; ++key) {
            CHECK(rcw_start_rule(m.get(), 5, 70, 3, 2, key * 0x9e3779b97f4a7c15ull, 60, 65, &tile, &outcome) == RCW_OK);
            CHECK(outcome == RCW_START_IN_BAND && tile % 5 == 2 && tile / 5 - 1 >= 60 && tile / 5 - 1 <= 65);
            CHECK(rcw_start_rule(m.get(), 5, 70, 3, 35, key, 60, 65, &tile, &outcome) == RCW_OK);
            CHECK(outcome == RCW_START_CLAMPED && tile == 2 + 5 * 68);
            CHECK(rcw_start_rule(m.get(), 5, 70, 3, 69, key, 67, MAX, &tile, &outcome) == RCW_OK);
            CHECK(outcome == RCW_START_IN_BAND && tile == 2 + 5 * 1);
        }
    }
    // (b) isolated cells: kept; a goal inside a wall, on the ring, off the map: kept
    {
        const auto m = make(7, 7, [](int i, int j) { return !(i % 2 == 1 && j % 2 == 1); });
        const int goals[][2] = {{2, 2}, {4, 6}, {3, 3}, {1, 1}, {7, 7}, {0, 0}, {8, 2}, {2, 8}, {-5, 3}, {2147483647, 2147483647}, {-2147483647 - 1, 1}};
        for (const auto& g : goals) {
            CHECK(rcw_start_rule(m.get(), 7, 7, g[0], g[1], 5, 1, 2, &tile, &outcome) == RCW_OK);
            CHECK(outcome == RCW_START_KEPT && tile == -1);
        }
    }
    // (c) two sealed rooms: the tile lies in the goal's room
    {
        const auto m = make(9, 12, [](int i, int j) { return i == 0 || i == 8 || j == 0 || j == 11 || j == 4; });
        for (uint64_t key = 0; key < 200; ++key) {
            CHECK(rcw_start_rule(m.get(), 9, 12, 2, 2, key << 56 | key, 1, MAX, &tile, &outcome) == RCW_OK);
            CHECK(outcome == RCW_START_IN_BAND && tile / 9 >= 1 && tile / 9 <= 3 && tile != 1 + 9 * 1);
            CHECK(rcw_start_rule(m.get(), 9, 12, 8, 11, key << 56 | key, 1, MAX, &tile, &outcome) == RCW_OK);
            CHECK(outcome == RCW_START_IN_BAND && tile / 9 >= 5 && tile / 9 <= 10 && tile != 7 + 9 * 10);
        }
    }
    // maps without a ring: the flood looks past every edge and corner
    {
        const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 2}, {3, 5}, {255, 257}};
        for (const auto& s : shapes) {
            const int H = s[0], W = s[1];
            const auto open = make(H, W, [](int, int) { return false; });
            const auto shut = make(H, W, [](int, int) { return true; });
            const int corners[][2] = {{1, 1}, {H, 1}, {1, W}, {H, W}};
            for (const auto& c : corners)
                for (int32_t lo : {1, 2, H + W > 3 ? H + W - 2 : 1, H + W, MAX}) {
                    CHECK(rcw_start_rule(open.get(), H, W, c[0], c[1], 77, lo, MAX, &tile, &outcome) == RCW_OK);
                    if (H * W == 1) CHECK(outcome == RCW_START_KEPT && tile == -1);
                    else CHECK((outcome == (lo <= H + W - 2 ? RCW_START_IN_BAND : RCW_START_CLAMPED)) && tile >= 0 && tile < H * W);
                    CHECK(rcw_start_rule(shut.get(), H, W, c[0], c[1], 77, lo, MAX, &tile, &outcome) == RCW_OK);
                    CHECK(outcome == RCW_START_KEPT && tile == -1);
                }
        }
    }
    // every refused argument changes neither output
    {
        const auto m = make(3, 3, [](int i, int j) { return i != 1 || j != 1; });
        tile = 123; outcome = 45;
        const int32_t bands[][2] = {{0, 3}, {-1, 3}, {4, 3}, {1, MAX + 1}, {0, 0}, {2147483647, 2147483647}, {3, -1}, {-2147483647 - 1, 1}};
        for (const auto& b : bands) CHECK(rcw_start_rule(m.get(), 3, 3, 2, 2, 1, b[0], b[1], &tile, &outcome) == RCW_ERR_INVALID_ARGUMENT);
        CHECK(rcw_start_rule(nullptr, 3, 3, 2, 2, 1, 1, 2, &tile, &outcome) == RCW_ERR_INVALID_ARGUMENT);
        CHECK(rcw_start_rule(m.get(), 3, 3, 2, 2, 1, 1, 2, nullptr, &outcome) == RCW_ERR_INVALID_ARGUMENT);
        CHECK(rcw_start_rule(m.get(), 3, 3, 2, 2, 1, 1, 2, &tile, nullptr) == RCW_ERR_INVALID_ARGUMENT);
        const int sizes[][2] = {{0, 3}, {3, 0}, {-1, 3}, {256, 256}, {65536, 1}, {2147483647, 2147483647}};
        for (const auto& s : sizes) CHECK(rcw_start_rule(m.get(), s[0], s[1], 2, 2, 1, 1, 2, &tile, &outcome) == RCW_ERR_INVALID_ARGUMENT);
        CHECK(tile == 123 && outcome == 45);
        CHECK(rcw_start_rule(m.get(), 3, 3, 2, 2, 1, 1, 2, &tile, &outcome) == RCW_OK && outcome == RCW_START_KEPT);
    }
    std::puts("san_start_main: ok");
    return 0;
}
