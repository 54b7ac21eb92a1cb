// san_frontier_main.cpp — a stand-alone driver of the frontier's HOST flood (rcw_frontier_rule) for AddressSanitizer + UndefinedBehaviorSanitizer.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_frontier_spec.py compiles this file TOGETHER with csrc/rcw_rules.hip (it includes it: one translation
// unit, host side only) under -fsanitize=address,undefined and runs the program on the CPU: nothing loads a sanitizer's runtime into Python.
// Every map and every field lies in a heap block of exactly its size, so a read or a write past either end is reported.  The inputs are the
// hostile ones: maps of every byte value, maps that are all unseen, all passable, passable with one unseen tile in each corner and on each
// edge — whose neighbours are off the map —, checkerboards of passable and unseen tiles (the most sources a map can have), at 5 x 5,
// at the largest size (H*W = 65535, as 255 x 257, 257 x 255, 1 x 65535, 65535 x 1), 1 x n and n x 1 strips; and every refused argument.
// Every result is held to the definition's invariants.  Exits 0 if nothing was reported and the checks hold.
#include "../raycastworlds.jl_amd/csrc/rcw_rules.hip"

#include <cstdarg>
#include <cstdio>
#include <memory>

// what the unit takes from the other units of the library (tests/san_guide_main.cpp): none of which the flood reaches
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

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "san_frontier_main: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static bool passable(uint8_t v) { return v == 1 || v == 3; }

// the flood of an H x W map filled by fill(i, j), both arrays in heap blocks of exactly H*W entries, and the definition's invariants:
// tiles counts the zeros; a zero lies on an unseen tile with a passable neighbour on the map, and every such tile holds one; a value
// f >= 1 lies on a passable tile that has a neighbour holding f - 1 and none holding less; nothing else holds anything but 0xFFFF.
template <typename Fill>
static int run(int H, int W, Fill fill, int32_t* tiles_out)
{
    const size_t HW = (size_t)H * (size_t)W;
    std::unique_ptr<uint8_t[]> map(new uint8_t[HW]);
    std::unique_ptr<uint16_t[]> field(new uint16_t[HW]);
    for (int j = 0; j < W; ++j)
        for (int i = 0; i < H; ++i) map[(size_t)i + (size_t)H * (size_t)j] = (uint8_t)fill(i, j);
    for (size_t t = 0; t < HW; ++t) field[t] = 0x1234;
    int32_t tiles = -7;
    CHECK(rcw_frontier_rule(H, W, map.get(), field.get(), &tiles) == RCW_OK);
    int32_t zeros = 0;
    for (int j = 0; j < W; ++j)
        for (int i = 0; i < H; ++i) {
            const size_t t = (size_t)i + (size_t)H * (size_t)j;
            const int side[4][2] = {{i - 1, j}, {i + 1, j}, {i, j - 1}, {i, j + 1}};
            bool beside_passable = false;
            uint32_t least = 0xFFFFu;
            for (const auto& s : side) {
                if (s[0] < 0 || s[0] >= H || s[1] < 0 || s[1] >= W) continue;
                const size_t n = (size_t)s[0] + (size_t)H * (size_t)s[1];
                beside_passable = beside_passable || passable(map[n]);
                if ((passable(map[n]) || field[n] == 0) && field[n] < least) least = field[n];
            }
            const uint32_t f = field[t];
            if (map[t] == 0 && beside_passable) { CHECK(f == 0); ++zeros; }
            else if (passable(map[t])) CHECK(f == (least == 0xFFFFu ? 0xFFFFu : least + 1u));
            else CHECK(f == 0xFFFFu);
        }
    CHECK(tiles == zeros);
    *tiles_out = tiles;
    return 0;
}

int main()
{
    int32_t tiles = 0;
    const int shapes[][2] = {{5, 5}, {255, 257}, {257, 255}, {1, 65535}, {65535, 1}, {1, 1}, {1, 2}, {2, 1}, {1, 9}, {9, 1}, {2, 2}, {3, 7}};
    for (const auto& hw : shapes) {
        const int H = hw[0], W = hw[1];
        for (int v = 0; v < 256; v += (size_t)H * W > 1000 ? 51 : 1) {                          // every byte value (the large maps: six of them)
            CHECK(run(H, W, [&](int, int) { return v; }, &tiles) == 0 && tiles == 0);
            CHECK(run(H, W, [&](int i, int j) { return (i + j) & 1 ? v : 1; }, &tiles) == 0);    // ... in a checkerboard with passable tiles
            CHECK(run(H, W, [&](int i, int j) { return (i * 7 + j * 13 + v) & 255; }, &tiles) == 0);   // ... and every value at once
        }
        CHECK(run(H, W, [&](int i, int j) { return (i + j) & 1 ? 0 : 3; }, &tiles) == 0);
        CHECK(tiles == (int32_t)(((size_t)H * W) / 2) || (size_t)H * W == 1);
        // passable everywhere but one unseen tile in a corner or on an edge: the farthest tile is a whole map away
        const int at[][2] = {{0, 0}, {H - 1, 0}, {0, W - 1}, {H - 1, W - 1}, {H / 2, 0}, {0, W / 2}, {H - 1, W / 2}, {H / 2, W - 1}};
        for (const auto& p : at) {
            CHECK(run(H, W, [&](int i, int j) { return i == p[0] && j == p[1] ? 0 : 1; }, &tiles) == 0);
            CHECK(tiles == ((size_t)H * W > 1 ? 1 : 0));
        }
        // a serpentine of passable tiles between walls, the unseen tile at its far end: as many levels as a map can have
        CHECK(run(H, W, [&](int i, int j) { return i == 0 && j == 0 ? 0 : ((j & 1) == 0 || i == ((j >> 1) & 1 ? 0 : H - 1) ? 1 : 2); }, &tiles) == 0);
    }
    // the column-wrap pair alone
    CHECK(run(4, 4, [&](int i, int j) { return i == 3 && j == 1 ? 1 : (i == 0 && j == 2 ? 0 : 2); }, &tiles) == 0 && tiles == 0);
    // refused
    uint8_t m[25] = {};
    uint16_t f[25];
    CHECK(rcw_frontier_rule(5, 5, nullptr, f, &tiles) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_frontier_rule(5, 5, m, nullptr, &tiles) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_frontier_rule(5, 5, m, f, nullptr) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_frontier_rule(0, 5, m, f, &tiles) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_frontier_rule(5, -1, m, f, &tiles) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_frontier_rule(256, 256, m, f, &tiles) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_frontier_rule(65536, 65536, m, f, &tiles) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_frontier_rule(2147483647, 2147483647, m, f, &tiles) == RCW_ERR_INVALID_ARGUMENT);
    std::puts("san_frontier_main: ok");
    return 0;
}
