// san_guide_main.cpp — a stand-alone driver of the guide's HOST rule (rcw_guide_rule) for AddressSanitizer + UndefinedBehaviorSanitizer.
//
// TEST INFRASTRUCTURE ONLY.  tests/test_guide_spec.py compiles this file TOGETHER with csrc/rcw_rules.hip (it includes it: one translation
// unit, host side only) under -fsanitize=address,undefined and runs the program on the CPU: nothing loads a sanitizer's runtime into Python.
// Every field and every table lies in a heap block of exactly its size, so a read past either end is reported.  The inputs are the
// hostile ones: positions on the corner tiles of the map (whose neighbours are off it), on its edges, off it, NaN, infinite and past
// every integer; fields whose entry has no nearer neighbour, whose every entry is 0, 0xFFFF or 1; tables of one entry, with NaN and
// infinite entries, all NaN; both world-unit types; and every refused argument.  Exits 0 if nothing was reported and the checks hold.
#include "../raycastworlds.jl_amd/csrc/rcw_rules.hip"

#include <cstdarg>
#include <cstdio>
#include <limits>
#include <memory>

// what the unit takes from the other units of the library (tests/san_snapshot_main.cpp): none of which the guide's rule reaches
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

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "san_guide_main: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

// the rule on a table of `nd` entries of T in a block of exactly 2 nd values; fill(k, c): component c of entry k
template <typename T, typename Fill>
static int run(int H, int W, const uint16_t* field, double x, double y, int d, int nd, Fill fill, double inc, uint8_t* action, int32_t* heading)
{
    std::unique_ptr<T[]> table(new T[2 * (size_t)nd]);
    for (int k = 0; k < nd; ++k) { table[2 * (size_t)k] = (T)fill(k, 0); table[2 * (size_t)k + 1] = (T)fill(k, 1); }
    return rcw_guide_rule(H, W, field, x, y, sizeof(T) == 8 ? 64 : 32, d, nd, table.get(), inc, action, heading);
}

template <typename T>
static int hostile()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const auto compass = [](int k, int c) { const double v[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}}; return v[k & 3][c]; };
    const double xs[] = {0.5, 0.0, -0.0, -0.5, -1e-30, 1.5, 2.5, 2.625, 4.5, 4.999999, 5.0, 6.5, 1e9, 3e9, 1e19, 1e300, -1e300, nan, inf, -inf};
    const int shapes[][2] = {{5, 5}, {1, 1}, {1, 7}, {7, 1}, {3, 4}};
    uint8_t action = 0;
    int32_t heading = 0;
    for (const auto& hw : shapes) {
        const int H = hw[0], W = hw[1], HW = H * W;
        std::unique_ptr<uint16_t[]> field(new uint16_t[(size_t)HW]);
        // entry t = t + 1 (linear order: the neighbour in front is nearer), every entry 0, 0xFFFF, 1 (no nearer neighbour), 0xFFFE
        for (int kind = 0; kind < 5; ++kind) {
            for (int t = 0; t < HW; ++t) field[(size_t)t] = kind == 0 ? (uint16_t)(t + 1) : (kind == 1 ? 0 : (kind == 2 ? 0xFFFF : (kind == 3 ? 1 : 0xFFFE)));
            for (const double x : xs)
                for (const double y : xs)
                    for (const int nd : {1, 4, 7}) {
                        CHECK(run<T>(H, W, field.get(), x, y, nd - 1, nd, compass, 0.125, &action, &heading) == RCW_OK);
                        CHECK(action >= 1 && action <= 4 && action != 2 && heading >= -1 && heading < nd);
                        CHECK((heading >= 0) || action == 3);
                        if (kind != 0 && kind != 4) CHECK(heading == -1);   // nothing is nearer: no advice anywhere
                    }
        }
    }
    // hostile tables on a field that has advice: tile (2, 2) of 5 x 5 holds 5, (3, 2) holds 4
    std::unique_ptr<uint16_t[]> f(new uint16_t[25]);
    for (int t = 0; t < 25; ++t) f[(size_t)t] = 0xFFFF;
    f[2 + 5 * 2] = 5; f[3 + 5 * 2] = 4;
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 0, 4, compass, 0.125, &action, &heading) == RCW_OK && heading == 0 && action == 1);
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 0, 3, [&](int, int) { return nan; }, 0.125, &action, &heading) == RCW_OK && heading == 0 && action == 1);
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 1, 3, [&](int, int) { return nan; }, 0.125, &action, &heading) == RCW_OK && heading == 0 && action == 4);
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 0, 4, [&](int k, int c) { return k == 2 ? compass(0, c) : nan; }, 0.125, &action, &heading) == RCW_OK && heading == 2 && action == 3);
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 0, 4, [&](int k, int c) { return k == 1 ? inf : (k == 3 && c == 0 ? -inf : compass(k, c)); }, 0.125, &action, &heading) == RCW_OK);
    CHECK(heading == 0);                                                    // (inf * 1 + inf * 0 is NaN; -inf + 0 loses)
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 0, 65, [&](int k, int c) { return k == 64 ? (c == 0 ? 2.0 : 0.0) : compass(k, c); }, 0.125, &action, &heading) == RCW_OK && heading == 64 && action == 4);
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 0, 1 << 16, compass, -1.0, &action, &heading) == RCW_OK && heading == 0);
    CHECK(run<T>(5, 5, f.get(), 2.5, 2.5, 0, 4, compass, nan, &action, &heading) == RCW_OK);
    // refused
    T one[2] = {1, 0};
    CHECK(rcw_guide_rule(5, 5, nullptr, 2.5, 2.5, 32, 0, 1, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, 5, f.get(), 2.5, 2.5, 32, 0, 1, nullptr, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, 5, f.get(), 2.5, 2.5, 32, 0, 1, one, 0.125, nullptr, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, 5, f.get(), 2.5, 2.5, 32, 0, 1, one, 0.125, &action, nullptr) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(0, 5, f.get(), 2.5, 2.5, 32, 0, 1, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, -1, f.get(), 2.5, 2.5, 32, 0, 1, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(65536, 65536, f.get(), 2.5, 2.5, 32, 0, 1, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, 5, f.get(), 2.5, 2.5, 16, 0, 1, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, 5, f.get(), 2.5, 2.5, 32, 0, 0, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, 5, f.get(), 2.5, 2.5, 32, 1, 1, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    CHECK(rcw_guide_rule(5, 5, f.get(), 2.5, 2.5, 32, -1, 1, one, 0.125, &action, &heading) == RCW_ERR_INVALID_ARGUMENT);
    return 0;
}

int main()
{
    if (hostile<float>() != 0 || hostile<double>() != 0) return 1;
    rcw_config cfg{};
    cfg.world_unit_bits = 32; cfg.player_radius_wu = 0.45f; cfg.position_increment_wu = 0.125f;
    CHECK(guide_promised(cfg) == 0);
    cfg.player_radius_wu = 0.3f; cfg.position_increment_wu = 0.2f;
    CHECK(guide_promised(cfg) == 1);
    std::puts("san_guide_main: ok");
    return 0;
}
