// The host-built tables, and every rule and validation of librcw_hip: no HIP call, and nothing of a handle changes.
// Host code in this file that does floating point follows the reference operation for
// operation and must be compiled with -ffp-contract=off (see Makefile).
#include "rcw_handle.h"
#include "rcw_rng.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

// directions_wu  SR:65-69: theta = (i-1)*2*pi/nd in Float64, components converted to T
template <typename T>
void build_direction_table(int nd, std::vector<T>& out)
{
    out.resize((size_t)2 * nd);
    for (int i = 1; i <= nd; ++i) {
        const double theta = (double)((long long)(i - 1) * 2) * 3.141592653589793 / (double)nd;
        out[2 * (size_t)(i - 1)] = (T)std::cos(theta);
        out[2 * (size_t)(i - 1) + 1] = (T)std::sin(theta);
    }
}

// Per heading d and ray i (SR:214-221, SR:404): the fan end points dir ± fov·rot₋₉₀(dir),
// the LinRange element (Float64 lerp converted to T), its normalisation, and the derived
// |1/dx|, |1/dy| (cast_ray's delta distances) and dir·ray (SR:404).
// Layout [nd][5][N]: see RCW_TABLE_ROWS.  T is the world-unit type; fov = convert(T, .) SR:267.
template <typename T>
void build_ray_table(const rcw_config& c, T fov, const std::vector<T>& dirs, std::vector<T>& out)
{
    const int N = c.num_rays, nd = c.num_directions;
    out.assign((size_t)nd * RCW_TABLE_ROWS * N, (T)0);
    const int lendiv = N - 1 > 1 ? N - 1 : 1;   // LinRange lendiv = max(len - 1, 1)
    for (int d = 0; d < nd; ++d) {
        const T d1 = dirs[2 * (size_t)d], d2 = dirs[2 * (size_t)d + 1];
        const T cam1 = d2, cam2 = -d1;                        // rotate_minus_90 SR:193
        const T fc1 = fov * cam1, fc2 = fov * cam2;
        const T first1 = d1 + fc1, first2 = d2 + fc2;         // SR:216
        const T last1 = d1 - fc1, last2 = d2 - fc2;           // SR:217
        T* row = out.data() + (size_t)d * RCW_TABLE_ROWS * N;
        for (int i = 0; i < N; ++i) {
            const double t = (double)i / (double)lendiv;      // lerpi: t = j/d in Float64
            const double omt = 1.0 - t;
            const double a1 = omt * (double)first1, b1 = t * (double)last1;
            const double a2 = omt * (double)first2, b2 = t * (double)last2;
            const T u1 = (T)(a1 + b1);
            const T u2 = (T)(a2 + b2);
            const T s1 = u1 * u1, s2 = u2 * u2;
            const T nrm = std::sqrt(s1 + s2);                 // norm(SVector) = sqrt(sum abs2)
            T r1, r2;
            if (c.normalize_mode == RCW_NORMALIZE_DIVIDE) {
                r1 = u1 / nrm; r2 = u2 / nrm;
            } else {
                const T inv = (T)1 / nrm;                     // inv(norm(a)) * a
                r1 = inv * u1; r2 = inv * u2;
            }
            const T m1 = d1 * r1, m2 = d2 * r2;               // sum(dir .* ray) SR:404
            row[i] = r1;
            row[(size_t)N + i] = r2;
            row[2 * (size_t)N + i] = std::fabs((T)1 / r1);
            row[3 * (size_t)N + i] = std::fabs((T)1 / r2);
            row[4 * (size_t)N + i] = m1 + m2;
        }
    }
}
template void build_direction_table<float>(int, std::vector<float>&);
template void build_direction_table<double>(int, std::vector<double>&);
template void build_ray_table<float>(const rcw_config&, float, const std::vector<float>&, std::vector<float>&);
template void build_ray_table<double>(const rcw_config&, double, const std::vector<double>&, std::vector<double>&);

// The geometry of a batch as the kernels' argument block holds it: what the launchers' and the top view's rules read (rcw_create; the
// development build's rcw_dev_plan_top_view, which runs the rule without a device).
void set_geometry(RcwPlan& d, const rcw_config* cfg, int32_t batch)
{
    d.B = batch; d.H = cfg->height_tile_map_tu; d.W = cfg->width_tile_map_tu; d.N = cfg->num_rays; d.nd = cfg->num_directions; d.Hc = cfg->height_camera_view_pu;
    d.real64 = cfg->world_unit_bits == 64 ? 1 : 0;
    d.pu = cfg->pu_per_tu;
    // player_radius_pu = wu_to_pu(player_radius_wu, pu_per_tu) SR:469 = floor(Int, r * pu) + 1 in T (UT:6)
    d.top_rp = d.real64 ? (int32_t)std::floor(cfg->player_radius_wu_f64 * (double)cfg->pu_per_tu) + 1
                        : (int32_t)std::floor(cfg->player_radius_wu * (float)cfg->pu_per_tu) + 1;
}

// ---- update_top_view! (SR:446-483): which form a handle takes — the RULES AS DATA ------------------------------------------------------
// Every threshold the choice of a form rests on, with the measurement that put it there.  The rule itself (top_view_rule below) is a pure
// function of the configuration, the batch and three numbers of the device (CUs, LDS and wavefronts a CU: rcw_create reads them from
// hipDeviceProp_t); tests/test_top_view_plan.py runs it on the CPU (development build: rcw_dev_plan_top_view) for every shape of the
// committed profile table and compares with tests/golden/top_view_plan_cases.json — the forms those profiles were taken with.  A retune
// on another box is an edit of this table, a re-run of tools/top_view_shapes.py and of tools/make_top_view_plan_cases.py; a change of a
// rule by accident is a red test.
namespace {
struct TopRule { const char* name; double value; const char* unit; const char* evidence; };
enum TopRuleId {
    kRingThreeBuffersLds, kRingLdsCap, kRingWorkgroupsPerCu, kLineWalkMaxPixels, kAloneTwoKernelsPixels, kAloneTwoKernelsBelowPu,
    kDrawWideBlockLds, kDrawBlockMin, kDrawBlockMax, kAloneBlock64Agents, kAloneBlock128Agents, kRunsLineToCameraNum, kRunsLineToCameraDen,
    kRuns4Gib, kRuns2Gib, kSideStreamMinBytes, kPartsMax, kPartsMinRays, kFillGBperMs, kFillLateStartUs, kDrawUsPerGibFewRays,
    kDrawUsPerGibManyRays, kDrawManyRays, kDrawPartialRound, kDrawLdsCap, kFillWavefrontsPerCu, kTopRuleCount
};
constexpr TopRule kTopRules[kTopRuleCount] = {
    /* kRingThreeBuffersLds   */ {"ring_three_buffers_max_lds", 52 * 1024, "B", "profiles/r02_top_view_summary.txt: three workgroups of 8 wavefronts a CU still fit beside each other up to 52 KiB of ring each"},
    /* kRingLdsCap            */ {"ring_lds_cap", 156 * 1024, "B", "the CU's 160 KiB less what the kernel's static words and the runtime keep: beyond it the in-place form (profiles/r02_top_draw_lds.txt)"},
    /* kRingWorkgroupsPerCu   */ {"ring_workgroups_per_cu_max", 3, "", "profiles/r02_top_view_summary.txt: 3 x 8 wavefronts is what the ring kernel's register use admits; 4 measured no faster"},
    /* kLineWalkMaxPixels     */ {"line_walk_max_pixels", 16384, "px", "exactness, not tuning: the bit-plane kernels step a line on the carry of a 32-bit fraction, exact for lines of up to 2^14 pixels (tests/test_host_logic.py)"},
    /* kAloneTwoKernelsPixels */ {"stand_alone_two_kernels_from_pixels", 65536, "px", "profiles/r05_top_view_shapes.txt (b): draw -> store back to back 217 / 224 / 198 / 210 / 218 us/GiB against 214 / 231 / 228 / 253 / 360 for the ring from 256^2 px up"},
    /* kAloneTwoKernelsBelowPu*/ {"stand_alone_two_kernels_below_pu", 16, "px/tile", "profiles/r05_top_view_shapes.txt (b): 10 / 13 px a tile 360 / 302 against 507 / 450, 12 px 310 against 347; the ring keeps 16, 20, 24 ... px below 256^2 (264 / 228 / 229 against 268 / 246 / 233)"},
    /* kDrawWideBlockLds      */ {"draw_wide_block_from_plane_lds", 64 * 1024, "B", "profiles/r04_top_view_small_batches.txt, r03_top_view_shapes.txt: planes beyond 64 KiB leave one or two workgroups a CU: 512^2 px 180 / 182 / 200, 768^2 212 / 200 / 203, 1024^2 357 / 265 / 216 us with 256 / 512 / 1024 threads"},
    /* kDrawBlockMin          */ {"draw_wide_block_min_threads", 512, "threads", "same measurement"},
    /* kDrawBlockMax          */ {"draw_wide_block_max_threads", 1024, "threads", "same measurement (a lane per ray up to 1024 rays)"},
    /* kAloneBlock64Agents    */ {"stand_alone_64_threads_from_agents", 24576, "agents", "profiles/r05_draw_kernel.txt: 41,943 images of 80^2 px 175 us with 64 threads against 193 with 256"},
    /* kAloneBlock128Agents   */ {"stand_alone_128_threads_from_agents", 12288, "agents", "profiles/r05_draw_kernel.txt: 16,384 images of 128^2 px 103 us with 128 threads against 109"},
    /* kRunsLineToCameraNum   */ {"runs_when_lines_to_camera_num", 7, "", "profiles/r03_top_view_shapes.txt: (H + W) pu / 2 >= 1.75 H_cam, i.e. 2 (H + W) pu >= 7 H_cam: the drawing no longer fits beside the camera fill"},
    /* kRunsLineToCameraDen   */ {"runs_when_lines_to_camera_den", 2, "", "same rule's left-hand factor"},
    /* kRuns4Gib              */ {"four_runs_from_gib", 4, "GiB", "profiles/r03_top_view_shapes.txt: 16 GiB of top view 4516 / 4409 / 4332 / 4294 us with 1 / 2 / 4 / 8 runs, 32 GiB 8586 / 8459 / 7658 / 8068"},
    /* kRuns2Gib              */ {"two_runs_from_gib", 2, "GiB", "same table; runs of 256 MiB do not pay (205 vs 181 us at 1 GiB of 512^2 px images)"},
    /* kSideStreamMinBytes    */ {"side_stream_form_from_bytes", 256.0 * 1048576.0, "B", "profiles/r04_top_view_small_batches.txt: the fork / join and the extra launch cost ~13 us a step (39 / 51 / 53 / 60 / 102 / 341 us against the ring's 36 / 38 / 41 / 47 / 103 / 387 at 1 .. 4096 agents)"},
    /* kPartsMax              */ {"draw_parts_max", 4, "workgroups", "profiles/r05_draw_kernel.txt (tools/experiments.md: r05_draw_parts.sh): 1024^2 px x 64 agents 53.6 / 38.6 / 30.5 us with 1 / 2 / 4 parts"},
    /* kPartsMinRays          */ {"draw_part_min_rays", 128, "rays", "same table: a part's fixed costs (plane cleared, every end point, plane scanned) are most of a workgroup's life; x 256 agents 61.4 / 78.7 / 110"},
    /* kFillGBperMs           */ {"camera_fill_rate", 6.5e6, "B/us", "profiles/r05_kernel_stats.csv: rcw_fill256_kernel 156 us a GiB = 6.88 TB/s; 6.5 with its smaller siblings"},
    /* kFillLateStartUs       */ {"side_stream_late_start", 12, "us", "profiles/r05_top_view_shapes.txt / tools/step_timeline.sh: a kernel behind an event of the other stream starts ~13 us later than behind a kernel of its own (19 against 6 us after the cast kernel's end)"},
    /* kDrawUsPerGibFewRays   */ {"draw_floor_few_rays", 34, "us/GiB", "profiles/r05_draw_kernel.txt, r05_top_view_shapes.txt (a): the draw kernel's floor per GiB of top view with up to 256 rays (768^2 px x 455: 37 us)"},
    /* kDrawUsPerGibManyRays  */ {"draw_floor_many_rays", 55, "us/GiB", "same: beyond 256 rays (1024^2 px x 256, 1024 rays: 58-61 us)"},
    /* kDrawManyRays          */ {"draw_many_rays_from", 257, "rays", "the boundary between the two floors above"},
    /* kDrawPartialRound      */ {"draw_partial_round", 0.7, "", "profiles/r05_draw_kernel.txt (tools/experiments.md: r05_draw_first.sh): a partial round of draw workgroups takes about as long as a full one (768^2 px x 114 / 228 / 341 agents 90 -> 75, 129 -> 115, 169 -> 155 us)"},
    /* kDrawLdsCap            */ {"draw_kernel_lds_cap", 159 * 1024, "B", "rcw_top_split_unit / rcw_top_flat_cols: the draw kernel's plane + ray lists within the CU's LDS less 1 KiB"},
    /* kFillWavefrontsPerCu   */ {"fill_wavefronts_per_cu", 4, "wavefronts", "one workgroup of the camera fill (four wavefronts) sits on every CU: what is left of the CU's wavefront slots is the drawing's"},
};
constexpr double top_rule(TopRuleId id) { return kTopRules[id].value; }
}  // namespace

// what the rule decides (fields of RcwPlan), from the configuration, the batch, the device's numbers and the caller's wishes; no HIP call.
// want_form: 0 = the rule, or one of RCW_TOP_VIEW_IN_PLACE / ONE_KERNEL / TWO_KERNELS (rcw_set_top_view_form); want_runs: 0 = the rule, or 1..8.
// `lenient`: a form the geometry cannot take falls back to the rule (development switches) instead of failing.
int top_view_rule(RcwPlan& d, const rcw_config* cfg, size_t B, const RcwHw& hw, int want_form, int want_runs, bool lenient)
{
    const int H = cfg->height_tile_map_tu, W = cfg->width_tile_map_tu, N = cfg->num_rays, Hc = cfg->height_camera_view_pu;
    d.top_lds = 0; d.top_split = 0; d.top_flat = 0; d.top_plane_words = 0; d.top_unit_px = 256; d.top_runs = 1;
    d.top_alone_split = 0; d.top_fused = 0; d.top_grid = hw.cus; d.top_store_grid = d.fill_grid; d.top_store_plain = 0; d.top_draw_block = 256; d.top_draw_block_alone = 256; d.top_draw_first = 0; d.top_parts = 1;
    if (!cfg->render_top_view) {
        if (want_form != 0 && !lenient) return fail(RCW_ERR_UNSUPPORTED, "handle was created with render_top_view = 0");
        return RCW_OK;
    }
    const size_t ring_cap = (size_t)top_rule(kRingLdsCap);
    // the write-once kernel keeps a ring of 1..3 agents' bit planes in LDS: three where three workgroups per CU still fit beside
    // each other, else two, else one; larger images take the in-place kernel
    d.top_lds = 3;
    if (rcw_top_view_lds_bytes(d) > (size_t)top_rule(kRingThreeBuffersLds)) d.top_lds = 2;
    if (rcw_top_view_lds_bytes(d) > ring_cap) d.top_lds = 1;
    if (rcw_top_view_lds_bytes(d) > ring_cap) d.top_lds = 0;             // (the size depends on top_lds)
    if ((long long)H * cfg->pu_per_tu > (long long)top_rule(kLineWalkMaxPixels) || (long long)W * cfg->pu_per_tu > (long long)top_rule(kLineWalkMaxPixels)) d.top_lds = 0;
    if (const char* v = RCW_DEV_ENV("RCW_TOP_RING")) { const int k = std::atoi(v); if (k >= 1 && k <= 3 && d.top_lds > 0) { d.top_lds = k; if (rcw_top_view_lds_bytes(d) > ring_cap) d.top_lds = 1; } }
    if (want_form == RCW_TOP_VIEW_IN_PLACE) d.top_lds = 0;
    if (want_form == RCW_TOP_VIEW_ONE_KERNEL && !d.top_lds && !lenient)
        return fail(RCW_ERR_UNSUPPORTED, "the image's bit planes do not fit in LDS: this geometry takes the in-place form only");
    {   // persistent grid: as many 8-wavefront workgroups per CU as registers and LDS allow
        const size_t lds = rcw_top_view_lds_bytes(d);
        int per_cu = lds ? (int)((size_t)hw.lds_per_cu / lds) : 4;
        per_cu = per_cu < 1 ? 1 : (per_cu > (int)top_rule(kRingWorkgroupsPerCu) ? (int)top_rule(kRingWorkgroupsPerCu) : per_cu);
        d.top_grid = per_cu * hw.cus;
    }
    if (const char* v = RCW_DEV_ENV("RCW_TOP_GRID")) { const int g = std::atoi(v); if (g >= 1 && g <= 65536) d.top_grid = g; }
    if (const char* v = RCW_DEV_ENV("RCW_TOP_STORE_GRID")) { const int g = std::atoi(v); if (g >= 1 && g <= 65536) d.top_store_grid = g; }
    // The two-kernel form where the geometry allows it: the unit kernels (whole tiles in runs of 256 / 128 / 64 / 32 rows)
    // or the flat kernel (any pixel scale from 9, any image height that is a multiple of 4 from 42 rows)
    int unit = d.top_lds > 0 ? rcw_top_split_unit(d) : 0;
    const int flat = d.top_lds > 0 ? rcw_top_flat_cols(d) : 0;
    // (several units a chunk: the flat kernel is the faster one — 384² / 320² / 288² px images, µs per GiB: 181 / 194 / 207 with
    // 2 / 4 / 8 units against 176 / 175 / 173; whole 256-row chunks keep rcw_top_store_kernel: 159 against 179)
    if (flat && unit && unit < 256) unit = 0;
    if (const char* v = RCW_DEV_ENV("RCW_TOP_FLAT")) { const int f = std::atoi(v); if (f == 1 && flat) unit = 0; if (f == 0 && rcw_top_split_unit(d) && d.top_lds > 0) unit = rcw_top_split_unit(d); }
    const bool eligible = unit || flat;
    d.top_unit_px = unit ? unit : 256;
    d.top_flat = unit ? 0 : flat;
    d.top_plane_words = d.top_flat ? rcw_top_plane_words(d) : 0;
    // ... at every batch size where a step's camera fill and the drawing go in ONE launch (rcw_fill256_draw_kernel); where the drawing
    // needs the side stream (another camera height, planes beyond 64 KiB, runs of agents), only where the batch is big enough to pay for
    // the fork / join and the extra launch (kSideStreamMinBytes).  (Decided below, when the draw kernel's block and the runs are known.)
    d.top_split = eligible ? 1 : 0;
    if (want_form == RCW_TOP_VIEW_ONE_KERNEL || want_form == RCW_TOP_VIEW_IN_PLACE) d.top_split = 0;
    if (want_form == RCW_TOP_VIEW_TWO_KERNELS) {
        if (eligible) d.top_split = 1;
        else if (!lenient) return fail(RCW_ERR_UNSUPPORTED, "this geometry does not take the two-kernel form (pu_per_tu >= 8, image height a multiple of 4 and of at least 42 rows, bit plane within LDS)");
    }
    if (!d.top_split) { d.top_unit_px = 256; d.top_flat = 0; d.top_plane_words = 0; }
    // rcw_update_top_view alone has no camera fill to hide the drawing behind (kAloneTwoKernelsPixels, kAloneTwoKernelsBelowPu): draw ->
    // store back to back for images from 256 x 256 px, pixel scales that are no multiple of 4 and tiles below 16 px; the one-kernel form
    // keeps what is left of the two-kernel form's geometries — and every geometry the two-kernel form cannot take.
    {
        const long long px = (long long)H * cfg->pu_per_tu * W * cfg->pu_per_tu;
        d.top_alone_split = d.top_split && (px >= (long long)top_rule(kAloneTwoKernelsPixels) || (cfg->pu_per_tu & 3) != 0 || cfg->pu_per_tu < (int)top_rule(kAloneTwoKernelsBelowPu)) ? 1 : 0;
    }
    if (const char* v = RCW_DEV_ENV("RCW_TOP_ALONE_SPLIT")) d.top_alone_split = d.top_split && std::atoi(v) ? 1 : 0;
    // draw kernel: one workgroup of 4 wavefronts per agent; where the bit plane leaves room for one or two workgroups on a CU
    // (kDrawWideBlockLds), 8 to 16 wavefronts: a lane per ray for N > 256, two lanes a ray for fewer
    if (rcw_top_view_lds_bytes(d) / (d.top_lds > 0 ? d.top_lds : 1) > (size_t)top_rule(kDrawWideBlockLds)) {
        const int b = ((N + 255) / 256) * 256;
        d.top_draw_block = b < (int)top_rule(kDrawBlockMin) ? (int)top_rule(kDrawBlockMin) : (b > (int)top_rule(kDrawBlockMax) ? (int)top_rule(kDrawBlockMax) : b);
    }
    // ... and alone, with tens of thousands of small images, one or two wavefronts an agent (the set-up per wavefront is what such a batch costs)
    d.top_draw_block_alone = d.top_draw_block;
    if (d.top_draw_block == 256) d.top_draw_block_alone = B >= (size_t)top_rule(kAloneBlock64Agents) ? 64 : (B >= (size_t)top_rule(kAloneBlock128Agents) ? 128 : 256);
    if (const char* v = RCW_DEV_ENV("RCW_TOP_DRAW_BLOCK")) { const int b = std::atoi(v); if (b == 64 || b == 128 || b == 256 || b == 512 || b == 768 || b == 1024) d.top_draw_block = d.top_draw_block_alone = b; }
    // runs of agents: where the lines are long against the camera image's columns the drawing does not fit beside the camera fill; with
    // several GiB of top view a step, runs of >= 1 GiB let the rest of it hide beside the storing of earlier runs
    if ((long long)top_rule(kRunsLineToCameraDen) * ((long long)H + W) * cfg->pu_per_tu >= (long long)top_rule(kRunsLineToCameraNum) * Hc) {
        const size_t gib = (B * (size_t)H * W * cfg->pu_per_tu * cfg->pu_per_tu * sizeof(uint32_t)) >> 30;
        d.top_runs = gib >= (size_t)top_rule(kRuns4Gib) ? 4 : (gib >= (size_t)top_rule(kRuns2Gib) ? 2 : 1);
    }
    if (want_runs >= 1) d.top_runs = want_runs <= 8 ? (want_runs <= (int)B ? want_runs : (int)B) : 8;
    // a step's camera fill and the drawing in one launch where the geometry allows (256-row camera view, one run, planes of a
    // 256-thread draw workgroup): no side stream in the step
    d.top_fused = rcw_fill_draw_fusable(d) ? 1 : 0;
    if (const char* v = RCW_DEV_ENV("RCW_TOP_FUSED")) d.top_fused = d.top_fused && std::atoi(v) ? 1 : 0;
    if (d.top_split && !d.top_fused && want_form != RCW_TOP_VIEW_TWO_KERNELS &&
        (double)(B * (size_t)H * W * cfg->pu_per_tu * cfg->pu_per_tu * sizeof(uint32_t)) < top_rule(kSideStreamMinBytes)) {
        d.top_split = 0; d.top_unit_px = 256; d.top_flat = 0; d.top_plane_words = 0; d.top_alone_split = 0;
    }
    // Several draw workgroups an agent (rcw_top_draw_kernel: each walks a part of the fan and ORs its plane into the agent's) where a batch
    // of big images leaves draw slots empty: as many parts as fill them (kPartsMax, kPartsMinRays).  Only with rcw_top_store_kernel, which
    // reads every plane word exactly once and leaves the zero the next drawing needs.
    const int draw_per_cu = rcw_top_draw_per_cu(d, d.top_draw_block, hw.lds_per_cu, hw.waves_per_cu - (int)top_rule(kFillWavefrontsPerCu));
    d.top_parts = 1;
    if (d.top_split && !d.top_flat && d.top_unit_px == 256 && !d.top_fused) {
        const long long slots = (long long)hw.cus * draw_per_cu;
        int parts = (int)std::min<long long>((long long)top_rule(kPartsMax), slots / (long long)B);
        while (parts > 1 && N / parts < (int)top_rule(kPartsMinRays)) --parts;
        d.top_parts = parts < 1 ? 1 : parts;
        if (const char* v = RCW_DEV_ENV("RCW_TOP_PARTS")) { const int q = std::atoi(v); if (q >= 1 && q <= 4 && N / q >= 16) d.top_parts = q; }
    }
    // The drawing first on the handle's stream and the camera fill on the side stream (launch_top_view) where the fill is the SHORTER of the
    // two: it then ends before the store kernel starts (where it is the longer one it runs into the store kernel — two moving windows on one
    // HBM — and the step takes up to 60 % longer).  Both are estimated from the sizes: the fill at kFillGBperMs plus its late start, the
    // drawing at its measured floor per GiB of top view — of the batch or, for a small one, of most of one round of workgroups.
    {
        const double fill_us = (double)B * N * Hc * 4.0 / top_rule(kFillGBperMs) + top_rule(kFillLateStartUs);
        const double image_gib = (double)H * W * cfg->pu_per_tu * cfg->pu_per_tu * 4.0 / (double)(1u << 30);
        const double round_gib = (double)hw.cus * draw_per_cu * image_gib;
        const double top_gib = std::max((double)B * image_gib, top_rule(kDrawPartialRound) * round_gib);
        const double draw_us = top_gib * (N >= (int)top_rule(kDrawManyRays) ? top_rule(kDrawUsPerGibManyRays) : top_rule(kDrawUsPerGibFewRays));
        d.top_draw_first = d.top_split && !d.top_fused && d.top_runs <= 1 && fill_us <= draw_us ? 1 : 0;
    }
    if (const char* v = RCW_DEV_ENV("RCW_TOP_DRAW_FIRST")) d.top_draw_first = d.top_split && !d.top_fused && std::atoi(v) ? 1 : 0;
    if (const char* v = RCW_DEV_ENV("RCW_TOP_STORE_PLAIN")) d.top_store_plain = std::atoi(v) ? 1 : 0;
    return RCW_OK;
}

// the RCW_TOP_VIEW_* name of the form a plan takes inside a step, and of rcw_update_top_view alone
int top_form_alone(const RcwPlan& d, bool split) { return !d.top_view ? RCW_TOP_VIEW_NONE : split ? RCW_TOP_VIEW_TWO_KERNELS : d.top_lds ? RCW_TOP_VIEW_ONE_KERNEL : RCW_TOP_VIEW_IN_PLACE; }
int top_form_alone(const RcwPlan& d) { return top_form_alone(d, d.top_split && d.top_alone_split); }
int top_form_in_step(const RcwPlan& d) { return top_form_alone(d, d.top_split != 0); }

// The one-launch step pays where the fill outlasts the casting half's own life: one casting workgroup marches FIVE fans one after the
// other, so a small batch waits for it (4096 x 256 columns: 17 us of casting life under a 154 us fill; 64 agents: 22 us a step against
// 12 for cast kernel + fill).  Measured crossovers (profiles/r06_small_batches.txt, frames of a step): 8x8 map, 256 columns ~128 MiB;
// 16x16, 512 columns ~100 MiB; 32x32, 1024 columns ~350 MiB; 8x8, 64 columns below 64 MiB — the casting life fits
// kStepCastBaseUs + kStepCastUsPerUnit x (view columns a lane x 5 fans x (H + W) tiles a ray may cross), the fill kFillGBperMs.
constexpr double kStepCastBaseUs = 4.5, kStepCastUsPerUnit = 0.045;
bool step_one_launch_pays(const RcwDev& d)
{
    const int lanes = d.N <= 256 ? 64 : 256;                                // a wavefront per agent up to 256 view columns, a workgroup beyond
    const double units = (double)((d.N + lanes - 1) / lanes) * 5.0 * (double)(d.H + d.W);
    const double cast_us = kStepCastBaseUs + kStepCastUsPerUnit * units;
    const double fill_us = (double)d.B * d.N * d.Hc * 4.0 / top_rule(kFillGBperMs);
    return fill_us >= cast_us;
}

// rcw_set_walls' refusals (include/rcw.h, "wall layouts") as a pure host function — no handle, no device: the development build exports it
// (rcw_dev_validate_walls).  0, or RCW_ERR_INVALID_ARGUMENT with the reason, naming the layout and the tile, in msg.  EVERY layout handed
// over is checked, also one no agent of the mask takes: a ring tile that is no wall lets a march leave the map (stage_tile_bytes, the guard
// bands of cast_ray_guarded), and a later call may well index it.
int validate_walls(int H, int W, int B, const uint8_t* walls, int layouts, const int32_t* index, const uint8_t* mask, char* msg, size_t cap)
{
    if (!walls) { std::snprintf(msg, cap, "NULL walls"); return RCW_ERR_INVALID_ARGUMENT; }
    if (layouts < 1) { std::snprintf(msg, cap, "layouts must be >= 1 (got %d)", layouts); return RCW_ERR_INVALID_ARGUMENT; }
    if (!index && layouts != 1 && layouts != B) {
        std::snprintf(msg, cap, "a NULL layout index needs 1 layout or one per agent (%d); got %d layouts", B, layouts);
        return RCW_ERR_INVALID_ARGUMENT;
    }
    for (int a = 0; index && a < B; ++a) {
        if (mask && !mask[a]) continue;
        if (index[a] < 0 || index[a] >= layouts) {
            std::snprintf(msg, cap, "agent %d: layout index %d not in 0..%d", a, index[a], layouts - 1);
            return RCW_ERR_INVALID_ARGUMENT;
        }
    }
    for (int m = 0; m < layouts; ++m) {
        const uint8_t* const q = walls + (size_t)m * (size_t)H * (size_t)W;
        int free_tiles = 0;
        for (int j = 1; j <= W; ++j)
            for (int i = 1; i <= H; ++i) {
                const bool wall = q[(i - 1) + (size_t)H * (j - 1)] != 0;
                const bool ring = i == 1 || i == H || j == 1 || j == W;                   // SR:57-60
                if (ring && !wall) {
                    std::snprintf(msg, cap, "layout %d: ring tile (%d,%d) is not a wall (the ring ends every ray)", m, i, j);
                    return RCW_ERR_INVALID_ARGUMENT;
                }
                if (!ring && !wall) ++free_tiles;
            }
        if (free_tiles < 2) {
            std::snprintf(msg, cap, "layout %d: %d free interior tile(s), a goal and a player need two", m, free_tiles);
            return RCW_ERR_INVALID_ARGUMENT;
        }
    }
    return RCW_OK;
}

int validate_config(const rcw_config* c, int32_t batch)
{
    if (c->abi_version != RCW_ABI_VERSION)
        return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_config.abi_version %d != %d", c->abi_version, RCW_ABI_VERSION);
    if (batch < 1) return fail(RCW_ERR_INVALID_ARGUMENT, "batch must be >= 1 (got %d)", batch);
    if (c->height_tile_map_tu < 3 || c->width_tile_map_tu < 3)
        return fail(RCW_ERR_INVALID_ARGUMENT, "tile map must be at least 3x3 (got %dx%d)",
                    c->height_tile_map_tu, c->width_tile_map_tu);
    // the cast kernel stages a byte per tile in dynamic LDS next to a few static words: 64 KiB per workgroup in all
    if ((long long)c->height_tile_map_tu * c->width_tile_map_tu + 2ll * c->height_tile_map_tu > 65536 - 256)   // (+ the cast kernel's two guard bands of H bytes)
        return fail(RCW_ERR_UNSUPPORTED, "tile map larger than 65280 tiles does not fit the LDS staging");
    if (c->num_directions < 1 || c->num_rays < 1 || c->height_camera_view_pu < 1)
        return fail(RCW_ERR_INVALID_ARGUMENT, "num_directions, num_rays, height_camera_view_pu must be >= 1");
    if (c->num_rays > (1 << 24)) return fail(RCW_ERR_INVALID_ARGUMENT, "num_rays not exactly representable in Float32");
    if (c->num_directions > (1 << 20) || (long long)c->num_directions * c->num_rays > (1ll << 24))
        return fail(RCW_ERR_UNSUPPORTED, "num_directions * num_rays = %lld: the (direction, ray) table is limited to 2^24 entries",
                    (long long)c->num_directions * c->num_rays);
    if (c->height_camera_view_pu > (1 << 20))
        return fail(RCW_ERR_UNSUPPORTED, "height_camera_view_pu larger than 2^20");
    if (c->reward_type < RCW_REWARD_FLOAT32 || c->reward_type > RCW_REWARD_INT64)
        return fail(RCW_ERR_INVALID_ARGUMENT, "reward_type must be one of RCW_REWARD_* (got %d)", c->reward_type);
    if (!std::isfinite(c->goal_reward) || !std::isfinite(c->goal_reward_f64))
        return fail(RCW_ERR_INVALID_ARGUMENT, "goal_reward must be finite");
    if ((c->reward_type == RCW_REWARD_INT32 || c->reward_type == RCW_REWARD_INT64) &&
        (c->goal_reward_f64 != std::floor(c->goal_reward_f64) || std::fabs(c->goal_reward_f64) > 2147483647.0))
        return fail(RCW_ERR_INVALID_ARGUMENT, "goal_reward_f64 = %g is not an integer the reward type holds", c->goal_reward_f64);
    if (c->world_unit_bits != 32 && c->world_unit_bits != 64)
        return fail(RCW_ERR_INVALID_ARGUMENT, "world_unit_bits must be 32 or 64 (got %d)", c->world_unit_bits);
    if (c->world_unit_bits == 64) {
        if (!(c->player_radius_wu_f64 > 0.0 && c->player_radius_wu_f64 < 0.5))
            return fail(RCW_ERR_INVALID_ARGUMENT, "player_radius_wu_f64 must be in (0, 0.5)");
        if (!(c->position_increment_wu_f64 > 0.0) || !std::isfinite(c->position_increment_wu_f64) ||
            !(c->semi_field_of_view_wu_f64 > 0.0) || !std::isfinite(c->semi_field_of_view_wu_f64) ||
            !(c->camera_height_tile_wu_f64 > 0.0) || !std::isfinite(c->camera_height_tile_wu_f64))
            return fail(RCW_ERR_INVALID_ARGUMENT, "the *_f64 world-unit parameters must be positive and finite");
    }
    if (!(c->player_radius_wu > 0.0f && c->player_radius_wu < 0.5f))   // "should be less than 0.5" SR:47
        return fail(RCW_ERR_INVALID_ARGUMENT, "player_radius_wu must be in (0, 0.5)");
    if (!(c->position_increment_wu > 0.0f) || !std::isfinite(c->position_increment_wu))
        return fail(RCW_ERR_INVALID_ARGUMENT, "position_increment_wu must be positive and finite");
    if (!(c->semi_field_of_view_wu > 0.0f) || !std::isfinite(c->semi_field_of_view_wu))
        return fail(RCW_ERR_INVALID_ARGUMENT, "semi_field_of_view_wu must be positive and finite");
    if (c->render_top_view && (c->pu_per_tu < 1 || c->pu_per_tu > 4096))
        return fail(RCW_ERR_INVALID_ARGUMENT, "pu_per_tu must be in 1..4096 for the top view");
    if (!(c->camera_height_tile_wu > 0.0f) || !std::isfinite(c->camera_height_tile_wu))
        return fail(RCW_ERR_INVALID_ARGUMENT, "camera_height_tile_wu must be positive and finite");
    if (c->dda_tie_break < 0 || c->dda_tie_break > 1 || c->dda_distance < 0 || c->dda_distance > 1 ||
        c->normalize_mode < 0 || c->normalize_mode > 1 || c->out_of_bounds < 0 || c->out_of_bounds > 1)
        return fail(RCW_ERR_INVALID_ARGUMENT, "dda_tie_break / dda_distance / normalize_mode / out_of_bounds out of range");
    return RCW_OK;
}

namespace {
// the channels of a format: its colour's, then the depth plane's
int view_channels(int32_t format) { return ((format & 3) == RCW_VIEW_RGB8 ? 3 : (format & 3) == RCW_VIEW_GRAY8 ? 1 : 0) + (format & RCW_VIEW_DEPTH8 ? 1 : 0); }
}  // namespace

// What rcw_set_learner_view_stack's arguments ask of this geometry (ViewPlan, rcw_handle.h), or the refusal
int plan_learner_view(const rcw_config& cfg, const RcwDev& dev, int32_t format, int32_t layout, int32_t height, int32_t width, int32_t flags,
                      int32_t frames, ViewPlan* plan)
{
    const int Hc = cfg.height_camera_view_pu, N = cfg.num_rays;
    if (format < RCW_VIEW_OFF || format > RCW_VIEW_GRAYD8 || format == (RCW_VIEW_RGB8 | RCW_VIEW_GRAY8))
        return fail(RCW_ERR_INVALID_ARGUMENT, "format must be RCW_VIEW_OFF / RCW_VIEW_RGB8 / RCW_VIEW_GRAY8 / RCW_VIEW_DEPTH8 / RCW_VIEW_RGBD8 / RCW_VIEW_GRAYD8 (got %d)", format);
    if (flags & ~RCW_VIEW_ONLY) return fail(RCW_ERR_INVALID_ARGUMENT, "unknown learner view flags 0x%x", (unsigned)flags);
    if (format == RCW_VIEW_OFF && flags) return fail(RCW_ERR_INVALID_ARGUMENT, "RCW_VIEW_ONLY needs a format");
    if (frames < 1 || frames > RCW_VIEW_MAX_FRAMES)
        return fail(RCW_ERR_INVALID_ARGUMENT, "frames must be in 1..%d (got %d)", RCW_VIEW_MAX_FRAMES, frames);
    if (format == RCW_VIEW_OFF) return RCW_OK;
    if (layout != RCW_VIEW_CHW && layout != RCW_VIEW_HWC)
        return fail(RCW_ERR_INVALID_ARGUMENT, "layout must be RCW_VIEW_CHW or RCW_VIEW_HWC (got %d)", layout);
    if (height < 1 || height > Hc || width < 1 || width > N)
        return fail(RCW_ERR_INVALID_ARGUMENT, "learner view size %d x %d outside 1..%d x 1..%d (no up-sampling)", height, width, Hc, N);
    if (frames > 1 && (long long)view_channels(format) * height * width >= (1ll << 31))
        return fail(RCW_ERR_UNSUPPORTED, "a stack of frames of 2 GiB or more");
    if (frames > 1 && layout != RCW_VIEW_CHW)
        return fail(RCW_ERR_UNSUPPORTED, "a stack of %d frames needs RCW_VIEW_CHW (slot s is channels [s C, (s + 1) C))", frames);
    RcwView& v = plan->v;
    v.C = view_channels(format);
    v.depth = format & RCW_VIEW_DEPTH8 ? 1 : 0;
    v.hwc = layout == RCW_VIEW_HWC ? 1 : 0;
    v.h = height; v.w = width;
    std::vector<int32_t>& t = plan->tab;
    try { t.resize((size_t)height + width + 2 + (v.depth ? (size_t)Hc + 1 : 0)); } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation failed"); }
    long long max_rows = 0, max_cols = 0;
    for (int r = 0; r <= height; ++r) t[r] = (int32_t)((long long)r * Hc / height);
    for (int c = 0; c <= width; ++c) t[(size_t)height + 1 + c] = (int32_t)((long long)c * N / width);
    for (int r = 0; r < height; ++r) max_rows = std::max<long long>(max_rows, t[r + 1] - t[r]);
    for (int c = 0; c < width; ++c) max_cols = std::max<long long>(max_cols, t[(size_t)height + 2 + c] - t[(size_t)height + 1 + c]);
    const long long n = max_rows * max_cols;
    v.wide = n * 256 + n >= (1ll << 31) ? 1 : 0;          // (a box's channel sum + n/2 must stay below 2^31 for 32-bit sums)
    v.full_ok = height == Hc && width == N && rcw_view_full_eligible(dev, v.C, v.hwc) ? 1 : 0;
    if (v.depth) {
        // the ceiling / floor depth byte De(y) = (255 u + Hc/2) / Hc, u = Hc - 2 min(y, Hc - 1 - y) (include/rcw.h), summed over rows [0, y):
        // at most 255 * 2^20
        int32_t* const ds = t.data() + (size_t)height + width + 2;
        ds[0] = 0;
        for (int y = 0; y < Hc; ++y) ds[y + 1] = ds[y] + (int32_t)((255ll * (Hc - 2 * std::min(y, Hc - 1 - y)) + Hc / 2) / Hc);
    }
    return RCW_OK;
}

// What rcw_set_local_map's arguments ask for, or the refusal; source != 0: the offset table off[k] = (T)(2k + 1 - S) / (T)(2r), k = 0..S-1, in
// the handle's world-unit type T — one correctly rounded division of two exactly representable integers (|2k + 1 - S| < 128, 2r <= 32) —
// as the bytes to upload.
int plan_local_map(int32_t source, int32_t size, int32_t cells_per_tile, bool real64, std::vector<unsigned char>* table)
{
    if (source != 0 && source != RCW_LOCAL_WORLD && source != RCW_LOCAL_SEEN)
        return fail(RCW_ERR_INVALID_ARGUMENT, "source must be 0 (off), RCW_LOCAL_WORLD or RCW_LOCAL_SEEN (got %d)", source);
    if (source == 0) return RCW_OK;
    if (size < 1 || size > RCW_LOCAL_MAX_SIZE)
        return fail(RCW_ERR_INVALID_ARGUMENT, "local map size must be in 1..%d (got %d)", RCW_LOCAL_MAX_SIZE, size);
    if (cells_per_tile < 1 || cells_per_tile > RCW_LOCAL_MAX_CELLS_PER_TILE)
        return fail(RCW_ERR_INVALID_ARGUMENT, "cells_per_tile must be in 1..%d (got %d)", RCW_LOCAL_MAX_CELLS_PER_TILE, cells_per_tile);
    try { table->resize((size_t)size * (real64 ? sizeof(double) : sizeof(float))); } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation failed"); }
    for (int k = 0; k < size; ++k) {
        if (real64) { const double v = (double)(2 * k + 1 - size) / (double)(2 * cells_per_tile); std::memcpy(table->data() + (size_t)k * sizeof v, &v, sizeof v); }
        else { const float v = (float)(2 * k + 1 - size) / (float)(2 * cells_per_tile); std::memcpy(table->data() + (size_t)k * sizeof v, &v, sizeof v); }
    }
    return RCW_OK;
}

// The wall bank's weights (include/rcw.h, "the wall bank") as the kernel reads them: cum[k] = w[0] + ... + w[k] (NULL: every weight 1), and
// their sum, which must lie in 1 .. 2^32 - 1 — or the refusal.
int plan_wall_bank_weights(const uint32_t* weights, int32_t layouts, uint32_t* cum, uint64_t* total)
{
    uint64_t sum = 0;
    for (int32_t k = 0; k < layouts; ++k) {
        sum += weights ? (uint64_t)weights[k] : 1u;
        if (sum > 0xFFFFFFFFull) return fail(RCW_ERR_INVALID_ARGUMENT, "the wall bank's weights sum to more than 2^32 - 1 (at layout %d)", k);
        cum[k] = (uint32_t)sum;
    }
    if (sum == 0) return fail(RCW_ERR_INVALID_ARGUMENT, "the wall bank's weights sum to zero: no layout could be drawn");
    *total = sum;
    return RCW_OK;
}

// ---- the wall generator (include/rcw.h, "the wall generator") ---------------------------------------------------------------------------
// The level range of a generator family (the maze, the caves and the rooms share the rule): levels of first_level .. first_level + levels - 1,
// Int32 all of them — or the refusal, in the family's words.
static bool level_range_ok(int32_t levels, int32_t first_level) { return levels >= 0 && first_level >= 0 && (int64_t)first_level + (int64_t)levels <= 2147483647ll; }
static int check_level_range(const char* whose, int32_t levels, int32_t first_level)
{
    if (level_range_ok(levels, first_level)) return RCW_OK;
    return fail(RCW_ERR_INVALID_ARGUMENT, "%s level range must satisfy levels >= 0, first_level >= 0 and first_level + levels <= 2^31 - 1 (got first_level %d, levels %d)", whose, first_level, levels);
}

// What rcw_set_wall_generator checks of a geometry and a level range before anything is queued — or the refusal.
int plan_wall_generator(int32_t H, int32_t W, int32_t levels, int32_t first_level)
{
    if (H < 5 || W < 5) return fail(RCW_ERR_INVALID_ARGUMENT, "the wall generator needs a map of at least 5 x 5 tiles (this one is %d x %d)", H, W);
    if (const int rc = check_level_range("the wall generator's", levels, first_level)) return rc;
    const int64_t cells = (int64_t)((H - 1) / 2) * (int64_t)((W - 1) / 2);
    if (cells > kWallGenMaxCells)
        return fail(RCW_ERR_UNSUPPORTED, "the wall generator makes mazes of at most %d cells (maps up to 129 x 129); %d x %d has %lld", kWallGenMaxCells, H, W, (long long)cells);
    return RCW_OK;
}

// The two handle-less exports: the rule once more on the host, for replay and evaluation — and, inside the library, a second implementation
// beside the device's Boruvka: plain Kruskal, the edges sorted by their order words, union-find with path halving.
extern "C" int rcw_wall_generator_key(uint64_t seed, int32_t global_agent, uint32_t episode, int32_t levels, int32_t first_level, uint64_t level_seed,
                                      uint64_t* maze_key, int32_t* level)
{
    if (global_agent < 0 || !level_range_ok(levels, first_level))
        return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_wall_generator_key: global_agent >= 0, levels >= 0, first_level >= 0 and first_level + levels <= 2^31 - 1 are required");
    const uint64_t u = rcw_draw(rcw_episode_key(seed, (uint64_t)global_agent, (uint64_t)episode), 0x8000000000000000ull);
    int32_t l = -1;
    uint64_t m = u;
    if (levels > 0) {
        l = first_level + (int32_t)rcw_below(u, (uint64_t)levels);
        m = rcw_episode_key(level_seed, (uint64_t)l, 0ull);
    }
    if (maze_key) *maze_key = m;
    if (level) *level = l;
    return RCW_OK;
}

extern "C" int rcw_wall_generator_layout(int32_t H, int32_t W, uint64_t maze_key, uint32_t loops, uint8_t* out_host)
{
    if (!out_host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (H < 5 || W < 5) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_wall_generator_layout: a maze needs at least 5 x 5 tiles (got %d x %d)", H, W);
    const int64_t ni = (H - 1) / 2, nj = (W - 1) / 2, C = ni * nj;
    if (2 * C >= (1ll << 20)) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_wall_generator_layout: edge ids must stay below 2^20 (%d x %d has %lld cells)", H, W, (long long)C);
    std::vector<uint64_t> order;
    std::vector<uint32_t> parent;
    try { order.reserve((size_t)(2 * C)); parent.resize((size_t)C); } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the maze's edges failed"); }
    std::memset(out_host, 1, (size_t)H * (size_t)W);
    auto open = [&](int64_t i, int64_t j) { out_host[(size_t)(i + (int64_t)H * j)] = 0; };   // tile (i, j), 0-based, in rcw_set_walls' order
    auto passage = [&](uint64_t id) {
        const int64_t c = (int64_t)(id >> 1), ci = c / nj, cj = c % nj;
        if (id & 1) open(2 * ci + 2, 2 * cj + 1); else open(2 * ci + 1, 2 * cj + 2);
    };
    for (int64_t c = 0; c < C; ++c) {
        const int64_t ci = c / nj, cj = c % nj;
        parent[(size_t)c] = (uint32_t)c;
        open(2 * ci + 1, 2 * cj + 1);
        for (uint64_t id = 2 * (uint64_t)c; id < 2 * (uint64_t)c + 2; ++id) {
            if ((id & 1) ? ci + 1 >= ni : cj + 1 >= nj) continue;
            order.push_back((rcw_draw(maze_key, id) & 0xFFFFFFFFFFF00000ull) | id);
            if ((uint32_t)(rcw_draw(maze_key, 2 * (uint64_t)C + id) >> 32) < loops) passage(id);   // (a tree edge too: it is opened either way)
        }
    }
    std::sort(order.begin(), order.end());
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (const uint64_t w : order) {
        const uint64_t id = w & 0xFFFFFull;
        const uint32_t c = (uint32_t)(id >> 1), d = c + ((id & 1) ? (uint32_t)nj : 1u);
        const uint32_t rc = find(c), rd = find(d);
        if (rc == rd) continue;
        parent[rc] = rd;
        passage(id);
    }
    return RCW_OK;
}

// ---- the wall generator: caves (include/rcw.h, "the wall generator: caves") ------------------------------------------------------------
// What rcw_set_wall_caves checks of a geometry, the smoothing count and a level range before anything is queued — or the refusal.
int plan_wall_caves(int32_t H, int32_t W, int32_t smooth, int32_t levels, int32_t first_level)
{
    if (H < 5 || W < 5) return fail(RCW_ERR_INVALID_ARGUMENT, "caves need a map of at least 5 x 5 tiles (this one is %d x %d)", H, W);
    if (smooth < 0 || smooth > kWallCavesMaxSmooth) return fail(RCW_ERR_INVALID_ARGUMENT, "caves are smoothed 0 .. %d times (got %d)", kWallCavesMaxSmooth, smooth);
    if (const int rc = check_level_range("the caves'", levels, first_level)) return rc;
    const int64_t tiles = (int64_t)(H - 2) * (int64_t)(W - 2);
    if (tiles > kWallCavesMaxTiles)
        return fail(RCW_ERR_UNSUPPORTED, "caves are made on at most %d interior tiles (maps up to 66 x 66); %d x %d has %lld", kWallCavesMaxTiles, H, W, (long long)tiles);
    return RCW_OK;
}

// The handle-less export: the rule once more on the host, by other algorithms than the device's — a queue flood fill a region where the kernel
// propagates labels, and rcw_wall_generator_layout's Kruskal for the fallback.
extern "C" int rcw_wall_caves_layout(int32_t H, int32_t W, uint64_t key, uint32_t fill, int32_t smooth, uint8_t* out_host, int32_t* fell_back)
{
    if (!out_host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const int rc = plan_wall_caves(H, W, smooth, 0, 0); if (rc) return rc;
    const size_t HW = (size_t)H * (size_t)W;
    std::vector<uint8_t> gen, nxt;
    std::vector<int32_t> region, queue;
    try { gen.assign(HW, 1); nxt.assign(HW, 1); region.assign(HW, -1); queue.reserve(HW); } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the cave failed"); }
    for (int j = 1; j + 1 < W; ++j)
        for (int i = 1; i + 1 < H; ++i) {
            const size_t t = (size_t)i + (size_t)H * (size_t)j;
            gen[t] = (uint32_t)(rcw_draw(key, 0x4000000000000000ull + (uint64_t)t) >> 32) < fill ? 1 : 0;
        }
    for (int s = 0; s < smooth; ++s) {
        for (int j = 1; j + 1 < W; ++j)
            for (int i = 1; i + 1 < H; ++i) {
                int walls = 0;
                for (int dj = -1; dj <= 1; ++dj)
                    for (int di = -1; di <= 1; ++di) walls += gen[(size_t)(i + di) + (size_t)H * (size_t)(j + dj)];
                nxt[(size_t)i + (size_t)H * (size_t)j] = walls >= 5 ? 1 : 0;
            }
        gen.swap(nxt);
    }
    // regions in the order of their smallest tile: a later one replaces the kept one only where it is strictly larger
    int32_t kept = -1, kept_size = 0, regions = 0;
    for (size_t t0 = 0; t0 < HW; ++t0) {
        if (gen[t0] || region[t0] >= 0) continue;
        const int32_t id = regions++;
        queue.clear(); queue.push_back((int32_t)t0); region[t0] = id;
        for (size_t head = 0; head < queue.size(); ++head) {
            const int32_t t = queue[head];
            const int32_t nb[4] = {t - 1, t + 1, t - H, t + H};            // (a free tile is interior: all four exist)
            for (const int32_t u : nb)
                if (!gen[(size_t)u] && region[(size_t)u] < 0) { region[(size_t)u] = id; queue.push_back(u); }
        }
        if ((int32_t)queue.size() > kept_size) { kept = id; kept_size = (int32_t)queue.size(); }
    }
    const int32_t need = std::max<int32_t>(7, (H - 2) * (W - 2) / 4);
    if (fell_back) *fell_back = kept_size < need ? 1 : 0;
    if (kept_size < need) return rcw_wall_generator_layout(H, W, key, 0u, out_host);
    for (size_t t = 0; t < HW; ++t) out_host[t] = region[t] == kept ? 0 : 1;
    return RCW_OK;
}

// ---- the wall generator: rooms (include/rcw.h, "the wall generator: rooms") ------------------------------------------------------------
// What rcw_set_wall_rooms checks of a geometry, the least room side and a level range before anything is queued — or the refusal.
int plan_wall_rooms(int32_t H, int32_t W, int32_t room, int32_t levels, int32_t first_level)
{
    if (H < 5 || W < 5) return fail(RCW_ERR_INVALID_ARGUMENT, "rooms need a map of at least 5 x 5 tiles (this one is %d x %d)", H, W);
    if (room < 1) return fail(RCW_ERR_INVALID_ARGUMENT, "a room's least side must be at least 1 tile (got %d)", room);
    if (const int rc = check_level_range("the rooms'", levels, first_level)) return rc;
    const long long bound = rcw_wall_rooms_bound(H, W), tiles = (long long)H * (long long)W;
    if (bound > kWallRoomsMaxRooms)
        return fail(RCW_ERR_UNSUPPORTED, "rooms are made on maps of at most %d odd-odd interior tiles, ceil((H - 2) / 2) ceil((W - 2) / 2) (up to 130 x 130 or 5 x 4097); %d x %d has %lld", kWallRoomsMaxRooms, H, W, bound);
    if (tiles > kWallRoomsMaxTiles)
        return fail(RCW_ERR_UNSUPPORTED, "rooms are made on maps of at most %d tiles; %d x %d has %lld", kWallRoomsMaxTiles, H, W, tiles);
    return RCW_OK;
}

// The level rows of the episode statistics' table (include/rcw.h, "episode statistics"), from the live layout source as of enabling: the bank
// a row per layout from 0, a generator family with a level range a row per level from first_level, anything else — and any count above
// RCW_EPISODE_STATS_MAX_ROWS — none: row 0 always works.
void plan_episode_stats_rows(RcwLayoutKind kind, int32_t layouts, int32_t levels, int32_t first_level, int32_t* rows, int32_t* first)
{
    const bool bank = kind == kLayoutBank, family = kind != kLayoutNone && !bank;
    const int32_t count = bank ? layouts : (family ? levels : 0);
    const bool any = count > 0 && count <= RCW_EPISODE_STATS_MAX_ROWS;
    *rows = any ? count : 0;
    *first = any && family ? first_level : 0;
}

// ---- the visit map (include/rcw.h, "the visit map") ---------------------------------------------------------------------------------------
// The table's level rows: episode statistics' rule from the shape's layout source — and none where the table, UInt32 (cells, 1 + rows),
// would pass RCW_VISIT_TABLE_MAX_BYTES (no error: row 0 always works).  64-bit arithmetic: cells < 2^35, 1 + rows < 2^32.
void plan_visit_table_rows(const SnapshotShape& sh, int32_t* rows, int32_t* first)
{
    plan_episode_stats_rows((RcwLayoutKind)sh.source_kind, sh.layouts, sh.levels, sh.first_level, rows, first);
    const uint64_t cells = (uint64_t)(uint32_t)sh.visit_sectors * (uint64_t)(uint32_t)sh.H * (uint64_t)(uint32_t)sh.W;
    if (cells * (1 + (uint64_t)(uint32_t)*rows) * sizeof(uint32_t) > (uint64_t)RCW_VISIT_TABLE_MAX_BYTES) { *rows = 0; *first = 0; }
}

namespace {
// The tile of (x, y) in the world-unit type T: i + H*j with (i, j) = (floor x, floor y), -1: not finite or off the map.
template <typename T>
int32_t visit_tile(int32_t H, int32_t W, T x, T y)
{
    if (!std::isfinite(x) || !std::isfinite(y)) return -1;
    const T fx = std::floor(x), fy = std::floor(y);
    if (fx < (T)0 || fx >= (T)H || fy < (T)0 || fy >= (T)W) return -1;
    return (int32_t)fx + H * (int32_t)fy;
}
}  // namespace

// The handle-less export: the cell rule for one agent on the host, needs no device.
extern "C" int rcw_visit_cell(int32_t H, int32_t W, int32_t nd, int32_t sectors, double x, double y, int32_t world_unit_bits, int32_t direction, int32_t* cell)
{
    if (!cell) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (H < 1 || W < 1 || (int64_t)H * W > INT32_MAX / RCW_VISIT_MAX_SECTORS) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_visit_cell: a map of %d x %d", H, W);
    if (world_unit_bits != 32 && world_unit_bits != 64) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_visit_cell: world_unit_bits must be 32 or 64 (got %d)", world_unit_bits);
    if (nd < 1 || direction < 0 || direction >= nd) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_visit_cell: direction %d of %d", direction, nd);
    if (sectors < 1 || sectors > RCW_VISIT_MAX_SECTORS || sectors > nd) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_visit_cell: sectors must be in 1..min(%d, nd = %d) (got %d)", RCW_VISIT_MAX_SECTORS, nd, sectors);
    const int32_t t = world_unit_bits == 64 ? visit_tile<double>(H, W, x, y) : visit_tile<float>(H, W, (float)x, (float)y);
    *cell = t < 0 ? -1 : (int32_t)(((int64_t)direction * sectors) / nd) * (H * W) + t;
    return RCW_OK;
}

// The handle-less export: the rule once more on the host, by another traversal than the device's — depth first off a plain stack, a chamber
// at a time, where the kernel cuts every chamber of a depth in one round.
extern "C" int rcw_wall_rooms_layout(int32_t H, int32_t W, uint64_t key, int32_t room, uint32_t stop, uint32_t doors, uint8_t* out_host, int32_t* rooms)
{
    if (!out_host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const int rc = plan_wall_rooms(H, W, room, 0, 0); if (rc) return rc;
    struct Chamber { int32_t i0, i1, j0, j1; };
    std::vector<Chamber> stack;
    try { stack.reserve(64); } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the rooms failed"); }
    for (int j = 0; j < W; ++j)
        for (int i = 0; i < H; ++i) out_host[(size_t)i + (size_t)H * (size_t)j] = (i == 0 || i == H - 1 || j == 0 || j == W - 1) ? 1 : 0;
    const int64_t least = std::min<int64_t>(room, kWallRoomsMaxTiles);   // (no side reaches it)
    const auto evens = [](int64_t lo, int64_t hi, int32_t* first) -> int32_t {   // the even numbers of lo .. hi
        const int64_t f = lo + (lo & 1);
        *first = (int32_t)f;
        return f > hi ? 0 : (int32_t)((hi - f) / 2 + 1);
    };
    int32_t count = 0;
    stack.push_back(Chamber{1, H - 2, 1, W - 2});
    while (!stack.empty()) {
        const Chamber c = stack.back();
        stack.pop_back();
        const bool root = c.i0 == 1 && c.j0 == 1 && c.i1 == H - 2 && c.j1 == W - 2;
        int32_t r0 = 0, c0 = 0;
        const int32_t nr = c.j1 > c.j0 ? evens(c.i0 + least, c.i1 - least, &r0) : 0;
        const int32_t nc = c.i1 > c.i0 ? evens(c.j0 + least, c.j1 - least, &c0) : 0;
        const uint64_t t0 = (uint64_t)(c.i0 + H * c.j0), t1 = (uint64_t)(c.i1 + H * c.j1);
        const uint64_t d = 0x2000000000000000ull + 8ull * ((t0 << 16) | t1);
        if ((nr == 0 && nc == 0) || (!root && (uint32_t)(rcw_draw(key, d + 1) >> 32) < stop)) { ++count; continue; }
        bool row = nc == 0;
        if (nr != 0 && nc != 0) {
            const int32_t di = c.i1 - c.i0, dj = c.j1 - c.j0;
            row = di != dj ? di > dj : (rcw_draw(key, d) >> 63) != 0;
        }
        const int32_t s = (row ? r0 : c0) + 2 * (int32_t)rcw_below(rcw_draw(key, d + 2), (uint64_t)(row ? nr : nc));
        const int32_t lo = row ? c.j0 : c.i0, hi = row ? c.j1 : c.i1, cnt = (hi - lo) / 2 + 1;
        const int32_t door1 = lo + 2 * (int32_t)rcw_below(rcw_draw(key, d + 3), (uint64_t)cnt);
        const int32_t door2 = (uint32_t)(rcw_draw(key, d + 4) >> 32) < doors ? lo + 2 * (int32_t)rcw_below(rcw_draw(key, d + 5), (uint64_t)cnt) : door1;
        for (int32_t x = lo; x <= hi; ++x)
            if (x != door1 && x != door2) out_host[row ? (size_t)s + (size_t)H * (size_t)x : (size_t)x + (size_t)H * (size_t)s] = 1;
        try {
            if (row) { stack.push_back(Chamber{s + 1, c.i1, c.j0, c.j1}); stack.push_back(Chamber{c.i0, s - 1, c.j0, c.j1}); }
            else     { stack.push_back(Chamber{c.i0, c.i1, s + 1, c.j1}); stack.push_back(Chamber{c.i0, c.i1, c.j0, s - 1}); }
        } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the rooms failed"); }
    }
    if (rooms) *rooms = count;
    return RCW_OK;
}

// ---- the guide (include/rcw.h, "the guide") ---------------------------------------------------------------------------------------------
// Whether the guide's promise holds for this configuration: position_increment + player_radius <= 0.5, the sum rounded once in T.
int guide_promised(const rcw_config& cfg)
{
    if (cfg.world_unit_bits == 64) return cfg.position_increment_wu_f64 + cfg.player_radius_wu_f64 <= 0.5 ? 1 : 0;
    const float sum = cfg.position_increment_wu + cfg.player_radius_wu;
    return sum <= 0.5f ? 1 : 0;
}

namespace {
// The rule for one agent, restated for the host: one pass over the table in index order that keeps the first greatest product sum
// (rcw_guide_kernel strides it a lane an entry and reduces pairs).  D: (2, nd), entry k at D[2 k], D[2 k + 1].
template <typename T>
void guide_rule_one(int H, int W, const uint16_t* F, T x, T y, int32_t d, int32_t nd, const T* D, T inc, uint8_t* action, int32_t* heading)
{
    *heading = -1;
    *action = 3;
    if (!std::isfinite(x) || !std::isfinite(y)) return;
    const T fx = std::floor(x), fy = std::floor(y);
    if (fx < (T)0 || fx >= (T)H || fy < (T)0 || fy >= (T)W) return;
    const int i = (int)fx, j = (int)fy;
    const auto at = [&](int ii, int jj) -> uint32_t {
        return ii >= 0 && ii < H && jj >= 0 && jj < W ? (uint32_t)F[(size_t)ii + (size_t)H * (size_t)jj] : 0xFFFFu;
    };
    const uint32_t f = at(i, j);
    if (f == 0xFFFFu || f == 0u) return;
    const int side[4][2] = {{i - 1, j}, {i + 1, j}, {i, j - 1}, {i, j + 1}};
    int n = -1;
    for (int c = 0; c < 4 && n < 0; ++c)
        if (at(side[c][0], side[c][1]) == f - 1u) n = c;
    if (n < 0) return;                                                     // (a field no flood wrote)
    const T ctx = (T)i + (T)0.5, cty = (T)j + (T)0.5;
    const T cnx = (T)side[n][0] + (T)0.5, cny = (T)side[n][1] + (T)0.5;
    const T e = n < 2 ? y - cty : x - ctx;
    const bool go = std::fabs(e) <= inc;
    const T vx = (go ? cnx : ctx) - x, vy = (go ? cny : cty) - y;
    int32_t arg = 0;
    bool any = false;
    T best = (T)0;
    for (int32_t k = 0; k < nd; ++k) {
        const T a = D[2 * (size_t)k] * vx, b = D[2 * (size_t)k + 1] * vy;
        const T s = a + b;
        if (std::isnan(s)) continue;
        if (!any || s > best) { any = true; best = s; arg = k; }
    }
    const int64_t delta = ((((int64_t)arg - (int64_t)d) % nd) + nd) % nd;
    *heading = arg;
    *action = delta == 0 ? 1 : (delta <= nd / 2 ? 3 : 4);
}
}  // namespace

// The handle-less export: needs no device.
extern "C" int rcw_guide_rule(int32_t H, int32_t W, const void* field, double x, double y, int32_t world_unit_bits, int32_t direction,
                              int32_t nd, const void* directions_wu, double position_increment, uint8_t* action, int32_t* heading)
{
    if (!field || !directions_wu || !action || !heading) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (H < 1 || W < 1 || (int64_t)H * W > 65535) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_guide_rule: a field of %d x %d", H, W);
    if (world_unit_bits != 32 && world_unit_bits != 64) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_guide_rule: world_unit_bits must be 32 or 64 (got %d)", world_unit_bits);
    if (nd < 1 || direction < 0 || direction >= nd) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_guide_rule: direction %d of %d", direction, nd);
    if (world_unit_bits == 64)
        guide_rule_one<double>(H, W, static_cast<const uint16_t*>(field), x, y, direction, nd, static_cast<const double*>(directions_wu), position_increment, action, heading);
    else
        guide_rule_one<float>(H, W, static_cast<const uint16_t*>(field), (float)x, (float)y, direction, nd, static_cast<const float*>(directions_wu), (float)position_increment, action, heading);
    return RCW_OK;
}

// ---- the frontier (include/rcw.h, "the frontier") ---------------------------------------------------------------------------------------
// The handle-less export: the flood for ONE agent on the host, needs no device.  A queue of tile indices in the order reached
// (rcw_frontier_kernel takes a level a pass of the wavefront; the values are the same: a breadth-first level is a set).  A neighbour is
// looked at by (row, column), never by linear distance: tile (H-1, j) and tile (0, j+1) are no neighbours.
extern "C" int rcw_frontier_rule(int32_t H, int32_t W, const uint8_t* seen_map, void* field_out, int32_t* tiles_out)
{
    if (!seen_map || !field_out || !tiles_out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (H < 1 || W < 1 || (int64_t)H * W > 65535) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_frontier_rule: a map of %d x %d", H, W);
    const int32_t HW = H * W;
    uint16_t* const F = static_cast<uint16_t*>(field_out);
    std::vector<int32_t> queue;
    try {
        queue.reserve((size_t)HW);
    } catch (const std::bad_alloc&) {
        return fail(RCW_ERR_OUT_OF_MEMORY, "rcw_frontier_rule: host allocation failed");
    }
    const auto passable = [&](int32_t t) { return seen_map[t] == 1 || seen_map[t] == 3; };   // (a byte above 4 is a wall)
    // the edge neighbours of t = i + H j that lie on the map
    const auto neighbours = [&](int32_t t, int32_t* out) {
        const int32_t i = t % H, j = t / H;
        int n = 0;
        if (i > 0) out[n++] = t - 1;
        if (i < H - 1) out[n++] = t + 1;
        if (j > 0) out[n++] = t - H;
        if (j < W - 1) out[n++] = t + H;
        return n;
    };
    int32_t nb[4];
    for (int32_t t = 0; t < HW; ++t) {
        F[t] = 0xFFFFu;
        if (seen_map[t] != 0) continue;
        const int n = neighbours(t, nb);
        for (int k = 0; k < n; ++k)
            if (passable(nb[k])) { F[t] = 0; queue.push_back(t); break; }
    }
    *tiles_out = (int32_t)queue.size();
    for (size_t head = 0; head < queue.size(); ++head) {                   // (every tile enters at most once: at most HW entries)
        const int32_t t = queue[head];
        const int n = neighbours(t, nb);
        for (int k = 0; k < n; ++k)
            if (passable(nb[k]) && F[nb[k]] == 0xFFFFu) { F[nb[k]] = (uint16_t)(F[t] + 1u); queue.push_back(nb[k]); }
    }
    return RCW_OK;
}

// ---- the start rule (include/rcw.h, "the start rule") -----------------------------------------------------------------------------------
int check_start_band(int32_t lo, int32_t hi) { return lo >= 1 && lo <= hi && hi <= RCW_START_DISTANCE_MAX ? RCW_OK : RCW_ERR_INVALID_ARGUMENT; }

// The handle-less export: steps 1 to 4 of the rule for ONE agent on the host, needs no device.  A queue flood from the goal by (row,
// column) neighbours, then one pass over the field in tile order that counts the band's tiles — or the farthest ones — and a second that
// stops at the drawn one (rcw_start_distance_kernel marks the band's queue segment in a bitmap and counts set bits: the same r-th tile).
// Neighbours are taken by (row, column), so a map without a wall ring is flooded correctly here; the kernel steps by linear index and
// relies on the ring of every map a handle holds: the two agree on ringed maps (include/rcw.h says so).
extern "C" int rcw_start_rule(const uint8_t* walls, int32_t H, int32_t W, int32_t gi, int32_t gj, uint64_t key, int32_t lo, int32_t hi,
                              int32_t* tile, int32_t* outcome)
{
    if (!walls || !tile || !outcome) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (H < 1 || W < 1 || (int64_t)H * W > 65535) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_start_rule: a map of %d x %d", H, W);
    if (check_start_band(lo, hi) != RCW_OK)
        return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_start_rule: the band must be 1 <= lo <= hi <= %d (got %d, %d)", RCW_START_DISTANCE_MAX, lo, hi);
    const int32_t HW = H * W;
    std::vector<uint16_t> F;
    std::vector<int32_t> queue;
    try {
        F.assign((size_t)HW, (uint16_t)0xFFFFu);
        queue.reserve((size_t)HW);
    } catch (const std::bad_alloc&) {
        return fail(RCW_ERR_OUT_OF_MEMORY, "rcw_start_rule: host allocation failed");
    }
    if (gi >= 1 && gi <= H && gj >= 1 && gj <= W && walls[(gi - 1) + H * (gj - 1)] == 0) {   // (a goal inside a wall reaches nothing)
        F[(size_t)((gi - 1) + H * (gj - 1))] = 0;
        queue.push_back((gi - 1) + H * (gj - 1));
    }
    int32_t D = -1;
    for (size_t head = 0; head < queue.size(); ++head) {                   // (every tile enters at most once: at most HW entries)
        const int32_t t = queue[head], i = t % H, j = t / H;
        D = F[(size_t)t];
        const int32_t nb[4] = {i > 0 ? t - 1 : -1, i < H - 1 ? t + 1 : -1, j > 0 ? t - H : -1, j < W - 1 ? t + H : -1};
        for (int k = 0; k < 4; ++k)
            if (nb[k] >= 0 && walls[nb[k]] == 0 && F[(size_t)nb[k]] == 0xFFFFu) { F[(size_t)nb[k]] = (uint16_t)(F[(size_t)t] + 1u); queue.push_back(nb[k]); }
    }
    int32_t from = lo, to = hi;
    *outcome = 1;
    if (D < lo) {                                                          // the band lies beyond what can be reached (or nothing is)
        if (D < 1) { *outcome = 3; *tile = -1; return RCW_OK; }
        *outcome = 2; from = D; to = D;
    }
    const auto in = [&](int32_t t) { return F[(size_t)t] != 0xFFFFu && (int32_t)F[(size_t)t] >= from && (int32_t)F[(size_t)t] <= to; };
    uint64_t n = 0;
    for (int32_t t = 0; t < HW; ++t) n += in(t) ? 1u : 0u;
    uint64_t r = rcw_below(rcw_draw(key, 0xC000000000000000ull), n);
    *tile = -1;
    for (int32_t t = 0; t < HW && *tile < 0; ++t)
        if (in(t) && r-- == 0) *tile = t;
    return RCW_OK;
}

// THE PER-AGENT ARRAYS (rcw_handle.h): the parts of `feature` (AgentFeature) of a handle of this shape, in the order an exported row of the
// state archive holds them, and the bytes of the feature's head.  What is off has no parts and no head.  This is the ONE place that knows
// an array's bytes per agent: the setters carve it, the archive records it, the readouts copy it.  `kept` = false: a part the archive
// does not record.  The local map's image is recorded (and not computed again behind a restore): it is then what binds the archive to the
// map's size.
void agent_arrays(const SnapshotShape& sh, int feature, AgentArrays* out)
{
    AgentArrays& p = *out;
    p = AgentArrays{};
    const uint32_t real = sh.real64 ? 8u : 4u, HW = (uint32_t)sh.H * (uint32_t)sh.W;
    const uint32_t reward = (sh.reward_type == RCW_REWARD_FLOAT64 || sh.reward_type == RCW_REWARD_INT64) ? 8u : 4u;
    const auto add = [&p](SnapshotField f, const char* name, uint32_t bytes, uint64_t tag = 0, bool kept = true) { p.part[p.n++] = AgentPart{f, name, bytes, tag, kept}; };
    if (feature == kFeatCore) {
        add(kSnapPos, sh.real64 ? "pos64" : "pos", 2 * real);
        add(kSnapDir, "dir", 4);
        add(kSnapGoal, "goal", 8);
        add(kSnapReward, "reward", reward, (uint64_t)sh.reward_type);
        add(kSnapDone, "done", 1);
        add(kSnapEpisode, "episode", 4);
        add(kSnapTileMap, "tile_map", 8u * ((2u * HW + 63u) / 64u));
        add(kSnapEpisodeSteps, "episode_steps", 4);
        add(kSnapTruncated, "truncated", 1);
    }
    if (feature == kFeatGoal && sh.goal) {
        add(kSnapGoalField, "goal_distance.field", 2u * HW);
        add(kSnapGoalDistance, "goal_distance.distance", 4);
        add(kSnapGoalStart, "goal_distance.start_distance", 4);
        add(kSnapGoalProgress, "goal_distance.progress", 4);
        add(kSnapGoalLast, "goal_distance.last_episode", 4);
    }
    if (feature == kFeatSeen && sh.seen) {
        add(kSnapSeenCount, "seen_map.seen_count", 4);
        add(kSnapSeenNew, "seen_map.newly_seen", 4);
        add(kSnapSeenGoal, "seen_map.goal_seen", 4);
        add(kSnapSeenLast, "seen_map.last_episode", 4);
        add(kSnapSeenBits, "seen_map.bits", 4u * ((HW + 31u) / 32u));
        add(kSnapSeenMap, "seen_map.map", HW);
    }
    if (feature == kFeatView && sh.view_fmt) {                             // head: the box tables (plan_learner_view's ViewPlan::tab)
        const uint32_t frame = (uint32_t)sh.view_C * (uint32_t)sh.view_h * (uint32_t)sh.view_w;
        const uint64_t tag = (uint64_t)sh.view_h | (uint64_t)sh.view_w << 16 | (uint64_t)sh.view_fmt << 32 | (uint64_t)sh.view_layout << 40 | (uint64_t)sh.view_frames << 48;
        p.head = sizeof(int32_t) * ((uint64_t)sh.view_h + (uint64_t)sh.view_w + 2 + (sh.view_fmt & RCW_VIEW_DEPTH8 ? (uint64_t)sh.Hc + 1 : 0));
        if (sh.view_frames > 1) {
            add(kSnapViewStack, "learner_view.stack", frame * (uint32_t)sh.view_frames, tag);
            add(kSnapViewLast, "learner_view.last_episode", 4);
            add(kSnapViewStaging, "learner_view.staging", frame, 0, false);
        } else {
            add(kSnapViewFrame, "learner_view.frame", frame, tag);
        }
    }
    if (feature == kFeatLocal && sh.local_source) {                        // head: the offset table (plan_local_map)
        p.head = (uint64_t)sh.local_size * real;
        add(kSnapLocalImage, "local_map.image", (uint32_t)sh.local_size * (uint32_t)sh.local_size,
            (uint64_t)sh.local_size | (uint64_t)sh.local_cells << 16 | (uint64_t)sh.local_source << 32);
    }
    if (feature == kFeatSource && sh.source_kind) {
        add(kSnapSourceLast, "layout_source.last_episode", 4, (uint64_t)sh.source_kind);
        add(kSnapSourceStatus, "layout_source.status_seen", 4, 0, false);
        add(kSnapSourceLayout, "layout_source.layout", 4, (uint64_t)sh.source_kind);
        add(kSnapSourceMask, "layout_source.mask", 1, 0, false);
    }
    if (feature == kFeatStats && sh.stats) {                               // head: the table, a row of the batch and the level rows
        int32_t rows = 0, first = 0;
        plan_episode_stats_rows((RcwLayoutKind)sh.source_kind, sh.layouts, sh.levels, sh.first_level, &rows, &first);
        p.head = sizeof(uint64_t) * RCW_EPISODE_STATS_ROW_WORDS * (1 + (uint64_t)rows);
        add(kSnapStatsFinished, "episode_stats.finished", 1);
        add(kSnapStatsOutcome, "episode_stats.outcome", 1);
        add(kSnapStatsLength, "episode_stats.length", 4);
        add(kSnapStatsMoves, "episode_stats.moves", 4);
        add(kSnapStatsLevel, "episode_stats.level", 4);
        add(kSnapStatsSpl, "episode_stats.spl_q16", 4);
        add(kSnapStatsEpisodes, "episode_stats.episodes", 4);
        add(kSnapStatsPrevX, "episode_stats.prev_x", real);
        add(kSnapStatsPrevY, "episode_stats.prev_y", real);
        add(kSnapStatsLast, "episode_stats.last_episode", 4);
    }
    if (feature == kFeatGuide && sh.guide) {                               // computed from the state, never recorded: a row fits a handle with or without it
        add(kSnapGuideAction, "guide.action", 1, 0, false);
        add(kSnapGuideHeading, "guide.heading", 4, 0, false);
    }
    if (feature == kFeatFrontier && sh.frontier) {                         // computed from the seen map, never recorded: a restore floods the restored agents again
        add(kSnapFrontierDistance, "frontier.distance", 4, 0, false);
        add(kSnapFrontierTiles, "frontier.tiles", 4, 0, false);
        add(kSnapFrontierAction, "frontier.action", 1, 0, false);
        add(kSnapFrontierHeading, "frontier.heading", 4, 0, false);
        add(kSnapFrontierLast, "frontier.last_episode", 4, 0, false);
        add(kSnapFrontierField, "frontier.field", 2u * HW, 0, false);
    }
    if (feature == kFeatVisits && sh.visit_sectors) {                      // head: the table (not part of a record); every part is episode state nothing recomputes
        const uint64_t cells = (uint64_t)sh.visit_sectors * HW;
        if (sh.visit_flags & RCW_VISIT_TABLE) {
            int32_t rows = 0, first = 0;
            plan_visit_table_rows(sh, &rows, &first);
            p.head = sizeof(uint32_t) * cells * (1 + (uint64_t)rows);
        }
        add(kSnapVisitHere, "visit_map.here", 4);
        add(kSnapVisitVisited, "visit_map.visited", 4);
        add(kSnapVisitFirst, "visit_map.first", 4);
        add(kSnapVisitLevelHere, "visit_map.level_here", 4);
        add(kSnapVisitLast, "visit_map.last_episode", 4);
        add(kSnapVisitMap, "visit_map.map", (uint32_t)(2u * cells), (uint64_t)sh.visit_sectors);   // (the tag: a 2-sector row is not a 1-sector one of a map twice the size)
    }
    if (feature == kFeatStart && sh.start) {                               // the mask is the last launch's and no part of a record
        add(kSnapStartLast, "start_distance.last_episode", 4);
        add(kSnapStartPlaced, "start_distance.placed", 1);
        add(kSnapStartMask, "start_distance.mask", 1, 0, false);
    }
}

// THE CARVE of one buffer: `head` bytes, then the `n` parts for B agents in list order, each on a multiple of 16 bytes — the offset of
// every part and the total to allocate.
AgentCarve carve_agent_arrays(uint64_t head, const AgentPart* part, int n, uint64_t B)
{
    const auto up16 = [](uint64_t v) { return (v + 15) & ~(uint64_t)15; };
    AgentCarve c;
    c.total = up16(head);
    for (int k = 0; k < n; ++k) { c.off[k] = c.total; c.total = up16(c.total + B * part[k].bytes); }
    return c;
}

// THE STATE ARCHIVE'S RECORD (include/rcw.h, "the state archive"): the segment table of a handle of this shape, in the order an exported row
// holds the segments — the archived parts of every feature, in the features' order.
void plan_snapshot(const SnapshotShape& sh, SnapshotPlan* plan)
{
    SnapshotPlan& p = *plan;
    p = SnapshotPlan{};
    for (int f = 0; f < kFeatCount; ++f) {
        AgentArrays a;
        agent_arrays(sh, f, &a);
        for (int k = 0; k < a.n; ++k)
            if (a.part[k].archived) p.seg[p.n++] = SnapshotSegment{a.part[k].id, a.part[k].name, a.part[k].bytes, a.part[k].tag};
    }
    uint64_t k = 0xcbf29ce484222325ull;                                    // FNV-1a, a byte at a time
    const auto mix = [&k](uint64_t v, int bytes) { for (int b = 0; b < bytes; ++b) { k ^= (v >> (8 * b)) & 0xffu; k *= 0x100000001b3ull; } };
    for (int s = 0; s < p.n; ++s) {
        p.row_bytes += p.seg[s].bytes;
        for (const char* c = p.seg[s].name; *c; ++c) mix((uint8_t)*c, 1);
        mix(p.seg[s].bytes, 4);
        mix(p.seg[s].tag, 8);
    }
    for (int32_t v : {sh.H, sh.W, sh.nd, sh.N, sh.Hc, sh.real64, sh.reward_type, (int32_t)RCW_ABI_VERSION}) mix((uint32_t)v, 4);
    p.key = k;
}

// The name of the first segment by which `now` — the handle's shape at a save or a restore — differs from `bound`, the archive's; NULL: none.
const char* snapshot_plan_differs(const SnapshotPlan& bound, const SnapshotPlan& now)
{
    for (int k = 0; k < bound.n || k < now.n; ++k) {
        if (k >= now.n) return bound.seg[k].name;
        if (k >= bound.n) return now.seg[k].name;
        const SnapshotSegment& a = bound.seg[k], &b = now.seg[k];
        if (a.field != b.field) return a.field < b.field ? a.name : b.name;   // (the table is in the enum's order: the lower one is the one the other side lacks)
        if (a.bytes != b.bytes || a.tag != b.tag) return a.name;
    }
    return nullptr;
}

// rcw_snapshot_rows_load's check of ONE exported row: the fields a kernel indexes with — goal interior, direction in range, position finite
// and inside the room, the map's border WALL bits set and its padding clear, the layout index in the source's range.  Everything else is
// the caller's word, as rcw_set_walls' layouts are.  msg: the field and why.
int validate_snapshot_row(const SnapshotShape& sh, const SnapshotPlan& plan, const uint8_t* row, char* msg, size_t cap)
{
    const int H = sh.H, W = sh.W;
    const auto at = [&](SnapshotField f) { return row + plan.offset(plan.find(f)); };
    int32_t goal[2], dir;
    std::memcpy(goal, at(kSnapGoal), sizeof goal);
    std::memcpy(&dir, at(kSnapDir), sizeof dir);
    if (goal[0] < 2 || goal[0] > H - 1 || goal[1] < 2 || goal[1] > W - 1) {
        std::snprintf(msg, cap, "goal: (%d,%d) not an interior tile", goal[0], goal[1]);
        return RCW_ERR_INVALID_ARGUMENT;
    }
    if (dir < 0 || dir >= sh.nd) {
        std::snprintf(msg, cap, "dir: %d not in 0..%d", dir, sh.nd - 1);
        return RCW_ERR_INVALID_ARGUMENT;
    }
    double x, y;
    if (sh.real64) { double v[2]; std::memcpy(v, at(kSnapPos), sizeof v); x = v[0]; y = v[1]; }
    else { float v[2]; std::memcpy(v, at(kSnapPos), sizeof v); x = v[0]; y = v[1]; }
    if (!(std::isfinite(x) && std::isfinite(y) && x >= 1.0 && x < (double)(H - 1) && y >= 1.0 && y < (double)(W - 1))) {
        std::snprintf(msg, cap, "%s: (%g,%g) not inside the room", sh.real64 ? "pos64" : "pos", x, y);
        return RCW_ERR_INVALID_ARGUMENT;
    }
    const uint8_t* const map = at(kSnapTileMap);
    const uint32_t map_bits = 8u * plan.seg[plan.find(kSnapTileMap)].bytes;
    const auto bit = [map](uint32_t b) { return (map[b >> 3] >> (b & 7u)) & 1u; };
    for (int j = 0; j < W; ++j)
        for (int i = 0; i < H; ++i)
            if ((i == 0 || i == H - 1 || j == 0 || j == W - 1) && !bit(2u * ((uint32_t)i + (uint32_t)H * (uint32_t)j))) {
                std::snprintf(msg, cap, "tile_map: the border tile (%d,%d) is not a wall", i + 1, j + 1);
                return RCW_ERR_INVALID_ARGUMENT;
            }
    for (uint32_t b = 2u * (uint32_t)H * (uint32_t)W; b < map_bits; ++b)
        if (bit(b)) {
            std::snprintf(msg, cap, "tile_map: padding bit %u is set", b);
            return RCW_ERR_INVALID_ARGUMENT;
        }
    if (sh.source_kind) {
        int32_t layout;
        std::memcpy(&layout, at(kSnapSourceLayout), sizeof layout);
        const bool bank = sh.source_kind == kLayoutBank;
        const int32_t lo = bank ? 0 : (sh.levels > 0 ? sh.first_level : -1), count = bank ? sh.layouts : (sh.levels > 0 ? sh.levels : 1);
        if (layout < lo || (int64_t)layout >= (int64_t)lo + count) {
            std::snprintf(msg, cap, "layout_source.layout: %d not in %d..%lld", layout, lo, (long long)lo + count - 1);
            return RCW_ERR_INVALID_ARGUMENT;
        }
    }
    return RCW_OK;
}

#ifdef RCW_DEV_SWITCHES
#include "dev/api_plan_export.inc"   // the rules and the step's facts without a device (tests/test_top_view_plan.py, tests/test_step_state.py)
#endif
