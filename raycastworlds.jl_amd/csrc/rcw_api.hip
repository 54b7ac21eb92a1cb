// C ABI of librcw_hip (include/rcw.h): the entry points, their argument checks, and where a failure's text is kept.
#include "rcw_handle.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <utility>
#include <vector>

namespace {

thread_local char g_err[512] = "";

void set_error(const char* fmt, va_list ap) { vsnprintf(g_err, sizeof g_err, fmt, ap); }

}  // namespace

// (the name in parentheses: the development build's macro of that name, rcw_error.h, is not meant here)
int (fail)(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    set_error(fmt, ap);
    va_end(ap);
    return code;
}
#ifdef RCW_DEV_SWITCHES
// Development build only (rcw_error.h): the error returns taken, a table of source lines for each host unit
namespace {
const char* const kFailUnits[] = {"rcw_api.hip", "rcw_rules.hip", "rcw_step.hip", "rcw_comm.hip"};
constexpr int kFailUnitCount = (int)(sizeof kFailUnits / sizeof kFailUnits[0]);
unsigned char g_fail_hit[kFailUnitCount][4096];
}  // namespace
int fail_at(const char* file, int line, int code, const char* fmt, ...)
{
    for (int u = 0; u < kFailUnitCount; ++u)
        if (!std::strcmp(file, kFailUnits[u]) && line >= 0 && line < (int)sizeof g_fail_hit[u]) g_fail_hit[u][line] = 1;
    va_list ap;
    va_start(ap, fmt);
    set_error(fmt, ap);
    va_end(ap);
    return code;
}
// the file name of host unit `unit` (0 ..), NULL past the last one; the lines of that unit taken so far: out[line] = 1, returns the bytes
// written, -1 for a bad argument or past the last unit
extern "C" __attribute__((visibility("default"))) const char* rcw_dev_fail_unit(int unit)
{
    return unit >= 0 && unit < kFailUnitCount ? kFailUnits[unit] : nullptr;
}
extern "C" __attribute__((visibility("default"))) int rcw_dev_fail_sites(int unit, unsigned char* out, int cap)
{
    if (unit < 0 || unit >= kFailUnitCount || !out || cap < 1) return -1;
    const int n = cap < (int)sizeof g_fail_hit[unit] ? cap : (int)sizeof g_fail_hit[unit];
    std::memcpy(out, g_fail_hit[unit], (size_t)n);
    return n;
}
#endif

const char* hip_failure(hipError_t e) { (void)hipGetLastError(); return hipGetErrorString(e); }
int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? RCW_ERR_OUT_OF_MEMORY : RCW_ERR_HIP; }   // the RCW_ERR_* of a failed runtime call

int check_handle(rcw_handle* h)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL handle");
    RCW_HIP(hipSetDevice(h->device));
    return RCW_OK;
}

namespace {

void rebuild_ray_table(rcw_handle* h)
{
    if (h->real64) build_ray_table<double>(h->cfg, h->cfg.semi_field_of_view_wu_f64, h->dir_table64, h->ray_table64);
    else build_ray_table<float>(h->cfg, h->cfg.semi_field_of_view_wu, h->dir_table, h->ray_table);
}

int upload_tables(rcw_handle* h)
{
    const void* dirs = h->real64 ? (const void*)h->dir_table64.data() : (const void*)h->dir_table.data();
    const void* rays = h->real64 ? (const void*)h->ray_table64.data() : (const void*)h->ray_table.data();
    const size_t nd2 = (size_t)2 * h->cfg.num_directions, nr = (size_t)h->cfg.num_directions * RCW_TABLE_ROWS * h->cfg.num_rays;
    RCW_HIP(hipMemcpyAsync(h->d_dir_table.get(), dirs, nd2 * h->real_size, hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipMemcpyAsync(h->d_ray_table.get(), rays, nr * h->real_size, hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipStreamSynchronize(h->stream));
    return RCW_OK;
}

// Wait for the stream, then surface the sticky device error word.
int sync_and_check(rcw_handle* h)
{
    RCW_HIP(hipMemcpyAsync(h->h_err.get(), h->d_err.get(), sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    RCW_HIP(hipStreamSynchronize(h->stream));
    const int32_t e = h->h_err.get<int32_t>()[0];
    if (e == RCW_ERR_INVALID_ACTION) return fail(e, "invalid action (must be in 1..%d); the agents it was given to were not stepped (rcw_status)", RCW_NUM_ACTIONS);
    if (e == RCW_ERR_OUT_OF_BOUNDS) return fail(e, "a tile index left the tile map (BoundsError in the reference)");
    if (e == RCW_ERR_HIP) return fail(e, "a kernel gave up waiting for another one after about a second (the top view's store kernel for its draw kernel): the images of that call are not valid");
    if (e == RCW_ERR_INVALID_ARGUMENT) return fail(e, "a row index given to rcw_snapshot_save_device / rcw_snapshot_restore_device was out of range or (restore) named an unfilled row; those agents were left as they were (rcw_status)");
    if (e != 0) return fail(e, "device error %d", e);
    return RCW_OK;
}

// The Float32 entry points serve Float32 worlds, the *64 ones Float64 worlds.
int check_real(rcw_handle* h, bool want64, const char* fn)
{
    if (h->real64 == want64) return RCW_OK;
    return fail(RCW_ERR_UNSUPPORTED, "%s: the handle's world-unit type is %s; use the %s entry point", fn,
                h->real64 ? "Float64" : "Float32", h->real64 ? "*64" : "Float32");
}

// agents [first, first + count) of the handle, count >= min_count (`ok`: what else the caller refuses with the same words — a NULL output pointer)
int check_range(rcw_handle* h, bool ok, int32_t first, int32_t count, int32_t min_count = 0)
{
    if (ok && first >= 0 && count >= min_count && first + (int64_t)count <= h->B) return RCW_OK;
    return fail(RCW_ERR_INVALID_ARGUMENT, "bad agent range [%d, %d)", first, first + count);
}

// rcw_ray_table / rcw_direction_table and their *64 twins: the host's copy of a table, as uploaded
template <typename T>
int table_out(rcw_handle* h, T* out, std::vector<T> rcw_handle::*table, const char* fn)
{
    if (!h || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = check_real(h, sizeof(T) == sizeof(double), fn); if (rc) return rc;
    std::memcpy(out, (h->*table).data(), (h->*table).size() * sizeof(T));
    return RCW_OK;
}

int upload_mask(rcw_handle* h, const uint8_t* mask_host, const uint8_t** mask_dev)
{
    *mask_dev = nullptr;
    if (!mask_host) return RCW_OK;
    RCW_HIP(hipMemcpyAsync(h->d_mask.get(), mask_host, (size_t)h->B, hipMemcpyHostToDevice, h->stream));
    // the host buffer may be pageable and reused by the caller right away
    RCW_HIP(hipStreamSynchronize(h->stream));
    *mask_dev = h->d_mask.get<uint8_t>();
    return RCW_OK;
}

// ---- the per-agent arrays (rcw_handle.h): the shape, the carve into a buffer, the swap, the two readouts ------------------------------------
// What of the handle fixes its arrays and the archive's record NOW (and, for rcw_snapshot_rows_load's check, the layout source's range).
SnapshotShape snapshot_shape(const rcw_handle* h)
{
    SnapshotShape s;
    s.H = h->dev.H; s.W = h->dev.W; s.nd = h->dev.nd; s.N = h->dev.N; s.Hc = h->dev.Hc;
    s.real64 = h->real64 ? 1 : 0; s.reward_type = h->cfg.reward_type;
    s.goal = h->goal.on(); s.seen = h->seen.on(); s.stats = h->stats.on();
    const rcw_handle::LearnerView& lv = h->learner;
    if (lv.on()) { s.view_fmt = lv.set.fmt; s.view_layout = lv.set.layout; s.view_C = lv.view.C; s.view_h = lv.set.h; s.view_w = lv.set.w; s.view_frames = lv.set.frames; }
    if (h->local.on()) { s.local_source = h->local.source; s.local_size = h->local.size; s.local_cells = h->local.cells_per_tile; }
    s.source_kind = (int32_t)h->source.dev.kind;
    s.layouts = h->source.dev.agents.layouts; s.levels = h->source.dev.gen.levels; s.first_level = h->source.dev.gen.first_level;
    s.guide = h->guide.on();
    s.frontier = h->frontier.on();
    if (h->visits.on()) { s.visit_sectors = h->visits.dev.sectors; s.visit_flags = h->visits.flags; }
    s.start = h->start.on();
    return s;
}

// ONE buffer of a feature a setter is building: `head` bytes, then parts [first, first + n) of `list` for the handle's agents
// (carve_agent_arrays).  at: the parts' entries, indexed as rcw_handle::live is; *bytes: the carve's total, allocated or not.
hipError_t alloc_parts(const rcw_handle* h, RcwBuf& buf, const AgentArrays& list, int first, int n, uint64_t head, LiveArray* at, size_t* bytes = nullptr)
{
    const AgentCarve c = carve_agent_arrays(head, list.part + first, n, (uint64_t)h->B);
    if (bytes) *bytes = (size_t)c.total;
    const hipError_t e = buf.hipMalloc((size_t)c.total);
    for (int k = 0; k < n && e == hipSuccess; ++k) at[list.part[first + k].id] = LiveArray{buf.get<uint8_t>() + c.off[k], list.part[first + k].bytes};
    return e;
}

// THE way a feature is swapped in, behind which the setter says `feature = std::move(fresh)` (an owner that takes another over frees what it
// had): every stream is waited for as for replace_buffers — queued work may still use the old arrays —, then the table takes the
// feature's entries of `at` — all null where the feature is switched off.  A failed wait leaves the handle as it was.
hipError_t take_live(rcw_handle* h, int feature, const LiveArray* at)
{
    const hipError_t e = replace_buffers(h, {});
    for (int id = kFeatureFirstId[feature]; id < kFeatureFirstId[feature + 1] && e == hipSuccess; ++id) h->live[id] = at[id];
    return e;
}

// Why a readout is refused while its feature is off.
const char* const kNoLearnerView = "the handle has no learner view (rcw_set_learner_view)";
const char* const kNoGoalDistance = "the handle has no goal distance (rcw_set_goal_distance)";
const char* const kNoSeenMap = "the handle has no seen map (rcw_set_seen_map)";
const char* const kNoLocalMap = "the handle has no local map (rcw_set_local_map)";
const char* const kNoDrawnWalls = "the handle has neither a wall bank (rcw_set_wall_bank) nor a wall generator (rcw_set_wall_generator, rcw_set_wall_caves, rcw_set_wall_rooms)";
const char* const kNoEpisodeStats = "the handle keeps no episode statistics (rcw_set_episode_stats)";
const char* const kNoGuide = "the handle has no guide (rcw_set_guide)";
const char* const kNoFrontier = "the handle has no frontier (rcw_set_frontier)";
const char* const kNoVisitMap = "the handle has no visit map (rcw_set_visit_map)";
const char* const kNoStartRule = "the handle has no start rule (rcw_set_start_distance)";
const char* const kNoVisitTable = "the handle's visit map has no table (rcw_set_visit_map with RCW_VISIT_TABLE)";
int need(bool on, const char* why_off) { return on ? RCW_OK : fail(RCW_ERR_UNSUPPORTED, "%s", why_off); }

// (the array of the learner view the caller sees: the k-frame stack, or the one frame)
SnapshotField view_id(const rcw_handle* h) { return h && h->learner.set.frames > 1 ? kSnapViewStack : kSnapViewFrame; }

// THE readout to the host, behind check_handle: every array of `outs` whose host pointer is not NULL, for all agents or — ranged — agents
// [first, first + count), behind ONE sync_and_check.  The checks in their order: the feature is off (why_off; NULL: the core state, always
// on), a bad range or a NULL pointer (ranged: of the one array; else a lone array's — of several, any may be NULL), the sticky device error.
struct HostOut { void* host; SnapshotField id; };
int copy_arrays(rcw_handle* h, const char* why_off, std::initializer_list<HostOut> outs, bool ranged = false, int32_t first = 0, int32_t count = 0)
{
    int rc = need(!why_off || h->live[outs.begin()->id].ptr, why_off); if (rc) return rc;
    if (ranged) { rc = check_range(h, outs.begin()->host != nullptr, first, count); if (rc) return rc; }
    else if (outs.size() == 1 && !outs.begin()->host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL output pointer");
    if (!ranged) count = h->B;
    rc = sync_and_check(h);
    for (const HostOut& o : outs) {
        const LiveArray& a = h->live[o.id];
        if (o.host) RCW_HIP(hipMemcpy(o.host, a.as<uint8_t>() + (size_t)first * a.bytes, (size_t)count * a.bytes, hipMemcpyDeviceToHost));
    }
    return rc;
}

// ... and the arrays' device pointers, which waits for nothing: a lone pointer must not be NULL, of several any may be.
struct DeviceOut { void** ptr; SnapshotField id; };
int hand_out(rcw_handle* h, const char* why_off, std::initializer_list<DeviceOut> outs)
{
    if (!h || (outs.size() == 1 && !outs.begin()->ptr)) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const int rc = need(!why_off || h->live[outs.begin()->id].ptr, why_off); if (rc) return rc;
    for (const DeviceOut& o : outs)
        if (o.ptr) *o.ptr = h->live[o.id].ptr;
    return RCW_OK;
}

}  // namespace

extern "C" {

int rcw_abi_version(void) { return RCW_ABI_VERSION; }
const char* rcw_last_error(void) { return g_err; }

int rcw_config_default(rcw_config* c)
{
    if (!c) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL config");
    std::memset(c, 0, sizeof *c);
    c->abi_version = RCW_ABI_VERSION;
    c->height_tile_map_tu = 8;          // SR:260
    c->width_tile_map_tu = 16;          // SR:261
    c->num_directions = 128;            // SR:262
    c->num_rays = 512;                  // SR:268
    c->height_camera_view_pu = 256;     // SR:271
    c->pu_per_tu = 32;                  // SR:269
    c->player_radius_wu = (float)(1.0 / 8.0);        // convert(T, 1/8) SR:263
    c->position_increment_wu = (float)(1.0 / 8.0);   // SR:264
    c->semi_field_of_view_wu = (float)(2.0 / 3.0);   // convert(T, 2/3) SR:267
    c->camera_height_tile_wu = 1.0f;    // SR:270
    c->goal_reward = 1.0f;              // one(R) SR:82
    c->floor_color = 0x00404040u;       // SR:291
    c->ceiling_color = 0x00FFFFFFu;     // SR:292
    c->wall_dim_1_color = 0x00808080u;  // SR:293
    c->wall_dim_2_color = 0x00c0c0c0u;  // SR:294
    c->goal_dim_1_color = 0x00800000u;  // SR:295
    c->goal_dim_2_color = 0x00c00000u;  // SR:296
    c->dda_tie_break = RCW_DDA_TIE_X_FIRST_ON_LT;
    c->dda_distance = RCW_DDA_DIST_SIDE_MINUS_DELTA;
    c->normalize_mode = RCW_NORMALIZE_INV_NORM_TIMES;
    c->auto_reset = 0;
    c->agent_id_offset = 0;
    c->reward_type = RCW_REWARD_FLOAT32;           // R = Float32 SR:266
    c->goal_reward_f64 = 1.0;                      // one(R) SR:82
    c->out_of_bounds = RCW_OOB_ERROR;
    c->world_unit_bits = 32;                       // T = Float32 SR:259
    c->player_radius_wu_f64 = 1.0 / 8.0;           // convert(Float64, .) of the same literals
    c->position_increment_wu_f64 = 1.0 / 8.0;
    c->semi_field_of_view_wu_f64 = 2.0 / 3.0;
    c->camera_height_tile_wu_f64 = 1.0;
    return RCW_OK;
}

int rcw_create(const rcw_config* cfg, int32_t batch, int32_t device, uint64_t seed, rcw_handle** out)
{
    if (!cfg || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    int rc = validate_config(cfg, batch);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(RCW_ERR_NO_DEVICE, "no HIP device visible: librcw_hip has no CPU fallback");
    if (device < 0 || device >= ndev)
        return fail(RCW_ERR_NO_DEVICE, "device %d not in 0..%d", device, ndev - 1);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(RCW_ERR_NO_DEVICE, "hipGetDeviceProperties(%d) failed", device);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RCW_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    RCW_HIP(hipSetDevice(device));

    std::unique_ptr<rcw_handle> h(new (std::nothrow) rcw_handle());   // (whichever return leaves from here on: ~rcw_handle, which waits for what was queued first)
    if (!h) return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->cfg = *cfg;
    h->B = batch;
    h->device = device;
    const int H = cfg->height_tile_map_tu, W = cfg->width_tile_map_tu, N = cfg->num_rays;
    const int nd = cfg->num_directions, Hc = cfg->height_camera_view_pu;
    h->nchunks = (2 * H * W + 63) / 64;   // BitArray chunks: cld(2HW, 64)
    h->real64 = cfg->world_unit_bits == 64;
    h->real_size = h->real64 ? sizeof(double) : sizeof(float);
    const size_t B = (size_t)batch;

    RCW_HIP(h->own_stream.hipStreamCreate());
    h->stream = h->own_stream.get();
    RCW_HIP(h->ev_start.hipEventCreate());
    RCW_HIP(h->ev_stop.hipEventCreate());
    {   // the core state: a buffer a part (+ 2 words: the flat top store kernel reads three words from any word of a map)
        SnapshotShape sh;
        sh.H = H; sh.W = W; sh.real64 = h->real64; sh.reward_type = cfg->reward_type;
        AgentArrays core;
        agent_arrays(sh, kFeatCore, &core);
        RcwBuf* const buf[] = {&h->d_pos, &h->d_dir, &h->d_goal, &h->d_reward, &h->d_done, &h->d_episode, &h->d_tile_map, &h->d_episode_steps, &h->d_truncated};
        for (int k = 0; k < core.n; ++k) {
            RCW_HIP(buf[k]->hipMalloc(B * core.part[k].bytes + 16));
            h->live[core.part[k].id] = LiveArray{buf[k]->get(), core.part[k].bytes};
        }
    }
    RCW_HIP(h->d_dir_table.hipMalloc((size_t)nd * 2 * h->real_size));
    RCW_HIP(h->d_ray_table.hipMalloc((size_t)nd * RCW_TABLE_ROWS * N * h->real_size));
    RCW_HIP(h->d_obs.hipMalloc(B * (size_t)N * Hc * sizeof(uint32_t)));
    RCW_HIP(h->d_col_h.hipMalloc(B * (size_t)N * sizeof(int32_t)));
    RCW_HIP(h->d_col_c.hipMalloc(B * (size_t)N));
    if (cfg->render_top_view)
        RCW_HIP(h->d_top_view.hipMalloc(B * (size_t)H * W * cfg->pu_per_tu * cfg->pu_per_tu * sizeof(uint32_t)));
    RCW_HIP(h->d_err.hipMalloc(sizeof(int32_t)));
    RCW_HIP(h->d_status.hipMalloc(B * sizeof(int32_t)));
    RCW_HIP(h->d_actions.hipMalloc(B));
    RCW_HIP(h->d_mask.hipMalloc(B));
    RCW_HIP(h->d_in_goal.hipMalloc(B * sizeof(int2)));
    RCW_HIP(h->d_in_pos.hipMalloc(B * 2 * h->real_size));
    RCW_HIP(h->d_in_dir.hipMalloc(B * sizeof(int32_t)));
    RCW_HIP(h->h_err.hipHostMalloc(sizeof(int32_t)));
    for (int k = 0; k < 2; ++k) {
        RCW_HIP(h->h_actions[k].hipHostMalloc(B));
        RCW_HIP(h->ev_actions[k].hipEventCreate(hipEventDisableTiming));
    }
    RCW_HIP(hipMemsetAsync(h->d_err.get(), 0, sizeof(int32_t), h->stream));
    RCW_HIP(hipMemsetAsync(h->d_status.get(), 0, B * sizeof(int32_t), h->stream));
    RCW_HIP(hipMemsetAsync(h->d_episode_steps.get(), 0, B * sizeof(uint32_t), h->stream));
    RCW_HIP(hipMemsetAsync(h->d_truncated.get(), 0, B, h->stream));

    RcwPlan& d = h->dev;
    set_geometry(d, cfg, batch);
    d.nwords = h->nchunks * 2;
    d.radius = cfg->player_radius_wu;
    d.radius_sq = cfg->player_radius_wu * cfg->player_radius_wu;        // radius * radius CD:18
    d.inc = cfg->position_increment_wu;
    d.goal_reward = cfg->goal_reward;
    d.goal_reward64 = cfg->goal_reward_f64;
    d.reward_type = cfg->reward_type;
    d.num = cfg->camera_height_tile_wu * (float)N;                      // SR:406 numerator
    d.two_fov = 2.0f * cfg->semi_field_of_view_wu;                      // 2 * fov
    d.radius64 = cfg->player_radius_wu_f64;
    d.radius_sq64 = cfg->player_radius_wu_f64 * cfg->player_radius_wu_f64;
    d.inc64 = cfg->position_increment_wu_f64;
    d.num64 = cfg->camera_height_tile_wu_f64 * (double)N;
    d.two_fov64 = 2.0 * cfg->semi_field_of_view_wu_f64;
    d.floor_color = cfg->floor_color; d.ceiling_color = cfg->ceiling_color;
    d.colour[RCW_COLOUR_WALL_DIM_1] = cfg->wall_dim_1_color;
    d.colour[RCW_COLOUR_WALL_DIM_2] = cfg->wall_dim_2_color;
    d.colour[RCW_COLOUR_GOAL_DIM_1] = cfg->goal_dim_1_color;
    d.colour[RCW_COLOUR_GOAL_DIM_2] = cfg->goal_dim_2_color;
    d.tie_le = cfg->dda_tie_break == RCW_DDA_TIE_X_FIRST_ON_LE;
    d.dist_pre = cfg->dda_distance == RCW_DDA_DIST_PRE_INCREMENT;
    d.auto_reset = cfg->auto_reset ? 1 : 0;
    d.agent_id_offset = cfg->agent_id_offset;
    d.seed = seed;
    d.pos = h->d_pos.get<float2>(); d.pos64 = h->d_pos.get<double2>(); d.dir = h->d_dir.get<int32_t>(); d.goal = h->d_goal.get<int2>();
    d.reward = h->d_reward.get(); d.done = h->d_done.get<uint8_t>(); d.episode = h->d_episode.get<uint32_t>();
    d.tile_map = h->d_tile_map.get<uint32_t>();
    d.dir_table = h->d_dir_table.get<float2>(); d.ray_table = h->d_ray_table.get<float>();
    d.dir_table64 = h->d_dir_table.get<double2>(); d.ray_table64 = h->d_ray_table.get<double>();
    d.obs = h->d_obs.get<uint32_t>(); d.col_h = h->d_col_h.get<int32_t>(); d.col_c = h->d_col_c.get<uint8_t>();
    d.err = h->d_err.get<int32_t>();
    d.top_view = h->d_top_view.get<uint32_t>();
    d.status = h->d_status.get<int32_t>();
    d.limit = RcwLimit{h->d_episode_steps.get<uint32_t>(), h->d_truncated.get<uint8_t>(), 0};
    d.oob_empty = cfg->out_of_bounds == RCW_OOB_TREAT_EMPTY;
    h->hw.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (prop.sharedMemPerBlock >= 64 * 1024) h->hw.lds_per_cu = (int)prop.sharedMemPerBlock;           // (gfx950: 160 KiB, the whole CU's)
    if (prop.maxThreadsPerMultiProcessor >= 64) h->hw.waves_per_cu = prop.maxThreadsPerMultiProcessor / 64;
    // fill kernel: one workgroup per CU (256 on an MI355X in SPX mode; a partitioned device reports fewer)
    d.fill_grid = h->hw.cus; d.fill_plain = 0; d.fill_flat = 0;
    // lanes per agent in the cast kernel: four rays a lane once the batch fills the chip (measured, µs: 512 columns 45.6 vs 51.4
    // with two a lane, 256 columns 12.3 vs 12.7; 1024 columns take 256 lanes either way), two a lane for small batches, where
    // an agent's own latency is what counts
    { const int lanes = h->B >= 1024 ? (N + 3) / 4 : (N + 1) / 2; d.cast_block = lanes >= 256 ? 256 : ((lanes + 63) / 64) * 64; }
    // development builds (make dev: -DRCW_DEV_SWITCHES -> librcw_hip_dev.so) read tuning knobs — each overrides a value the rule
    // computes, and so selects code the shipped library can reach too — from the environment; the shipped library reads nothing but
    // RCW_RCCL_LIBRARY
    if (const char* v = RCW_DEV_ENV("RCW_CAST_BLOCK")) { const int b = std::atoi(v); if (b == 64 || b == 128 || b == 192 || b == 256) d.cast_block = b; }
    if (const char* v = RCW_DEV_ENV("RCW_FILL_GRID")) { const int g = std::atoi(v); if (g >= 1 && g <= 65536) d.fill_grid = g; }
    if (const char* v = RCW_DEV_ENV("RCW_FILL_PLAIN")) d.fill_plain = std::atoi(v) ? 1 : 0;
    if (const char* v = RCW_DEV_ENV("RCW_FILL_FLAT")) d.fill_flat = std::atoi(v) ? 1 : 0;
    d.top_rotate = 33;                                                       // (measured: rcw_top_store.hip, rcw_top_store_flat_kernel)
    if (const char* v = RCW_DEV_ENV("RCW_TOP_ROTATE")) { const int r = std::atoi(v); if (r >= 0 && r < 65536) d.top_rotate = r; }
    {
        int want_form = 0, want_runs = 0;
        if (const char* v = RCW_DEV_ENV("RCW_TOP_SPLIT")) { const int f = std::atoi(v); if (!f) want_form = RCW_TOP_VIEW_ONE_KERNEL; else if (f == 2) want_form = RCW_TOP_VIEW_TWO_KERNELS; }
        if (const char* v = RCW_DEV_ENV("RCW_TOP_INPLACE")) { if (std::atoi(v)) want_form = RCW_TOP_VIEW_IN_PLACE; }
        if (const char* v = RCW_DEV_ENV("RCW_TOP_RUNS")) { const int r = std::atoi(v); if (r >= 1 && r <= 8 && r <= batch) want_runs = r; }
        rc = plan_top_view(h.get(), want_form, want_runs, /*lenient=*/true); if (rc) return rc;
    }
    if (rcw_step_lds_bytes(d) > 64 * 1024)
        return fail(RCW_ERR_UNSUPPORTED, "tile map + column buffer need %zu B of LDS (> 64 KiB)", rcw_step_lds_bytes(d));
    if (const char* v = RCW_DEV_ENV("RCW_STEP_STORE_ALL")) h->step.set_store_all(std::atoi(v) != 0);
    {
        int want = 0;
        if (const char* v = RCW_DEV_ENV("RCW_STEP_FORM")) { const int f = std::atoi(v); if (f == RCW_STEP_TWO_LAUNCHES) want = f; }
        rc = plan_step_form(h.get(), want); if (rc) return rc;
    }

    try {
        if (h->real64) build_direction_table<double>(nd, h->dir_table64); else build_direction_table<float>(nd, h->dir_table);
        rebuild_ray_table(h.get());
    } catch (const std::bad_alloc&) {
        return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the (direction, ray) table failed");
    }
    rc = upload_tables(h.get()); if (rc) return rc;
    const hipError_t e = rcw_launch_init_tile_map(d, h->stream);
    if (e != hipSuccess) return fail(RCW_ERR_HIP, "init_tile_map launch: %s", hip_failure(e));
    rc = rcw_reset(h.get(), nullptr, seed); if (rc) return rc;
    rc = sync_and_check(h.get()); if (rc) return rc;
    *out = h.release();
    return RCW_OK;
}

int rcw_destroy(rcw_handle* h)
{
    delete h;            // (NULL: nothing; everything a handle owns goes in ~rcw_handle)
    return RCW_OK;
}

extern "C++" {
template <typename T>
int set_direction_table_impl(rcw_handle* h, const T* directions_wu, std::vector<T>& table)
{
    if (!directions_wu) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL direction table");
    RCW_HIP(hipStreamSynchronize(h->stream));
    try {
        table.assign(directions_wu, directions_wu + (size_t)2 * h->cfg.num_directions);
        rebuild_ray_table(h);
    } catch (const std::bad_alloc&) {
        return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the (direction, ray) table failed");
    }
    int rc = upload_tables(h); if (rc) return rc;
    RCW_HIP(launch_step(h, nullptr, nullptr, kStackRefillSameWorld));   // re-render
    return RCW_OK;
}
}  // extern "C++"

int rcw_set_direction_table(rcw_handle* h, const float* directions_wu)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, false, "rcw_set_direction_table"); if (rc) return rc;
    return set_direction_table_impl<float>(h, directions_wu, h->dir_table);
}
int rcw_set_direction_table64(rcw_handle* h, const double* directions_wu)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, true, "rcw_set_direction_table64"); if (rc) return rc;
    return set_direction_table_impl<double>(h, directions_wu, h->dir_table64);
}

int rcw_set_stream(rcw_handle* h, void* hip_stream)
{
    int rc = check_handle(h); if (rc) return rc;
    RCW_HIP(hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream.get();
    return RCW_OK;
}

int rcw_get_stream(rcw_handle* h, void** hip_stream)
{
    if (!h || !hip_stream) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *hip_stream = (void*)h->stream;
    return RCW_OK;
}

int rcw_bind_obs(rcw_handle* h, void* device_ptr)
{
    int rc = check_handle(h); if (rc) return rc;
    if (device_ptr && ((uintptr_t)device_ptr & 15u))
        return fail(RCW_ERR_INVALID_ARGUMENT, "observation buffer must be 16-byte aligned");
    // No synchronisation: the pointer travels in the kernel arguments of the launches that follow,
    // work already enqueued keeps the buffer it was launched with (double-buffered observations).
    h->dev.obs = device_ptr ? (uint32_t*)device_ptr : h->d_obs.get<uint32_t>();
    h->step.obs_unknown();      // (also with the pointer it had: the caller may have written into the buffer — the next step stores every frame)
    return RCW_OK;
}

int rcw_reset(rcw_handle* h, const uint8_t* mask_host, uint64_t seed)
{
    int rc = check_handle(h); if (rc) return rc;
    const uint8_t* mask_dev = nullptr;
    rc = upload_mask(h, mask_host, &mask_dev); if (rc) return rc;
    h->step.reset(mask_dev != nullptr, seed != h->dev.seed, h->dev.auto_reset != 0);
    h->dev.seed = seed;
    RCW_HIP(rcw_launch_reset(h->dev, mask_dev, h->stream));            // SR:110-132
    RCW_HIP(launch_layout_source(h, false));                           // (a handle with a layout source: the agents of the mask take a layout each)
    RCW_HIP(launch_start_distance(h, false));                          // (... with the start rule: and a tile of the band)
    RCW_HIP(launch_step(h, nullptr, mask_dev, kStackRefill));    // SR:134, SR:329
    return RCW_OK;
}

// ---- the layout sources (rcw_handle::LayoutSource): the wall bank and the wall generator's mazes, caves and rooms ------------------------
// A setter is its own validation and parameters around three shared pieces: the refusal beside another live source, the drop, the install.
extern "C++" {
namespace {

using LayoutSource = rcw_handle::LayoutSource;

// Per kind: what a failed allocation of its install is called, and how a caller is told that it is live — `by_walls` to rcw_set_walls and
// rcw_set_wall_bank, `by_family` to the setters of the generator's families.
struct SourceWords { const char* name; const char* by_walls; const char* by_family; };
const SourceWords kSourceWords[] = {
    /* kLayoutNone  */ {"", "", ""},
    /* kLayoutBank  */ {"wall bank",
                        "the handle draws its walls from a wall bank; switch the bank off first (rcw_set_wall_bank(h, NULL, 0, NULL))",
                        "the handle draws its walls from a wall bank; switch the bank off first (rcw_set_wall_bank(h, NULL, 0, NULL))"},
    /* kLayoutMazes */ {"wall generator",
                        "the handle makes its walls with the wall generator; switch the generator off first (rcw_set_wall_generator(h, 0, ...))",
                        "the handle makes mazes; switch the generator off first (rcw_set_wall_generator(h, 0, ...))"},
    /* kLayoutCaves */ {"wall caves",
                        "the handle makes its walls with the wall generator's caves; switch them off first (rcw_set_wall_caves(h, 0, ...))",
                        "the handle makes caves; switch them off first (rcw_set_wall_caves(h, 0, ...))"},
    /* kLayoutRooms */ {"wall rooms",
                        "the handle makes its walls with the wall generator's rooms; switch them off first (rcw_set_wall_rooms(h, 0, ...))",
                        "the handle makes rooms; switch them off first (rcw_set_wall_rooms(h, 0, ...))"},
};

// THE refusal: `caller` would install a source of kind `wants` (rcw_set_walls: none, it writes walls of its own) beside a live one of another
// kind.  The live kind over itself is a re-install and passes.
int refuse_other_source(rcw_handle* h, const char* caller, RcwLayoutKind wants)
{
    const RcwLayoutKind live = h->source.dev.kind;
    if (live == kLayoutNone || live == wants) return RCW_OK;
    const bool family = wants != kLayoutNone && wants != kLayoutBank;
    return fail(RCW_ERR_UNSUPPORTED, "%s: %s", caller, family ? kSourceWords[live].by_family : kSourceWords[live].by_walls);
}

// THE off branch of a setter: the agents keep the walls they have.  A source of another kind is not this call's to end.
int drop_layout_source(rcw_handle* h, RcwLayoutKind kind)
{
    if (!h->source.is(kind)) return RCW_OK;
    const LiveArray none[kSnapFieldCount] = {};
    RCW_HIP(take_live(h, kFeatSource, none));
    h->source = LayoutSource();
    return RCW_OK;
}

// THE install, behind a setter's validation and staging.  `fresh` holds the kind and its parameters and — the bank — the bank's resources; the
// per-agent arrays of every kind are carved here.  An allocation that fails leaves the handle as it was.  Then the handle takes `fresh`
// over, the bank's weights and layouts are uploaded, and every agent is
// restarted under the source's rule: the body of rcw_reset(h, NULL, <the handle's seed>) with the source's kernel forced for every agent.
int install_layout_source(rcw_handle* h, LayoutSource& fresh)
{
    LayoutSource& ls = h->source;
    SnapshotShape sh = snapshot_shape(h);
    sh.source_kind = fresh.dev.kind;
    AgentArrays list;
    agent_arrays(sh, kFeatSource, &list);
    LiveArray at[kSnapFieldCount] = {};
    size_t agent_bytes = 0;
    const hipError_t e = alloc_parts(h, fresh.agents, list, 0, list.n, 0, at, &agent_bytes);
    if (e != hipSuccess) return fail(hip_code(e), "%s: %s", kSourceWords[fresh.dev.kind].name, hip_failure(e));
    RCW_HIP(take_live(h, kFeatSource, at));
    ls = std::move(fresh);
    RcwWallBank& v = ls.dev.agents;
    v.words = ls.words.get<uint32_t>(); v.cum = ls.cum.get<uint32_t>();
    v.last_episode = at[kSnapSourceLast].as<uint32_t>(); v.status_seen = at[kSnapSourceStatus].as<int32_t>();
    v.layout = at[kSnapSourceLayout].as<int32_t>(); v.mask = at[kSnapSourceMask].as<uint8_t>();
    const size_t B = (size_t)h->B;
    if (ls.is(kLayoutBank)) {                                          // (the weights wait in h_cum, the layouts in d_in_walls)
        RCW_HIP(hipMemcpyAsync(ls.cum.get(), ls.h_cum.get(), (size_t)v.layouts * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        RCW_HIP(hipEventRecord(ls.ev_cum.get(), h->stream));
        RCW_HIP(rcw_launch_wall_bank_pack(h->dev, h->d_in_walls.get<uint8_t>(), ls.words.get<uint32_t>(), v.layouts, h->stream));
    }
    RCW_HIP(hipMemsetAsync(ls.agents.get(), 0, agent_bytes, h->stream));
    RCW_HIP(hipMemcpyAsync(v.status_seen, h->d_status.get(), B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    h->step.reset(false, false, h->dev.auto_reset != 0);
    RCW_HIP(rcw_launch_reset(h->dev, nullptr, h->stream));             // the counters move by one ...
    RCW_HIP(launch_layout_source(h, true));                            // ... and every agent starts that episode on a layout of the source
    RCW_HIP(launch_start_distance(h, true));
    RCW_HIP(launch_step(h, nullptr, nullptr, kStackRefill));
    return RCW_OK;
}

}  // namespace
}  // extern "C++"

// Wall layouts (include/rcw.h): validate on the host, stage layouts and index, write the (masked) agents' WALL layer — and from there on the
// body of rcw_reset with the handle's own seed: no step fact moves that a reset with the same seed would not move.
int rcw_set_walls(rcw_handle* h, const uint8_t* walls_host, int32_t layouts, const int32_t* layout_index_host, const uint8_t* mask_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = refuse_other_source(h, "rcw_set_walls", kLayoutNone); if (rc) return rc;
    const int H = h->cfg.height_tile_map_tu, W = h->cfg.width_tile_map_tu;
    char why[256];
    if (validate_walls(H, W, h->B, walls_host, layouts, layout_index_host, mask_host, why, sizeof why) != RCW_OK)
        return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_set_walls: %s", why);
    const size_t B = (size_t)h->B, bytes = (size_t)layouts * (size_t)H * (size_t)W;
    std::vector<int32_t> index;
    try {
        index.resize(B);
    } catch (const std::bad_alloc&) {
        return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the layout index failed");
    }
    // (an agent outside the mask takes no layout: its entry is never read, and a stray value of the caller's must not reach the device)
    for (size_t a = 0; a < B; ++a) {
        const bool in = !mask_host || mask_host[a];
        index[a] = !in ? 0 : (layout_index_host ? layout_index_host[a] : (layouts == 1 ? 0 : (int32_t)a));
    }
    if (bytes > h->in_walls_cap) {
        RcwBuf larger; RCW_HIP(larger.hipMalloc(bytes));
        RCW_HIP(replace_buffers(h, {&h->d_in_walls}, {&larger}));
        h->in_walls_cap = bytes;
    }
    if (!h->d_in_wall_index.get()) RCW_HIP(h->d_in_wall_index.hipMalloc(B * sizeof(int32_t)));
    const uint8_t* mask_dev = nullptr;
    rc = upload_mask(h, mask_host, &mask_dev); if (rc) return rc;
    RCW_HIP(hipMemcpyAsync(h->d_in_walls.get(), walls_host, bytes, hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipMemcpyAsync(h->d_in_wall_index.get(), index.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipStreamSynchronize(h->stream));                          // (pageable host memory, the caller's and ours)
    h->step.reset(mask_dev != nullptr, false, h->dev.auto_reset != 0);
    RCW_HIP(rcw_launch_set_walls(h->dev, h->d_in_walls.get<uint8_t>(), h->d_in_wall_index.get<int32_t>(), mask_dev, h->stream));
    RCW_HIP(rcw_launch_reset(h->dev, mask_dev, h->stream));            // SR:110-132 against the new walls
    RCW_HIP(launch_start_distance(h, false));
    RCW_HIP(launch_step(h, nullptr, mask_dev, kStackRefill));          // SR:134, SR:329
    return RCW_OK;
}

extern "C++" {
template <typename T>
int set_state_impl(rcw_handle* h, const int32_t* goal_ij, const T* position_wu, const int32_t* direction_au,
                   const uint8_t* mask_host)
{
    if (!goal_ij || !position_wu || !direction_au) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL state array");
    const int H = h->cfg.height_tile_map_tu, W = h->cfg.width_tile_map_tu;
    for (int32_t a = 0; a < h->B; ++a) {
        if (mask_host && !mask_host[a]) continue;
        const int gi = goal_ij[2 * a], gj = goal_ij[2 * a + 1];
        if (gi < 2 || gi > H - 1 || gj < 2 || gj > W - 1)   // rand(2:H-1), rand(2:W-1) SR:120
            return fail(RCW_ERR_INVALID_ARGUMENT, "agent %d: goal (%d,%d) not an interior tile", a, gi, gj);
        if (direction_au[a] < 0 || direction_au[a] >= h->cfg.num_directions)
            return fail(RCW_ERR_INVALID_ARGUMENT, "agent %d: direction %d not in 0..%d", a, direction_au[a], h->cfg.num_directions - 1);
        const T x = position_wu[2 * a], y = position_wu[2 * a + 1];
        if (!(std::isfinite(x) && std::isfinite(y) && x >= (T)1 && x < (T)(H - 1) && y >= (T)1 && y < (T)(W - 1)))
            return fail(RCW_ERR_INVALID_ARGUMENT, "agent %d: position (%g,%g) not inside the room", a, (double)x, (double)y);
    }
    const uint8_t* mask_dev = nullptr;
    int rc = upload_mask(h, mask_host, &mask_dev); if (rc) return rc;
    const size_t B = (size_t)h->B;
    RCW_HIP(hipMemcpyAsync(h->d_in_goal.get(), goal_ij, B * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipMemcpyAsync(h->d_in_pos.get(), position_wu, B * 2 * sizeof(T), hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipMemcpyAsync(h->d_in_dir.get(), direction_au, B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipStreamSynchronize(h->stream));
    RCW_HIP(rcw_launch_set_state(h->dev, h->d_in_goal.get<int2>(), h->d_in_pos.get(), h->d_in_dir.get<int32_t>(), mask_dev,
                                 h->stream));
    RCW_HIP(launch_step(h, nullptr, mask_dev, kStackRefill));
    return RCW_OK;
}
}  // extern "C++"

int rcw_set_state(rcw_handle* h, const int32_t* goal_ij, const float* position_wu,
                  const int32_t* direction_au, const uint8_t* mask_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, false, "rcw_set_state"); if (rc) return rc;
    return set_state_impl<float>(h, goal_ij, position_wu, direction_au, mask_host);
}
int rcw_set_state64(rcw_handle* h, const int32_t* goal_ij, const double* position_wu,
                    const int32_t* direction_au, const uint8_t* mask_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, true, "rcw_set_state64"); if (rc) return rc;
    return set_state_impl<double>(h, goal_ij, position_wu, direction_au, mask_host);
}

int rcw_step(rcw_handle* h, const uint8_t* actions_host)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!actions_host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL actions");
    for (int32_t a = 0; a < h->B; ++a)   // @assert action in Base.OneTo(NUM_ACTIONS) SR:140
        if (actions_host[a] < 1 || actions_host[a] > RCW_NUM_ACTIONS)
            return fail(RCW_ERR_INVALID_ACTION, "Invalid action: %d (agent %d)", (int)actions_host[a], a);
    // Stage through a pinned ring so the caller may reuse its buffer at once and the host
    // can run one step ahead of the GPU; the copy is ordered on the stream behind the
    // previous step, which is still reading d_actions.
    const int slot = h->action_slot;
    h->action_slot ^= 1;
    RCW_HIP(hipEventSynchronize(h->ev_actions[slot].get()));
    std::memcpy(h->h_actions[slot].get(), actions_host, (size_t)h->B);
    RCW_HIP(hipMemcpyAsync(h->d_actions.get(), h->h_actions[slot].get(), (size_t)h->B, hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipEventRecord(h->ev_actions[slot].get(), h->stream));
    RCW_HIP(launch_step(h, h->d_actions.get<uint8_t>(), nullptr, kStackPush));
    return RCW_OK;
}

int rcw_step_device(rcw_handle* h, const uint8_t* actions_device)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!actions_device) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL actions");
    RCW_HIP(launch_step(h, actions_device, nullptr, kStackPush));
    return RCW_OK;
}

// The episode time limit (include/rcw.h).  The limit itself is a kernel argument (dev.limit.max_steps): a step takes the *_limit_kernel
// instantiations while it is > 0 and the plain kernels otherwise; the counters count from this call.
int rcw_set_time_limit(rcw_handle* h, int32_t max_episode_steps)
{
    int rc = check_handle(h); if (rc) return rc;
    if (max_episode_steps < 0) return fail(RCW_ERR_INVALID_ARGUMENT, "max_episode_steps must be >= 0 (0: no limit; got %d)", max_episode_steps);
    RCW_HIP(hipMemsetAsync(h->d_episode_steps.get(), 0, (size_t)h->B * sizeof(uint32_t), h->stream));
    RCW_HIP(hipMemsetAsync(h->d_truncated.get(), 0, (size_t)h->B, h->stream));
    h->dev.limit.max_steps = max_episode_steps;
    h->step.time_limit_set();
    return RCW_OK;
}

int rcw_time_limit(rcw_handle* h, int32_t* out)
{
    if (!h || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = h->dev.limit.max_steps; return RCW_OK;
}

int rcw_cast_rays(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    RCW_HIP(rcw_launch_cast(h->dev, nullptr, nullptr, h->stream));   // no action: rays + descriptors only
    h->step.columns_cast();
    return RCW_OK;
}

int rcw_update_camera_view(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    h->step.obs_unknown();
    rc = ensure_columns(h); if (rc) return rc;
    RCW_HIP(paint_camera(h, nullptr, h->stream));
    h->step.camera_repainted();
    return RCW_OK;
}

int rcw_update_top_view(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!h->d_top_view.get()) return fail(RCW_ERR_UNSUPPORTED, "handle was created with render_top_view = 0");
    RCW_HIP(launch_top_view_alone(h, nullptr));
    return RCW_OK;
}

int rcw_sync(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    return sync_and_check(h);
}

int rcw_clear_error(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    RCW_HIP(hipMemsetAsync(h->d_err.get(), 0, sizeof(int32_t), h->stream));
    RCW_HIP(hipMemsetAsync(h->d_status.get(), 0, (size_t)h->B * sizeof(int32_t), h->stream));
    if (h->source.live()) RCW_HIP(hipMemsetAsync(h->source.dev.agents.status_seen, 0, (size_t)h->B * sizeof(int32_t), h->stream));   // (the layout source's record of them)
    RCW_HIP(hipStreamSynchronize(h->stream));
    return RCW_OK;
}

int rcw_obs_device_ptr(rcw_handle* h, void** device_ptr)
{
    if (!h || !device_ptr) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *device_ptr = h->dev.obs;
    return RCW_OK;
}

int rcw_obs_copy(rcw_handle* h, uint32_t* out_host, int32_t first, int32_t count)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_range(h, out_host != nullptr, first, count); if (rc) return rc;
    rc = sync_and_check(h);
    const size_t frame = (size_t)h->cfg.num_rays * h->cfg.height_camera_view_pu;
    RCW_HIP(hipMemcpy(out_host, h->dev.obs + (size_t)first * frame, (size_t)count * frame * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    return rc;
}

int rcw_top_view_device_ptr(rcw_handle* h, void** device_ptr)
{
    if (!h || !device_ptr) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!h->d_top_view.get()) return fail(RCW_ERR_UNSUPPORTED, "handle was created with render_top_view = 0");
    *device_ptr = h->d_top_view.get();
    return RCW_OK;
}

int rcw_top_view_copy(rcw_handle* h, uint32_t* out_host, int32_t first, int32_t count)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!h->d_top_view.get()) return fail(RCW_ERR_UNSUPPORTED, "handle was created with render_top_view = 0");
    rc = check_range(h, out_host != nullptr, first, count); if (rc) return rc;
    rc = sync_and_check(h);
    const size_t frame = (size_t)h->cfg.height_tile_map_tu * h->cfg.width_tile_map_tu * h->cfg.pu_per_tu * h->cfg.pu_per_tu;
    RCW_HIP(hipMemcpy(out_host, h->d_top_view.get<uint32_t>() + (size_t)first * frame, (size_t)count * frame * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    return rc;
}

int rcw_reward(rcw_handle* h, float* out)
{
    int rc = check_handle(h); if (rc) return rc;
    if (h->cfg.reward_type != RCW_REWARD_FLOAT32)
        return fail(RCW_ERR_UNSUPPORTED, "rcw_reward: the handle's reward type is not Float32; use rcw_reward_typed");
    return copy_arrays(h, nullptr, {{out, kSnapReward}});
}
int rcw_reward_typed(rcw_handle* h, void* out) { int rc = check_handle(h); if (rc) return rc; return copy_arrays(h, nullptr, {{out, kSnapReward}}); }
int rcw_done(rcw_handle* h, uint8_t* out) { int rc = check_handle(h); if (rc) return rc; return copy_arrays(h, nullptr, {{out, kSnapDone}}); }
int rcw_position(rcw_handle* h, float* out)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, false, "rcw_position"); if (rc) return rc;
    return copy_arrays(h, nullptr, {{out, kSnapPos}});
}
int rcw_position64(rcw_handle* h, double* out)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, true, "rcw_position64"); if (rc) return rc;
    return copy_arrays(h, nullptr, {{out, kSnapPos}});
}
int rcw_direction(rcw_handle* h, int32_t* out) { int rc = check_handle(h); if (rc) return rc; return copy_arrays(h, nullptr, {{out, kSnapDir}}); }
int rcw_goal(rcw_handle* h, int32_t* out) { int rc = check_handle(h); if (rc) return rc; return copy_arrays(h, nullptr, {{out, kSnapGoal}}); }
int rcw_episode(rcw_handle* h, uint32_t* out) { int rc = check_handle(h); if (rc) return rc; return copy_arrays(h, nullptr, {{out, kSnapEpisode}}); }
int rcw_episode_steps(rcw_handle* h, uint32_t* out) { int rc = check_handle(h); if (rc) return rc; return copy_arrays(h, nullptr, {{out, kSnapEpisodeSteps}}); }
int rcw_truncated(rcw_handle* h, uint8_t* out) { int rc = check_handle(h); if (rc) return rc; return copy_arrays(h, nullptr, {{out, kSnapTruncated}}); }

int rcw_status(rcw_handle* h, int32_t* out)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL output pointer");
    RCW_HIP(hipStreamSynchronize(h->stream));
    RCW_HIP(hipMemcpy(out, h->d_status.get(), (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RCW_OK;
}

int rcw_reward_device_ptr(rcw_handle* h, void** p) { return hand_out(h, nullptr, {{p, kSnapReward}}); }
int rcw_done_device_ptr(rcw_handle* h, void** p) { return hand_out(h, nullptr, {{p, kSnapDone}}); }
int rcw_episode_steps_device_ptr(rcw_handle* h, void** p) { return hand_out(h, nullptr, {{p, kSnapEpisodeSteps}}); }
int rcw_truncated_device_ptr(rcw_handle* h, void** p) { return hand_out(h, nullptr, {{p, kSnapTruncated}}); }

int rcw_tile_map_num_chunks(rcw_handle* h, int32_t* out)
{
    if (!h || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = h->nchunks; return RCW_OK;
}
int rcw_tile_map_chunks(rcw_handle* h, uint64_t* out)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, nullptr, {{out, kSnapTileMap}});
}

extern "C++" {
template <typename T>
int rays_impl(rcw_handle* h, int32_t first, int32_t count, int64_t* stop_ij, int64_t* hit_dimension,
              T* distance_wu, T* directions_wu)
{
    int rc = check_range(h, true, first, count, 1); if (rc) return rc;
    const size_t n = (size_t)count * h->cfg.num_rays;
    RcwRayOut out{};
    // device scratch lives in the handle and only ever grows: no hipMalloc/hipFree per call
    const size_t want[4] = {stop_ij ? 2 * n * sizeof(int64_t) : 0, hit_dimension ? n * sizeof(int64_t) : 0,
                            distance_wu ? n * sizeof(T) : 0, directions_wu ? 2 * n * sizeof(T) : 0};
    for (int k = 0; k < 4; ++k) {
        if (want[k] <= h->rays_cap[k]) continue;
        RcwBuf larger; RCW_HIP(larger.hipMalloc(want[k]));
        RCW_HIP(replace_buffers(h, {&h->d_rays[k]}, {&larger}));
        h->rays_cap[k] = want[k];
    }
    if (stop_ij) out.stop_ij = h->d_rays[0].get<int64_t>();
    if (hit_dimension) out.hit_dim = h->d_rays[1].get<int64_t>();
    if (distance_wu) out.dist = h->d_rays[2].get();
    if (directions_wu) out.dirs = h->d_rays[3].get();
    RCW_HIP(rcw_launch_rays(h->dev, first, count, out, h->stream));
    RCW_HIP(hipStreamSynchronize(h->stream));
    if (stop_ij) RCW_HIP(hipMemcpy(stop_ij, h->d_rays[0].get(), want[0], hipMemcpyDeviceToHost));
    if (hit_dimension) RCW_HIP(hipMemcpy(hit_dimension, h->d_rays[1].get(), want[1], hipMemcpyDeviceToHost));
    if (distance_wu) RCW_HIP(hipMemcpy(distance_wu, h->d_rays[2].get(), want[2], hipMemcpyDeviceToHost));
    if (directions_wu) RCW_HIP(hipMemcpy(directions_wu, h->d_rays[3].get(), want[3], hipMemcpyDeviceToHost));
    return RCW_OK;
}
}  // extern "C++"

int rcw_rays(rcw_handle* h, int32_t first, int32_t count, int64_t* stop_ij, int64_t* hit_dimension,
             float* distance_wu, float* directions_wu)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, false, "rcw_rays"); if (rc) return rc;
    return rays_impl<float>(h, first, count, stop_ij, hit_dimension, distance_wu, directions_wu);
}
int rcw_rays64(rcw_handle* h, int32_t first, int32_t count, int64_t* stop_ij, int64_t* hit_dimension,
               double* distance_wu, double* directions_wu)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_real(h, true, "rcw_rays64"); if (rc) return rc;
    return rays_impl<double>(h, first, count, stop_ij, hit_dimension, distance_wu, directions_wu);
}

int rcw_columns(rcw_handle* h, int32_t first, int32_t count, int32_t* height_line_pu, uint8_t* colour_id)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = check_range(h, true, first, count); if (rc) return rc;
    rc = ensure_columns(h); if (rc) return rc;
    rc = sync_and_check(h);
    const size_t N = (size_t)h->cfg.num_rays;
    if (height_line_pu)
        RCW_HIP(hipMemcpy(height_line_pu, h->d_col_h.get<int32_t>() + (size_t)first * N, (size_t)count * N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (colour_id)
        RCW_HIP(hipMemcpy(colour_id, h->d_col_c.get<uint8_t>() + (size_t)first * N, (size_t)count * N, hipMemcpyDeviceToHost));
    return rc;
}

int rcw_columns_device_ptr(rcw_handle* h, void** height_line_pu, void** colour_id)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL handle");
    {   // from now on every step refreshes the descriptors (the caller reads them through the pointers, behind the library's back)
        int rc = check_handle(h); if (rc) return rc;
        h->step.columns_wanted();
        rc = ensure_columns(h); if (rc) return rc;
    }
    if (height_line_pu) *height_line_pu = h->d_col_h.get();
    if (colour_id) *colour_id = h->d_col_c.get();
    return RCW_OK;
}

int rcw_expand_columns(rcw_handle* h, const int32_t* height_line_pu_device, const uint8_t* colour_id_device,
                       int32_t count, void* frames_device)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!height_line_pu_device || !colour_id_device || !frames_device || count < 1)
        return fail(RCW_ERR_INVALID_ARGUMENT, "bad argument");
    if ((uintptr_t)frames_device & 15u) return fail(RCW_ERR_INVALID_ARGUMENT, "frames must be 16-byte aligned");
    RCW_HIP(rcw_launch_expand(h->dev, height_line_pu_device, colour_id_device, count, (uint32_t*)frames_device, h->stream));
    return RCW_OK;
}

// ---- the learner view ---------------------------------------------------------------------------------------
int rcw_set_learner_view(rcw_handle* h, int32_t format, int32_t layout, int32_t height, int32_t width, int32_t flags)
{
    return rcw_set_learner_view_stack(h, format, layout, height, width, flags, 1);
}

int rcw_set_learner_view_stack(rcw_handle* h, int32_t format, int32_t layout, int32_t height, int32_t width, int32_t flags, int32_t frames)
{
    int rc = check_handle(h); if (rc) return rc;
    ViewPlan plan;
    rc = plan_learner_view(h->cfg, h->dev, format, layout, height, width, flags, frames, &plan); if (rc) return rc;
    rcw_handle::LearnerView& lv = h->learner;
    const bool was_only = lv.only();
    rcw_handle::LearnerView fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (format != RCW_VIEW_OFF) {
        fresh.set = {format, layout, height, width, flags, frames};
        fresh.view = plan.v;
        SnapshotShape sh = snapshot_shape(h);
        sh.view_fmt = format; sh.view_layout = layout; sh.view_C = plan.v.C; sh.view_h = height; sh.view_w = width; sh.view_frames = frames;
        AgentArrays list;                                          // the stack, its counter, the kernels' frame — or that frame alone; head: the box tables
        agent_arrays(sh, kFeatView, &list);
        hipError_t e = list.head == plan.tab.size() * sizeof(int32_t) ? alloc_parts(h, fresh.frame, list, list.n - 1, 1, 0, at) : hipErrorInvalidValue;
        if (e == hipSuccess) e = fresh.tab.hipMalloc((size_t)list.head);
        if (e == hipSuccess) e = hipMemcpy(fresh.tab.get(), plan.tab.data(), (size_t)list.head, hipMemcpyHostToDevice);
        if (e == hipSuccess && frames > 1) e = alloc_parts(h, fresh.stack, list, 0, 1, 0, at);
        if (e == hipSuccess && frames > 1) e = alloc_parts(h, fresh.last_episode, list, 1, 1, 0, at);
        if (e != hipSuccess)                                       // the handle keeps its previous view
            return fail(hip_code(e), "learner view buffer of %zu bytes: %s", (size_t)h->B * list.part[0].bytes, hip_failure(e));
        fresh.view.rows = fresh.tab.get<int32_t>();
        fresh.view.cols = fresh.tab.get<int32_t>() + height + 1;
        fresh.view.dsum = plan.v.depth ? fresh.tab.get<int32_t>() + height + width + 2 : nullptr;
    }
    RCW_HIP(take_live(h, kFeatView, at));                          // (the new view, or none: the view switched off)
    lv = std::move(fresh);
    if (lv.on()) {
        // the view kernel reads the descriptors: every step of the handle refreshes them from now on (as for rcw_columns_device_ptr)
        h->step.columns_wanted();
        rc = ensure_columns(h); if (rc) return rc;
    }
    if (lv.only()) {                                              // (a caller's one-launch request gives way: the step has no camera fill)
        rc = plan_step_form(h, h->step.want() == RCW_STEP_ONE_LAUNCH ? 0 : h->step.want()); if (rc) return rc;
    }
    else if (was_only) {                                          // back to the camera view in the step: its form by the rule, its frames now
        rc = plan_step_form(h, h->step.want()); if (rc) return rc;
        RCW_HIP(paint_camera(h, nullptr, h->stream));
    }
    if (lv.on()) RCW_HIP(launch_view(h, nullptr, kStackRefill));
    return RCW_OK;
}

int rcw_learner_view_stack(rcw_handle* h, int32_t* frames)
{
    if (!h || !frames) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *frames = h->learner.set.frames;
    return RCW_OK;
}

int rcw_learner_view_info(rcw_handle* h, int32_t* format, int32_t* layout, int32_t* height, int32_t* width, int32_t* flags)
{
    if (!h || !format || !layout || !height || !width || !flags) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const auto& set = h->learner.set;
    *format = set.fmt; *layout = set.layout; *height = set.h; *width = set.w; *flags = set.flags;
    return RCW_OK;
}

int rcw_learner_view_device_ptr(rcw_handle* h, void** device_ptr) { return hand_out(h, kNoLearnerView, {{device_ptr, view_id(h)}}); }

int rcw_learner_view_copy(rcw_handle* h, uint8_t* out_host, int32_t first, int32_t count)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoLearnerView, {{out_host, view_id(h)}}, true, first, count);
}

// The goal distance (include/rcw.h).  Enabling allocates and floods every agent at once, stream-ordered behind what is queued; enabling
// again does the same again; an allocation failure leaves what was there.  The guide lives on the field: switching the goal distance off
// switches the guide off first, enabling it again rewrites the guide's words from the new field.
int rcw_set_goal_distance(rcw_handle* h, int32_t enable)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::GoalDistance& gd = h->goal;
    if (!enable && !gd.on()) return RCW_OK;
    if (!enable) { rc = rcw_set_guide(h, 0); if (rc) return rc; }
    rcw_handle::GoalDistance fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (enable) {
        SnapshotShape sh = snapshot_shape(h);
        sh.goal = 1;
        AgentArrays list;                                          // the field | the three words | the counter: a buffer each
        agent_arrays(sh, kFeatGoal, &list);
        size_t bytes = 0;
        hipError_t e = alloc_parts(h, fresh.field, list, 0, 1, 0, at, &bytes);
        if (e == hipSuccess) e = alloc_parts(h, fresh.word_buf, list, 1, 3, 0, at);
        if (e == hipSuccess) e = alloc_parts(h, fresh.last_episode, list, 4, 1, 0, at);
        if (e != hipSuccess) return fail(hip_code(e), "goal distance field of %zu bytes: %s", bytes, hip_failure(e));
        fresh.words = RcwGoalWords{at[kSnapGoalDistance].as<int32_t>(), at[kSnapGoalStart].as<int32_t>(), at[kSnapGoalProgress].as<int32_t>()};
    }
    RCW_HIP(take_live(h, kFeatGoal, at));
    gd = std::move(fresh);
    if (gd.on()) RCW_HIP(launch_goal_distance(h, nullptr, kStackRefill));
    if (gd.on()) RCW_HIP(launch_guide(h, kStackRefill));
    return RCW_OK;
}

int rcw_goal_distance_enabled(rcw_handle* h, int32_t* out)
{
    if (!h || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = h->goal.on() ? 1 : 0;
    return RCW_OK;
}

int rcw_goal_distance(rcw_handle* h, int32_t* distance, int32_t* start_distance, int32_t* progress)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoGoalDistance, {{distance, kSnapGoalDistance}, {start_distance, kSnapGoalStart}, {progress, kSnapGoalProgress}});
}

int rcw_goal_distance_device_ptr(rcw_handle* h, void** distance, void** start_distance, void** progress)
{
    return hand_out(h, kNoGoalDistance, {{distance, kSnapGoalDistance}, {start_distance, kSnapGoalStart}, {progress, kSnapGoalProgress}});
}

int rcw_goal_distance_field(rcw_handle* h, int32_t first, int32_t count, void* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoGoalDistance, {{out_host, kSnapGoalField}}, true, first, count);
}

int rcw_goal_distance_field_device_ptr(rcw_handle* h, void** ptr) { return hand_out(h, kNoGoalDistance, {{ptr, kSnapGoalField}}); }

// The guide (include/rcw.h).  Enabling allocates and computes every agent's words at once, stream-ordered behind what is queued; enabling
// again does the same again; an allocation failure leaves what was there.
int rcw_set_guide(rcw_handle* h, int32_t enable)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::Guide& gu = h->guide;
    if (!enable && !gu.on()) return RCW_OK;
    if (enable) { rc = need(h->goal.on(), "the guide follows the goal distance's field: enable it first (rcw_set_goal_distance(h, 1))"); if (rc) return rc; }
    rcw_handle::Guide fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (enable) {
        SnapshotShape sh = snapshot_shape(h);
        sh.guide = 1;
        AgentArrays list;
        agent_arrays(sh, kFeatGuide, &list);
        size_t bytes = 0;
        const hipError_t e = alloc_parts(h, fresh.buf, list, 0, list.n, list.head, at, &bytes);
        if (e != hipSuccess) return fail(hip_code(e), "guide words of %zu bytes: %s", bytes, hip_failure(e));
        fresh.words = RcwGuideWords{at[kSnapGuideAction].as<uint8_t>(), at[kSnapGuideHeading].as<int32_t>()};
    }
    RCW_HIP(take_live(h, kFeatGuide, at));
    gu = std::move(fresh);
    if (gu.on()) RCW_HIP(launch_guide(h, kStackRefill));
    return RCW_OK;
}

int rcw_guide_info(rcw_handle* h, int32_t* enabled, int32_t* promised)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (enabled) *enabled = h->guide.on() ? 1 : 0;
    if (promised) *promised = guide_promised(h->cfg);
    return RCW_OK;
}

int rcw_guide(rcw_handle* h, uint8_t* action, int32_t* heading)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoGuide, {{action, kSnapGuideAction}, {heading, kSnapGuideHeading}});
}

int rcw_guide_device_ptr(rcw_handle* h, void** action, void** heading)
{
    return hand_out(h, kNoGuide, {{action, kSnapGuideAction}, {heading, kSnapGuideHeading}});
}

// The seen map (include/rcw.h).  Enabling allocates and marks every agent afresh at once, stream-ordered behind what is queued; enabling
// again does the same again; an allocation failure leaves what was there.
int rcw_set_seen_map(rcw_handle* h, int32_t enable)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::SeenMap& sm = h->seen;
    if (!enable && !sm.on()) return RCW_OK;
    if (!enable && h->local.source == RCW_LOCAL_SEEN)
        return fail(RCW_ERR_UNSUPPORTED, "the handle's local map reads the seen map: switch the local map off first (rcw_set_local_map)");
    if (!enable && h->frontier.on())
        return fail(RCW_ERR_UNSUPPORTED, "the handle's frontier floods over the seen map: switch the frontier off first (rcw_set_frontier(h, 0))");
    rcw_handle::SeenMap fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (enable) {
        SnapshotShape sh = snapshot_shape(h);
        sh.seen = 1;
        AgentArrays list;
        agent_arrays(sh, kFeatSeen, &list);
        size_t bytes = 0;
        const hipError_t e = alloc_parts(h, fresh.buf, list, 0, list.n, 0, at, &bytes);
        if (e != hipSuccess) return fail(hip_code(e), "seen map of %zu bytes: %s", bytes, hip_failure(e));
        fresh.words = RcwSeenWords{at[kSnapSeenCount].as<int32_t>(), at[kSnapSeenNew].as<int32_t>(), at[kSnapSeenGoal].as<int32_t>()};
        fresh.last_episode = at[kSnapSeenLast].as<uint32_t>();
        fresh.bits = at[kSnapSeenBits].as<uint32_t>();
        fresh.map = at[kSnapSeenMap].as<uint8_t>();
    }
    RCW_HIP(take_live(h, kFeatSeen, at));
    sm = std::move(fresh);
    if (sm.on()) RCW_HIP(launch_seen_map(h, nullptr, kStackRefill));
    if (sm.on()) RCW_HIP(launch_frontier(h, nullptr, kStackRefill));
    if (sm.on()) RCW_HIP(launch_local_map(h, kStackRefill));
    return RCW_OK;
}

int rcw_seen_map_enabled(rcw_handle* h, int32_t* out)
{
    if (!h || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = h->seen.on() ? 1 : 0;
    return RCW_OK;
}

int rcw_seen_words(rcw_handle* h, int32_t* seen_count, int32_t* newly_seen, int32_t* goal_seen)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoSeenMap, {{seen_count, kSnapSeenCount}, {newly_seen, kSnapSeenNew}, {goal_seen, kSnapSeenGoal}});
}

int rcw_seen_words_device_ptr(rcw_handle* h, void** seen_count, void** newly_seen, void** goal_seen)
{
    return hand_out(h, kNoSeenMap, {{seen_count, kSnapSeenCount}, {newly_seen, kSnapSeenNew}, {goal_seen, kSnapSeenGoal}});
}

int rcw_seen_map(rcw_handle* h, int32_t first, int32_t count, void* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoSeenMap, {{out_host, kSnapSeenMap}}, true, first, count);
}

int rcw_seen_map_device_ptr(rcw_handle* h, void** ptr) { return hand_out(h, kNoSeenMap, {{ptr, kSnapSeenMap}}); }

// The frontier (include/rcw.h).  Enabling allocates and floods every agent at once, stream-ordered behind what is queued; enabling again
// does the same again; an allocation failure leaves what was there.
int rcw_set_frontier(rcw_handle* h, int32_t enable)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::Frontier& fr = h->frontier;
    if (!enable && !fr.on()) return RCW_OK;
    if (enable) { rc = need(h->seen.on(), "the frontier floods over the seen map: enable it first (rcw_set_seen_map(h, 1))"); if (rc) return rc; }
    if (enable && (int64_t)h->dev.H * h->dev.W > 65535) return fail(RCW_ERR_UNSUPPORTED, "the frontier's field holds UInt16 tile indices: a map of %d x %d is too large", h->dev.H, h->dev.W);
    rcw_handle::Frontier fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (enable) {
        SnapshotShape sh = snapshot_shape(h);
        sh.frontier = 1;
        AgentArrays list;
        agent_arrays(sh, kFeatFrontier, &list);
        size_t bytes = 0;
        const hipError_t e = alloc_parts(h, fresh.buf, list, 0, list.n, list.head, at, &bytes);
        if (e != hipSuccess) return fail(hip_code(e), "frontier of %zu bytes: %s", bytes, hip_failure(e));
        fresh.words = RcwFrontierWords{at[kSnapFrontierDistance].as<int32_t>(), at[kSnapFrontierTiles].as<int32_t>()};
        fresh.advice = RcwGuideWords{at[kSnapFrontierAction].as<uint8_t>(), at[kSnapFrontierHeading].as<int32_t>()};
        fresh.last_episode = at[kSnapFrontierLast].as<uint32_t>();
        fresh.field = at[kSnapFrontierField].as<uint16_t>();
    }
    RCW_HIP(take_live(h, kFeatFrontier, at));
    fr = std::move(fresh);
    if (fr.on()) RCW_HIP(launch_frontier(h, nullptr, kStackRefill));
    return RCW_OK;
}

int rcw_frontier_info(rcw_handle* h, int32_t* enabled)
{
    if (!h || !enabled) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *enabled = h->frontier.on() ? 1 : 0;
    return RCW_OK;
}

int rcw_frontier(rcw_handle* h, int32_t* distance, int32_t* tiles, uint8_t* action, int32_t* heading)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoFrontier, {{distance, kSnapFrontierDistance}, {tiles, kSnapFrontierTiles}, {action, kSnapFrontierAction}, {heading, kSnapFrontierHeading}});
}

int rcw_frontier_device_ptr(rcw_handle* h, void** distance, void** tiles, void** action, void** heading)
{
    return hand_out(h, kNoFrontier, {{distance, kSnapFrontierDistance}, {tiles, kSnapFrontierTiles}, {action, kSnapFrontierAction}, {heading, kSnapFrontierHeading}});
}

int rcw_frontier_field(rcw_handle* h, int32_t first, int32_t count, void* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoFrontier, {{out_host, kSnapFrontierField}}, true, first, count);
}

int rcw_frontier_field_device_ptr(rcw_handle* h, void** ptr) { return hand_out(h, kNoFrontier, {{ptr, kSnapFrontierField}}); }

// The local map (include/rcw.h).  Enabling allocates and computes every agent's image at once, stream-ordered behind what is queued; new
// parameters replace the old; an allocation failure leaves what was there.
int rcw_set_local_map(rcw_handle* h, int32_t source, int32_t size, int32_t cells_per_tile)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::LocalMap& lm = h->local;
    std::vector<unsigned char> table;
    rc = plan_local_map(source, size, cells_per_tile, h->real64, &table); if (rc) return rc;
    if (source == RCW_LOCAL_SEEN && !h->seen.on())
        return fail(RCW_ERR_UNSUPPORTED, "RCW_LOCAL_SEEN needs the handle's seen map (rcw_set_seen_map)");
    if (source == 0 && !lm.on()) return RCW_OK;
    rcw_handle::LocalMap fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (source != 0) {
        SnapshotShape sh = snapshot_shape(h);
        sh.local_source = source; sh.local_size = size; sh.local_cells = cells_per_tile;
        AgentArrays list;                                          // head: the offset table
        agent_arrays(sh, kFeatLocal, &list);
        size_t bytes = 0;
        hipError_t e = list.head == table.size() ? alloc_parts(h, fresh.buf, list, 0, list.n, list.head, at, &bytes) : hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMemcpy(fresh.buf.get(), table.data(), table.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(hip_code(e), "local map of %zu bytes: %s", bytes, hip_failure(e));
        fresh.source = source; fresh.size = size; fresh.cells_per_tile = cells_per_tile;
        fresh.off = fresh.buf.get();
        fresh.img = at[kSnapLocalImage].as<uint8_t>();
    }
    RCW_HIP(take_live(h, kFeatLocal, at));
    lm = std::move(fresh);
    RCW_HIP(launch_local_map(h, kStackRefill));
    return RCW_OK;
}

int rcw_local_map_info(rcw_handle* h, int32_t* source, int32_t* size, int32_t* cells_per_tile)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (source) *source = h->local.source;
    if (size) *size = h->local.size;
    if (cells_per_tile) *cells_per_tile = h->local.cells_per_tile;
    return RCW_OK;
}

int rcw_local_map_device_ptr(rcw_handle* h, void** device_ptr) { return hand_out(h, kNoLocalMap, {{device_ptr, kSnapLocalImage}}); }

int rcw_local_map_copy(rcw_handle* h, uint8_t* out_host, int32_t first, int32_t count)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoLocalMap, {{out_host, kSnapLocalImage}}, true, first, count);
}

extern "C++" {
namespace {
// (the table's level rows were counted from the source that is live: it stays until the statistics are switched off)
int refuse_under_episode_stats(rcw_handle* h, const char* caller)
{
    if (h->visits.table()) return fail(RCW_ERR_UNSUPPORTED, "%s: the handle keeps a visit table, whose level rows follow the layout source; switch the visit map off first (rcw_set_visit_map(h, 0, 0, 0))", caller);
    return h->stats.on() ? fail(RCW_ERR_UNSUPPORTED, "%s: the handle keeps episode statistics, whose level rows follow the layout source; switch them off first (rcw_set_episode_stats(h, 0))", caller) : RCW_OK;
}
}  // namespace
}  // extern "C++"

// The wall bank (include/rcw.h): validated, allocated and its layouts staged before the install.
int rcw_set_wall_bank(rcw_handle* h, const uint8_t* walls_host, int32_t layouts, const uint32_t* weights_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = refuse_under_episode_stats(h, "rcw_set_wall_bank"); if (rc) return rc;
    if (layouts == 0 || !walls_host) return drop_layout_source(h, kLayoutBank);
    rc = refuse_other_source(h, "rcw_set_wall_bank", kLayoutBank); if (rc) return rc;
    const int H = h->cfg.height_tile_map_tu, W = h->cfg.width_tile_map_tu;
    char why[256];
    if (layouts < 0) return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_set_wall_bank: layouts must be >= 0 (got %d)", layouts);
    if (validate_walls(H, W, layouts, walls_host, layouts, nullptr, nullptr, why, sizeof why) != RCW_OK)   // (a layout each of `layouts` agents: every one is checked)
        return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_set_wall_bank: %s", why);
    const size_t L = (size_t)layouts, bytes = L * (size_t)H * (size_t)W, nwords = (size_t)h->dev.nwords;
    std::vector<uint32_t> cum;
    try { cum.resize(L); } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the cumulative weights failed"); }
    LayoutSource fresh;
    rc = plan_wall_bank_weights(weights_host, layouts, cum.data(), &fresh.total_weight); if (rc) return rc;
    {
        hipError_t e = fresh.words.hipMalloc(L * nwords * sizeof(uint32_t));
        if (e == hipSuccess) e = fresh.cum.hipMalloc(L * sizeof(uint32_t));
        if (e == hipSuccess) e = fresh.h_cum.hipHostMalloc(L * sizeof(uint32_t));
        if (e == hipSuccess) e = fresh.ev_cum.hipEventCreate(hipEventDisableTiming);
        if (e != hipSuccess) return fail(hip_code(e), "wall bank of %d layouts: %s", layouts, hip_failure(e));
    }
    if (bytes > h->in_walls_cap) {
        RcwBuf larger; RCW_HIP(larger.hipMalloc(bytes));
        RCW_HIP(replace_buffers(h, {&h->d_in_walls}, {&larger}));
        h->in_walls_cap = bytes;
    }
    RCW_HIP(hipMemcpyAsync(h->d_in_walls.get(), walls_host, bytes, hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipStreamSynchronize(h->stream));                          // (pageable host memory of the caller's)
    std::memcpy(fresh.h_cum.get(), cum.data(), L * sizeof(uint32_t));
    fresh.dev.kind = kLayoutBank;
    fresh.dev.agents.layouts = layouts;
    return install_layout_source(h, fresh);
}

// New weights for the installed bank, stream-ordered behind what is queued and without waiting for it: the cumulative weights travel through the
// bank's pinned buffer, whose previous copy the event guards.
int rcw_set_wall_bank_weights(rcw_handle* h, const uint32_t* weights_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need(h->source.is(kLayoutBank), "the handle has no wall bank (rcw_set_wall_bank)"); if (rc) return rc;
    LayoutSource& wb = h->source;
    const int32_t layouts = wb.dev.agents.layouts;
    const size_t L = (size_t)layouts;
    std::vector<uint32_t> cum;
    try { cum.resize(L); } catch (const std::bad_alloc&) { return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the cumulative weights failed"); }
    uint64_t total = 0;
    rc = plan_wall_bank_weights(weights_host, layouts, cum.data(), &total); if (rc) return rc;
    RCW_HIP(hipEventSynchronize(wb.ev_cum.get()));
    std::memcpy(wb.h_cum.get(), cum.data(), L * sizeof(uint32_t));
    RCW_HIP(hipMemcpyAsync(wb.cum.get(), wb.h_cum.get(), L * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    RCW_HIP(hipEventRecord(wb.ev_cum.get(), h->stream));
    wb.total_weight = total;
    return RCW_OK;
}

int rcw_wall_bank_info(rcw_handle* h, int32_t* layouts, uint64_t* total_weight)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (layouts) *layouts = h->source.dev.agents.layouts;              // (zeros while the bank is off: a family has no layouts and no weights)
    if (total_weight) *total_weight = h->source.total_weight;
    return RCW_OK;
}

int rcw_wall_layout(rcw_handle* h, int32_t* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoDrawnWalls, {{out_host, kSnapSourceLayout}});
}

int rcw_wall_layout_device_ptr(rcw_handle* h, void** device_ptr) { return hand_out(h, kNoDrawnWalls, {{device_ptr, kSnapSourceLayout}}); }

// The wall generator's mazes (include/rcw.h, "the wall generator").
int rcw_set_wall_generator(rcw_handle* h, int32_t enable, uint32_t loops, int32_t levels, int32_t first_level, uint64_t level_seed)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = refuse_under_episode_stats(h, "rcw_set_wall_generator"); if (rc) return rc;
    if (!enable) return drop_layout_source(h, kLayoutMazes);
    const int H = h->cfg.height_tile_map_tu, W = h->cfg.width_tile_map_tu;
    rc = plan_wall_generator(H, W, levels, first_level); if (rc) return rc;
    rc = refuse_other_source(h, "rcw_set_wall_generator", kLayoutMazes); if (rc) return rc;
    LayoutSource fresh;
    fresh.dev.kind = kLayoutMazes;
    fresh.dev.gen = RcwWallGen{loops, levels, first_level, level_seed, (H - 1) / 2, (W - 1) / 2};
    return install_layout_source(h, fresh);
}

// (any family: the level rule is the generator's, and loops is 0 while caves or rooms are live)
int rcw_wall_generator_info(rcw_handle* h, int32_t* enabled, uint32_t* loops, int32_t* levels, int32_t* first_level, uint64_t* level_seed)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const RcwWallGen& g = h->source.dev.gen;                           // (zeros while no family is live)
    if (enabled) *enabled = h->source.live() && !h->source.is(kLayoutBank) ? 1 : 0;
    if (loops) *loops = g.loops;
    if (levels) *levels = g.levels;
    if (first_level) *first_level = g.first_level;
    if (level_seed) *level_seed = g.level_seed;
    return RCW_OK;
}

// The caves (include/rcw.h, "the wall generator: caves"); the level rule also carries the fallback maze's grid (loops 0).
int rcw_set_wall_caves(rcw_handle* h, int32_t enable, uint32_t fill, int32_t smooth, int32_t levels, int32_t first_level, uint64_t level_seed)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = refuse_under_episode_stats(h, "rcw_set_wall_caves"); if (rc) return rc;
    if (!enable) return drop_layout_source(h, kLayoutCaves);
    const int H = h->cfg.height_tile_map_tu, W = h->cfg.width_tile_map_tu;
    rc = plan_wall_caves(H, W, smooth, levels, first_level); if (rc) return rc;
    rc = refuse_other_source(h, "rcw_set_wall_caves", kLayoutCaves); if (rc) return rc;
    LayoutSource fresh;
    fresh.dev.kind = kLayoutCaves;
    fresh.dev.gen = RcwWallGen{0u, levels, first_level, level_seed, (H - 1) / 2, (W - 1) / 2};
    fresh.dev.caves = RcwWallCaves{fill, smooth};
    return install_layout_source(h, fresh);
}

int rcw_wall_caves_info(rcw_handle* h, int32_t* enabled, uint32_t* fill, int32_t* smooth)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const RcwWallCaves& c = h->source.dev.caves;                       // (zeros while the caves are off)
    if (enabled) *enabled = h->source.is(kLayoutCaves) ? 1 : 0;
    if (fill) *fill = c.fill;
    if (smooth) *smooth = c.smooth;
    return RCW_OK;
}

// The rooms (include/rcw.h, "the wall generator: rooms"); the level rule alone (loops 0, no grid: rooms have no fallback maze).
int rcw_set_wall_rooms(rcw_handle* h, int32_t enable, int32_t room, uint32_t stop, uint32_t doors, int32_t levels, int32_t first_level, uint64_t level_seed)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = refuse_under_episode_stats(h, "rcw_set_wall_rooms"); if (rc) return rc;
    if (!enable) return drop_layout_source(h, kLayoutRooms);
    const int H = h->cfg.height_tile_map_tu, W = h->cfg.width_tile_map_tu;
    rc = plan_wall_rooms(H, W, room, levels, first_level); if (rc) return rc;
    rc = refuse_other_source(h, "rcw_set_wall_rooms", kLayoutRooms); if (rc) return rc;
    LayoutSource fresh;
    fresh.dev.kind = kLayoutRooms;
    fresh.dev.gen = RcwWallGen{0u, levels, first_level, level_seed, 0, 0};
    fresh.dev.rooms = RcwWallRooms{room, stop, doors};
    return install_layout_source(h, fresh);
}

int rcw_wall_rooms_info(rcw_handle* h, int32_t* enabled, int32_t* room, uint32_t* stop, uint32_t* doors)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const RcwWallRooms& r = h->source.dev.rooms;                       // (zeros while the rooms are off)
    if (enabled) *enabled = h->source.is(kLayoutRooms) ? 1 : 0;
    if (room) *room = r.room;
    if (stop) *stop = r.stop;
    if (doors) *doors = r.doors;
    return RCW_OK;
}

// Episode statistics (include/rcw.h).  Enabling allocates, zeroes the table and the agents' counts and begins every agent's record at once,
// stream-ordered behind what is queued; enabling again does the same again; an allocation failure leaves what was there.
int rcw_set_episode_stats(rcw_handle* h, int32_t enable)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::EpisodeStats& es = h->stats;
    if (!enable && !es.on()) return RCW_OK;
    rcw_handle::EpisodeStats fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (enable) {
        RcwEpisodeStats& d = fresh.dev;
        plan_episode_stats_rows(h->source.dev.kind, h->source.dev.agents.layouts, h->source.dev.gen.levels, h->source.dev.gen.first_level, &d.rows, &d.first);
        SnapshotShape sh = snapshot_shape(h);
        sh.stats = 1;
        AgentArrays list;                                          // head: the table
        agent_arrays(sh, kFeatStats, &list);
        size_t bytes = 0;
        const hipError_t e = list.head == fresh.table_bytes() ? alloc_parts(h, fresh.buf, list, 0, list.n, list.head, at, &bytes) : hipErrorInvalidValue;
        if (e != hipSuccess) return fail(hip_code(e), "episode statistics of %zu bytes: %s", bytes, hip_failure(e));
        d.table = fresh.buf.get<uint64_t>();
        d.prev_x = at[kSnapStatsPrevX].ptr;
        d.prev_y = at[kSnapStatsPrevY].ptr;
        d.words = RcwEpisodeWords{at[kSnapStatsFinished].as<uint8_t>(), at[kSnapStatsOutcome].as<uint8_t>(), at[kSnapStatsLength].as<uint32_t>(), at[kSnapStatsMoves].as<uint32_t>(),
                                  at[kSnapStatsLevel].as<int32_t>(), at[kSnapStatsSpl].as<int32_t>(), at[kSnapStatsEpisodes].as<uint32_t>()};
        d.last_episode = at[kSnapStatsLast].as<uint32_t>();
    }
    RCW_HIP(take_live(h, kFeatStats, at));
    es = std::move(fresh);
    if (es.on()) {
        RCW_HIP(hipMemsetAsync(es.dev.table, 0, es.table_bytes(), h->stream));
        RCW_HIP(hipMemsetAsync(es.dev.words.episodes, 0, (size_t)h->B * sizeof(uint32_t), h->stream));
        RCW_HIP(launch_episode_stats(h, nullptr, kStackRefill));
    }
    return RCW_OK;
}

int rcw_episode_stats_info(rcw_handle* h, int32_t* enabled, int32_t* rows, int32_t* first)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (enabled) *enabled = h->stats.on() ? 1 : 0;
    if (rows) *rows = h->stats.dev.rows;                                // (zeros while off)
    if (first) *first = h->stats.dev.first;
    return RCW_OK;
}

int rcw_episode_stats(rcw_handle* h, uint8_t* finished, uint8_t* outcome, uint32_t* length, uint32_t* moves, int32_t* level, int32_t* spl_q16, uint32_t* episodes)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoEpisodeStats, {{finished, kSnapStatsFinished}, {outcome, kSnapStatsOutcome}, {length, kSnapStatsLength}, {moves, kSnapStatsMoves},
                                            {level, kSnapStatsLevel}, {spl_q16, kSnapStatsSpl}, {episodes, kSnapStatsEpisodes}});
}

int rcw_episode_stats_device_ptr(rcw_handle* h, void** finished, void** outcome, void** length, void** moves, void** level, void** spl_q16, void** episodes)
{
    return hand_out(h, kNoEpisodeStats, {{finished, kSnapStatsFinished}, {outcome, kSnapStatsOutcome}, {length, kSnapStatsLength}, {moves, kSnapStatsMoves},
                                         {level, kSnapStatsLevel}, {spl_q16, kSnapStatsSpl}, {episodes, kSnapStatsEpisodes}});
}

int rcw_episode_stats_table(rcw_handle* h, uint64_t* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need(h->stats.on(), kNoEpisodeStats); if (rc) return rc;
    if (!out_host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL output pointer");
    rc = sync_and_check(h);
    RCW_HIP(hipMemcpy(out_host, h->stats.dev.table, h->stats.table_bytes(), hipMemcpyDeviceToHost));
    return rc;
}

int rcw_episode_stats_table_device_ptr(rcw_handle* h, void** ptr)
{
    if (!h || !ptr) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = need(h->stats.on(), kNoEpisodeStats); if (rc) return rc;
    *ptr = h->stats.dev.table;
    return RCW_OK;
}

// (stream-ordered and without waiting for the stream: a step queued before it adds to the old table, one queued behind it to the zeroed one)
int rcw_episode_stats_clear(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need(h->stats.on(), kNoEpisodeStats); if (rc) return rc;
    RCW_HIP(hipMemsetAsync(h->stats.dev.table, 0, h->stats.table_bytes(), h->stream));
    return RCW_OK;
}

// The visit map (include/rcw.h).  Enabling allocates, zeroes the table and begins every agent at once (its map cleared, its cell counted),
// stream-ordered behind what is queued; enabling again does the same again, with new parameters if they differ; an allocation failure
// leaves what was there.
int rcw_set_visit_map(rcw_handle* h, int32_t enable, int32_t sectors, int32_t flags)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::VisitMap& vm = h->visits;
    if (!enable && !vm.on()) return RCW_OK;
    rcw_handle::VisitMap fresh;
    LiveArray at[kSnapFieldCount] = {};
    if (enable) {
        if (sectors < 1 || sectors > RCW_VISIT_MAX_SECTORS || sectors > h->dev.nd)
            return fail(RCW_ERR_INVALID_ARGUMENT, "sectors must be in 1..min(%d, num_directions = %d) (got %d)", RCW_VISIT_MAX_SECTORS, h->dev.nd, sectors);
        if (flags & ~RCW_VISIT_TABLE) return fail(RCW_ERR_INVALID_ARGUMENT, "flags: the only bit is RCW_VISIT_TABLE (got %d)", flags);
        if ((int64_t)sectors * h->dev.H * h->dev.W > INT32_MAX / 2) return fail(RCW_ERR_UNSUPPORTED, "a visit map of %d sectors on a map of %d x %d is too large", sectors, h->dev.H, h->dev.W);
        RcwVisitMap& d = fresh.dev;
        SnapshotShape sh = snapshot_shape(h);
        sh.visit_sectors = sectors; sh.visit_flags = flags;
        if (flags & RCW_VISIT_TABLE) plan_visit_table_rows(sh, &d.rows, &d.first_level);
        AgentArrays list;                                          // head: the table
        agent_arrays(sh, kFeatVisits, &list);
        size_t bytes = 0;
        const hipError_t e = alloc_parts(h, fresh.buf, list, 0, list.n, list.head, at, &bytes);
        if (e != hipSuccess) return fail(hip_code(e), "visit map of %zu bytes: %s", bytes, hip_failure(e));
        d.sectors = sectors; d.cells = sectors * h->dev.H * h->dev.W;
        d.table = (flags & RCW_VISIT_TABLE) ? fresh.buf.get<uint32_t>() : nullptr;
        d.here = at[kSnapVisitHere].as<int32_t>(); d.visited = at[kSnapVisitVisited].as<int32_t>(); d.first = at[kSnapVisitFirst].as<int32_t>();
        d.level_here = at[kSnapVisitLevelHere].as<uint32_t>(); d.last_episode = at[kSnapVisitLast].as<uint32_t>();
        d.map = at[kSnapVisitMap].as<uint16_t>();
        fresh.flags = flags;
    }
    RCW_HIP(take_live(h, kFeatVisits, at));
    vm = std::move(fresh);
    if (vm.on()) {
        if (vm.table()) RCW_HIP(hipMemsetAsync(vm.dev.table, 0, vm.table_bytes(), h->stream));
        RCW_HIP(hipMemsetAsync(vm.dev.level_here, 0, (size_t)h->B * sizeof(uint32_t), h->stream));   // (stays 0 on a handle without the table)
        RCW_HIP(launch_visit_map(h, nullptr, kStackRefill));
    }
    return RCW_OK;
}

int rcw_visit_map_info(rcw_handle* h, int32_t* enabled, int32_t* sectors, int32_t* flags, int32_t* rows, int32_t* first_level)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    const rcw_handle::VisitMap& vm = h->visits;                        // (zeros while off)
    if (enabled) *enabled = vm.on() ? 1 : 0;
    if (sectors) *sectors = vm.dev.sectors;
    if (flags) *flags = vm.flags;
    if (rows) *rows = vm.dev.rows;
    if (first_level) *first_level = vm.dev.first_level;
    return RCW_OK;
}

int rcw_visit_words(rcw_handle* h, int32_t* here, int32_t* visited, int32_t* first, uint32_t* level_here)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoVisitMap, {{here, kSnapVisitHere}, {visited, kSnapVisitVisited}, {first, kSnapVisitFirst}, {level_here, kSnapVisitLevelHere}});
}

int rcw_visit_words_device_ptr(rcw_handle* h, void** here, void** visited, void** first, void** level_here)
{
    return hand_out(h, kNoVisitMap, {{here, kSnapVisitHere}, {visited, kSnapVisitVisited}, {first, kSnapVisitFirst}, {level_here, kSnapVisitLevelHere}});
}

int rcw_visit_map(rcw_handle* h, int32_t first, int32_t count, void* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoVisitMap, {{out_host, kSnapVisitMap}}, true, first, count);
}

int rcw_visit_map_device_ptr(rcw_handle* h, void** ptr) { return hand_out(h, kNoVisitMap, {{ptr, kSnapVisitMap}}); }

int rcw_visit_table(rcw_handle* h, uint32_t* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need(h->visits.on(), kNoVisitMap); if (rc) return rc;
    rc = need(h->visits.table(), kNoVisitTable); if (rc) return rc;
    if (!out_host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL output pointer");
    rc = sync_and_check(h);
    RCW_HIP(hipMemcpy(out_host, h->visits.dev.table, h->visits.table_bytes(), hipMemcpyDeviceToHost));
    return rc;
}

int rcw_visit_table_device_ptr(rcw_handle* h, void** ptr)
{
    if (!h || !ptr) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = need(h->visits.on(), kNoVisitMap); if (rc) return rc;
    rc = need(h->visits.table(), kNoVisitTable); if (rc) return rc;
    *ptr = h->visits.dev.table;
    return RCW_OK;
}

// (stream-ordered and without waiting for the stream, as rcw_episode_stats_clear; no per-agent word is touched)
int rcw_visit_table_clear(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need(h->visits.on(), kNoVisitMap); if (rc) return rc;
    rc = need(h->visits.table(), kNoVisitTable); if (rc) return rc;
    RCW_HIP(hipMemsetAsync(h->visits.dev.table, 0, h->visits.table_bytes(), h->stream));
    return RCW_OK;
}

// The start rule (include/rcw.h).  Enabling allocates, records the counters as they are and clears `placed`: no agent moves, the rule holds
// from the next start of an episode.  On a handle that has it only the band changes — a kernel argument of the launches that follow: no
// allocation, no wait.  A refused band changes nothing.
int rcw_set_start_distance(rcw_handle* h, int32_t enable, int32_t lo, int32_t hi)
{
    int rc = check_handle(h); if (rc) return rc;
    rcw_handle::StartRule& sr = h->start;
    if (!enable && !sr.on()) return RCW_OK;
    if (enable) {
        if (check_start_band(lo, hi) != RCW_OK)
            return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_set_start_distance: the band must be 1 <= lo <= hi <= %d (got %d, %d)", RCW_START_DISTANCE_MAX, lo, hi);
        if (sr.on()) { sr.lo = lo; sr.hi = hi; return RCW_OK; }
    }
    rcw_handle::StartRule fresh;
    LiveArray at[kSnapFieldCount] = {};
    size_t bytes = 0;
    if (enable) {
        SnapshotShape sh = snapshot_shape(h);
        sh.start = 1;
        AgentArrays list;
        agent_arrays(sh, kFeatStart, &list);
        const hipError_t e = alloc_parts(h, fresh.buf, list, 0, list.n, 0, at, &bytes);
        if (e != hipSuccess) return fail(hip_code(e), "start rule of %zu bytes: %s", bytes, hip_failure(e));
        fresh.dev.last_episode = at[kSnapStartLast].as<uint32_t>();
        fresh.dev.placed = at[kSnapStartPlaced].as<uint8_t>();
        fresh.dev.mask = at[kSnapStartMask].as<uint8_t>();
        fresh.lo = lo; fresh.hi = hi;
    }
    RCW_HIP(take_live(h, kFeatStart, at));
    sr = std::move(fresh);
    if (sr.on()) {
        RCW_HIP(hipMemsetAsync(sr.buf.get(), 0, bytes, h->stream));
        RCW_HIP(hipMemcpyAsync(sr.dev.last_episode, h->d_episode.get(), (size_t)h->B * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    }
    return RCW_OK;
}

int rcw_start_distance_info(rcw_handle* h, int32_t* enabled, int32_t* lo, int32_t* hi)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if (enabled) *enabled = h->start.on() ? 1 : 0;                      // (zeros while off)
    if (lo) *lo = h->start.lo;
    if (hi) *hi = h->start.hi;
    return RCW_OK;
}

int rcw_start_distance(rcw_handle* h, uint8_t* placed)
{
    int rc = check_handle(h); if (rc) return rc;
    return copy_arrays(h, kNoStartRule, {{placed, kSnapStartPlaced}});
}

int rcw_start_distance_device_ptr(rcw_handle* h, void** placed) { return hand_out(h, kNoStartRule, {{placed, kSnapStartPlaced}}); }

// ---- the state archive (include/rcw.h, rcw_handle::Snapshots) -----------------------------------------------------------------------------
extern "C++" {
namespace {

using Snapshots = rcw_handle::Snapshots;

int need_snapshots(rcw_handle* h) { return need(h->snaps.on(), "the handle has no state archive (rcw_set_snapshots)"); }

// A save or a restore of a handle whose shape is no longer the archive's is refused, and names the first segment that differs.
int check_snapshot_shape(rcw_handle* h, const char* caller)
{
    SnapshotPlan now;
    plan_snapshot(snapshot_shape(h), &now);
    const char* const seg = snapshot_plan_differs(h->snaps.plan, now);
    return seg ? fail(RCW_ERR_UNSUPPORTED, "%s: the handle's shape differs from the archive's in segment %s; bind the archive again (rcw_set_snapshots)", caller, seg) : RCW_OK;
}

// The device half of both variants: the checks that need no index, then the launches.
int snapshot_device(rcw_handle* h, const char* caller, const int32_t* rows_dev, const uint8_t* mask_dev, bool restore)
{
    int rc = need_snapshots(h); if (rc) return rc;
    rc = check_snapshot_shape(h, caller); if (rc) return rc;
    if (!rows_dev && h->snaps.rows < h->B)
        return fail(RCW_ERR_INVALID_ARGUMENT, "%s: without row indices agent a takes row a, which needs rows >= %d (the archive has %d)", caller, h->B, h->snaps.rows);
    RCW_HIP(launch_snapshot(h, rows_dev, mask_dev, restore));
    return RCW_OK;
}

// The host variants: the indices of the masked agents are checked here — in range, filled (restore), distinct (save) —, a violation names
// the agent and changes nothing; then mask and indices are staged and the device half runs.
int snapshot_host(rcw_handle* h, const char* caller, const int32_t* rows_host, const uint8_t* mask_host, bool restore)
{
    int rc = need_snapshots(h); if (rc) return rc;
    rc = check_snapshot_shape(h, caller); if (rc) return rc;
    Snapshots& sn = h->snaps;
    const int32_t B = h->B, rows = sn.rows;
    if (!rows_host && rows < B)
        return fail(RCW_ERR_INVALID_ARGUMENT, "%s: without row indices agent a takes row a, which needs rows >= %d (the archive has %d)", caller, B, rows);
    std::vector<uint8_t> filled;
    std::vector<int32_t> taken;
    try {
        if (restore) filled.resize((size_t)rows); else taken.assign((size_t)rows, -1);
    } catch (const std::bad_alloc&) {
        return fail(RCW_ERR_OUT_OF_MEMORY, "host allocation of the archive's row flags failed");
    }
    if (restore) {                                                     // (device saves queued before this call count: wait for them)
        RCW_HIP(hipStreamSynchronize(h->stream));
        RCW_HIP(hipMemcpy(filled.data(), sn.filled, (size_t)rows, hipMemcpyDeviceToHost));
    }
    for (int32_t a = 0; a < B; ++a) {
        if (mask_host && !mask_host[a]) continue;
        const int32_t r = rows_host ? rows_host[a] : a;
        if (r < 0 || r >= rows) return fail(RCW_ERR_INVALID_ARGUMENT, "%s: agent %d: row %d not in 0..%d", caller, a, r, rows - 1);
        if (restore && !filled[(size_t)r]) return fail(RCW_ERR_INVALID_ARGUMENT, "%s: agent %d: row %d has not been filled", caller, a, r);
        if (!restore) {
            if (taken[(size_t)r] >= 0) return fail(RCW_ERR_INVALID_ARGUMENT, "%s: agent %d: row %d is also agent %d's (a host save takes distinct rows)", caller, a, r, taken[(size_t)r]);
            taken[(size_t)r] = a;
        }
    }
    const uint8_t* mask_dev = nullptr;
    rc = upload_mask(h, mask_host, &mask_dev); if (rc) return rc;
    if (rows_host) {
        RCW_HIP(hipMemcpyAsync(sn.in_rows, rows_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        RCW_HIP(hipStreamSynchronize(h->stream));                      // (pageable host memory of the caller's)
    }
    RCW_HIP(launch_snapshot(h, rows_host ? sn.in_rows : nullptr, mask_dev, restore));
    return RCW_OK;
}

int check_snapshot_rows(rcw_handle* h, const char* caller, int32_t first, int32_t count, const void* host)
{
    if (host && first >= 0 && count >= 0 && first + (int64_t)count <= h->snaps.rows) return RCW_OK;
    return fail(RCW_ERR_INVALID_ARGUMENT, "%s: bad row range [%d, %lld) of %d rows, or a NULL buffer", caller, first, (long long)first + count, h->snaps.rows);
}

}  // namespace
}  // extern "C++"

// Bind the archive to the handle's shape as of now: `rows` empty records.  Everything is allocated before anything is given up.
int rcw_set_snapshots(rcw_handle* h, int32_t rows)
{
    int rc = check_handle(h); if (rc) return rc;
    if (rows < 0 || rows > RCW_SNAPSHOT_MAX_ROWS) return fail(RCW_ERR_INVALID_ARGUMENT, "rows must be in 0..%d (got %d)", RCW_SNAPSHOT_MAX_ROWS, rows);
    Snapshots& sn = h->snaps;
    if (rows == 0 && !sn.on()) return RCW_OK;
    Snapshots fresh;
    if (rows > 0) {
        plan_snapshot(snapshot_shape(h), &fresh.plan);
        const size_t R = (size_t)rows, B = (size_t)h->B;
        const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        size_t off[kSnapshotMaxSegments], bytes = 0;
        for (int k = 0; k < fresh.plan.n; ++k) { off[k] = bytes; bytes = up16(bytes + R * fresh.plan.seg[k].bytes); }
        const size_t ints = bytes;
        bytes += (R + 2 * B) * sizeof(int32_t);
        const size_t flags = bytes;
        bytes += R;
        const hipError_t e = fresh.buf.hipMalloc(bytes);
        if (e != hipSuccess) return fail(hip_code(e), "state archive of %d rows of %llu bytes: %s", rows, (unsigned long long)fresh.plan.row_bytes, hip_failure(e));
        uint8_t* const base = fresh.buf.get<uint8_t>();
        for (int k = 0; k < fresh.plan.n; ++k) fresh.arc[k] = base + off[k];
        fresh.owner = reinterpret_cast<int32_t*>(base + ints);
        fresh.sel = fresh.owner + R;
        fresh.in_rows = fresh.sel + B;
        fresh.filled = base + flags;
        fresh.rows = rows;
        RCW_HIP(hipMemsetAsync(base, 0, bytes, h->stream));            // (no row is filled; an unfilled row reads as zeros)
    }
    RCW_HIP(replace_buffers(h, {}));                                   // (every stream waited for: queued work may still use the old rows)
    sn = std::move(fresh);
    return RCW_OK;
}

// (without an archive: no rows, and the record the handle's shape would have now)
int rcw_snapshot_info(rcw_handle* h, int32_t* rows, uint64_t* row_bytes, uint64_t* shape_key)
{
    if (!h) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    SnapshotPlan now;
    if (!h->snaps.on()) plan_snapshot(snapshot_shape(h), &now);
    const SnapshotPlan& p = h->snaps.on() ? h->snaps.plan : now;
    if (rows) *rows = h->snaps.rows;
    if (row_bytes) *row_bytes = p.row_bytes;
    if (shape_key) *shape_key = p.key;
    return RCW_OK;
}

int rcw_snapshot_save(rcw_handle* h, const int32_t* rows_host, const uint8_t* mask_host)
{
    int rc = check_handle(h); if (rc) return rc;
    return snapshot_host(h, "rcw_snapshot_save", rows_host, mask_host, false);
}
int rcw_snapshot_restore(rcw_handle* h, const int32_t* rows_host, const uint8_t* mask_host)
{
    int rc = check_handle(h); if (rc) return rc;
    return snapshot_host(h, "rcw_snapshot_restore", rows_host, mask_host, true);
}
int rcw_snapshot_save_device(rcw_handle* h, const int32_t* rows_device, const uint8_t* mask_device)
{
    int rc = check_handle(h); if (rc) return rc;
    return snapshot_device(h, "rcw_snapshot_save_device", rows_device, mask_device, false);
}
int rcw_snapshot_restore_device(rcw_handle* h, const int32_t* rows_device, const uint8_t* mask_device)
{
    int rc = check_handle(h); if (rc) return rc;
    return snapshot_device(h, "rcw_snapshot_restore_device", rows_device, mask_device, true);
}

int rcw_snapshot_filled(rcw_handle* h, uint8_t* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need_snapshots(h); if (rc) return rc;
    if (!out_host) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL output pointer");
    RCW_HIP(hipStreamSynchronize(h->stream));
    RCW_HIP(hipMemcpy(out_host, h->snaps.filled, (size_t)h->snaps.rows, hipMemcpyDeviceToHost));
    return RCW_OK;
}

// Rows [first, first + count) as the caller keeps them: row_bytes each, the segments in the table's order, unpadded.
int rcw_snapshot_rows_copy(rcw_handle* h, int32_t first, int32_t count, void* out_host)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need_snapshots(h); if (rc) return rc;
    rc = check_snapshot_rows(h, "rcw_snapshot_rows_copy", first, count, out_host); if (rc) return rc;
    const Snapshots& sn = h->snaps;
    rc = sync_and_check(h); if (rc) return rc;                          // (a sticky device error: nothing is copied, rcw_clear_error first)
    for (int k = 0; k < sn.plan.n && count > 0; ++k) {
        const size_t b = sn.plan.seg[k].bytes;
        RCW_HIP(hipMemcpy2D(static_cast<uint8_t*>(out_host) + sn.plan.offset(k), (size_t)sn.plan.row_bytes, sn.arc[k] + (size_t)first * b, b, b, (size_t)count, hipMemcpyDeviceToHost));
    }
    return rc;
}

// ... and back, into a handle of the same shape (the key): every row is checked on the host first (validate_snapshot_row), and nothing is
// loaded unless all pass.  The rows loaded count as filled.
int rcw_snapshot_rows_load(rcw_handle* h, int32_t first, int32_t count, const void* in_host, uint64_t shape_key)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need_snapshots(h); if (rc) return rc;
    rc = check_snapshot_shape(h, "rcw_snapshot_rows_load"); if (rc) return rc;   // (the row check below reads the rows by the handle's shape NOW)
    rc = check_snapshot_rows(h, "rcw_snapshot_rows_load", first, count, in_host); if (rc) return rc;
    const Snapshots& sn = h->snaps;
    if (shape_key != sn.plan.key)
        return fail(RCW_ERR_UNSUPPORTED, "rcw_snapshot_rows_load: the rows' shape key %016llx is not the archive's (%016llx)", (unsigned long long)shape_key, (unsigned long long)sn.plan.key);
    const SnapshotShape shape = snapshot_shape(h);
    const uint8_t* const in = static_cast<const uint8_t*>(in_host);
    char why[256];
    for (int32_t r = 0; r < count; ++r)
        if (validate_snapshot_row(shape, sn.plan, in + (size_t)r * sn.plan.row_bytes, why, sizeof why) != RCW_OK)
            return fail(RCW_ERR_INVALID_ARGUMENT, "rcw_snapshot_rows_load: row %d: %s", first + r, why);
    if (count == 0) return RCW_OK;
    RCW_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < sn.plan.n; ++k) {
        const size_t b = sn.plan.seg[k].bytes;
        RCW_HIP(hipMemcpy2D(sn.arc[k] + (size_t)first * b, b, in + sn.plan.offset(k), (size_t)sn.plan.row_bytes, b, (size_t)count, hipMemcpyHostToDevice));
    }
    RCW_HIP(hipMemsetAsync(sn.filled + first, 1, (size_t)count, h->stream));   // (the handle's stream, as all of the archive's device work)
    RCW_HIP(hipStreamSynchronize(h->stream));
    return RCW_OK;
}

int rcw_expand_columns_view(rcw_handle* h, const int32_t* height_line_pu_device, const uint8_t* colour_id_device,
                            int32_t count, void* view_device)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need(h->learner.on(), kNoLearnerView); if (rc) return rc;
    if (!height_line_pu_device || !colour_id_device || !view_device || count < 1)
        return fail(RCW_ERR_INVALID_ARGUMENT, "bad argument");
    RCW_HIP(rcw_launch_view(h->dev, h->learner.view, height_line_pu_device, colour_id_device, count, nullptr, (uint8_t*)view_device, h->stream));
    return RCW_OK;
}

int rcw_device_malloc(rcw_handle* h, uint64_t bytes, void** device_ptr)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!device_ptr || bytes == 0) return fail(RCW_ERR_INVALID_ARGUMENT, "bad argument");
    *device_ptr = nullptr;
    RCW_HIP(hipMalloc(device_ptr, (size_t)bytes));
    return RCW_OK;
}
int rcw_device_free(rcw_handle* h, void* device_ptr)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!device_ptr) return RCW_OK;
    RCW_HIP(hipStreamSynchronize(h->stream));   // work enqueued on the handle may still use it
    RCW_HIP(hipFree(device_ptr));
    return RCW_OK;
}
int rcw_memcpy_to_host(rcw_handle* h, void* dst_host, const void* src_device, uint64_t bytes)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!dst_host || !src_device) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    rc = sync_and_check(h);
    RCW_HIP(hipMemcpy(dst_host, src_device, (size_t)bytes, hipMemcpyDeviceToHost));
    return rc;
}

int rcw_ray_table(rcw_handle* h, float* out) { return table_out(h, out, &rcw_handle::ray_table, "rcw_ray_table"); }
int rcw_direction_table(rcw_handle* h, float* out) { return table_out(h, out, &rcw_handle::dir_table, "rcw_direction_table"); }
int rcw_ray_table64(rcw_handle* h, double* out) { return table_out(h, out, &rcw_handle::ray_table64, "rcw_ray_table64"); }
int rcw_direction_table64(rcw_handle* h, double* out) { return table_out(h, out, &rcw_handle::dir_table64, "rcw_direction_table64"); }

int rcw_timer_start(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    RCW_HIP(hipEventRecord(h->ev_start.get(), h->stream));
    return RCW_OK;
}
int rcw_timer_stop(rcw_handle* h, float* elapsed_ms)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!elapsed_ms) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    RCW_HIP(hipEventRecord(h->ev_stop.get(), h->stream));
    RCW_HIP(hipEventSynchronize(h->ev_stop.get()));
    RCW_HIP(hipEventElapsedTime(elapsed_ms, h->ev_start.get(), h->ev_stop.get()));
    return RCW_OK;
}

int rcw_profile(rcw_handle* h, int32_t enable)
{
    int rc = check_handle(h); if (rc) return rc;
    RCW_HIP(hipStreamSynchronize(h->stream));
    rcw_handle::Profile& p = h->prof;
    if (enable && p.ev.empty()) {
        p.ev.resize(4 * p.kSlots);
        for (RcwEvent& ev : p.ev) RCW_HIP(ev.hipEventCreate());
    }
    p.on = enable != 0;
    p.count = 0;
    return RCW_OK;
}

int rcw_profile_read(rcw_handle* h, float* cast_ms, float* top_view_ms, float* fill_ms, int32_t* steps)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!cast_ms || !top_view_ms || !fill_ms || !steps) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    RCW_HIP(hipStreamSynchronize(h->stream));
    double c = 0.0, t = 0.0, f = 0.0;
    const rcw_handle::Profile& p = h->prof;
    for (int k = 0; k < p.count; ++k) {
        float a = 0.0f, b = 0.0f, d = 0.0f;
        RCW_HIP(hipEventElapsedTime(&a, p.ev[4 * k].get(), p.ev[4 * k + 1].get()));
        RCW_HIP(hipEventElapsedTime(&b, p.ev[4 * k + 1].get(), p.ev[4 * k + 2].get()));
        RCW_HIP(hipEventElapsedTime(&d, p.ev[4 * k + 2].get(), p.ev[4 * k + 3].get()));
        c += a;
        if (h->dev.top_split) { f += b; t += d; } else { t += b; f += d; }      // two-kernel top view: cast | fill (+ draw beside it) | store
    }
    *steps = p.count;
    *cast_ms = p.count ? (float)(c / p.count) : 0.0f;
    *top_view_ms = p.count && h->dev.top_view ? (float)(t / p.count) : 0.0f;
    *fill_ms = p.count ? (float)(f / p.count) : 0.0f;
    return RCW_OK;
}

int rcw_top_view_form(rcw_handle* h, int32_t* form)
{
    if (!h || !form) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *form = top_form_in_step(h->dev);
    return RCW_OK;
}

int rcw_update_top_view_form(rcw_handle* h, int32_t* form)
{
    if (!h || !form) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *form = top_form_alone(h->dev);
    return RCW_OK;
}

int rcw_set_top_view_form(rcw_handle* h, int32_t form, int32_t runs)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!h->d_top_view.get()) return fail(RCW_ERR_UNSUPPORTED, "handle was created with render_top_view = 0");
    if (form != 0 && form != RCW_TOP_VIEW_IN_PLACE && form != RCW_TOP_VIEW_ONE_KERNEL && form != RCW_TOP_VIEW_TWO_KERNELS)
        return fail(RCW_ERR_INVALID_ARGUMENT, "form must be 0 (automatic) or RCW_TOP_VIEW_IN_PLACE / ONE_KERNEL / TWO_KERNELS (got %d)", form);
    if (runs < 0 || runs > 8) return fail(RCW_ERR_INVALID_ARGUMENT, "runs must be 0 (automatic) or 1..8 (got %d)", runs);
    rc = plan_top_view(h, form, runs, /*lenient=*/false);   // (waits for every stream first: the scratch of the current form may be in use)
    if (rc != RCW_OK) {                               // leave a usable handle behind: back to the automatic choice
        const int rc2 = plan_top_view(h, 0, 0, true);
        return rc2 != RCW_OK ? rc2 : rc;
    }
    return RCW_OK;
}

int rcw_step_form(rcw_handle* h, int32_t* form)
{
    if (!h || !form) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *form = h->step.on() ? RCW_STEP_ONE_LAUNCH : RCW_STEP_TWO_LAUNCHES;
    return RCW_OK;
}

int rcw_set_step_form(rcw_handle* h, int32_t form)
{
    int rc = check_handle(h); if (rc) return rc;
    if (form != 0 && form != RCW_STEP_TWO_LAUNCHES && form != RCW_STEP_ONE_LAUNCH)
        return fail(RCW_ERR_INVALID_ARGUMENT, "form must be 0 (automatic) or RCW_STEP_TWO_LAUNCHES / RCW_STEP_ONE_LAUNCH (got %d)", form);
    const bool was_on = h->step.on();
    rc = plan_step_form(h, form); if (rc) return rc;
    if (h->step.on() && !was_on) RCW_HIP(launch_step(h, nullptr, nullptr, kStackKeep));   // prime the slots (re-renders the current frames: the same pixels)
    return RCW_OK;
}

int rcw_fill_kernel_name(rcw_handle* h, char* buf, int32_t buflen)
{
    if (!h || !buf || buflen < 1) return fail(RCW_ERR_INVALID_ARGUMENT, "bad argument");
    std::snprintf(buf, (size_t)buflen, "%s", h->step.on() ? (h->dev.Hc == 256 ? "rcw_fill256_cast_kernel" : "rcw_fill_window_cast_kernel") : rcw_fill_kernel_name(h->dev, (long long)h->dev.B * h->dev.N));
    return RCW_OK;
}

int rcw_batch(rcw_handle* h, int32_t* out)
{
    if (!h || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = h->B; return RCW_OK;
}
int rcw_get_config(rcw_handle* h, rcw_config* out)
{
    if (!h || !out) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = h->cfg; return RCW_OK;
}
int rcw_device_name(rcw_handle* h, char* buf, int32_t buflen)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!buf || buflen < 1) return fail(RCW_ERR_INVALID_ARGUMENT, "bad buffer");
    hipDeviceProp_t prop;
    RCW_HIP(hipGetDeviceProperties(&prop, h->device));
    std::snprintf(buf, (size_t)buflen, "%s (%s)", prop.name, prop.gcnArchName);
    return RCW_OK;
}

}  // extern "C"
