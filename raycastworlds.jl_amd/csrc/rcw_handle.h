// The handle of librcw_hip, the facts of its step, and what the host units call on one another (Makefile: which unit holds what).
// Types and declarations only (and RCW_DEV_ENV, the development build's read of a tuning knob).
#pragma once
#include "../../include/rcw.h"
#include "rcw_error.h"
#include "rcw_kernels.h"
#include "rcw_owned.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

// THE FACTS OF A STEP: what decides which launches a step of a handle makes, and whether the one-launch step (rcw_fill256_cast_kernel) may
// leave the frame of an agent whose view it does not change as it is (`keep`).  No HIP call — the development build drives it without a
// device (rcw_dev_step_facts, tests/test_step_state.py) —, and private: only the events below, what happens to a handle, change a fact.
//   on, want, captured     a step is ONE launch; what rcw_set_step_form asked for (0 = the rule); a step of the handle was captured into a graph
//   cur, primed            of the one-launch step's two buffers of [B][5][N] packed column words (rcw_handle::Step), `cur` holds the frames of
//                          the CURRENT state (slot 0) and of its four successors (slots 1..4), written by the last casting launch — primed: for
//                          every agent (each buffer ends in one byte per agent: which of its slots hold the very frame slot 0 holds — cast_body)
//   obs_current            dev.obs holds, for EVERY agent, the frame of the state the primed slots were cast from: the one-launch step may then
//                          skip the unchanged frames.  False costs nothing but the skip: the next one-launch step writes every pixel and sets it.
//   cols_live, cols_stale  The (height_line_pu, colour id) descriptors of the current frames (d_col_h / d_col_c) are what the two-launch step
//                          hands from its cast kernel to its fill kernel; the one-launch step's fill reads the slots instead, and every store of
//                          the casting workgroups costs the launch more than its bytes (profiles/r06_step_forms.txt) — so it writes them only
//                          for a caller that holds their device pointers (cols_live), and otherwise leaves them stale: ensure_columns recasts
//                          the current state in front of whatever reads them (rcw_columns, the gathers, rcw_update_camera_view).
//   store_all              development build (RCW_STEP_STORE_ALL=1): every frame is stored, changed or not — the A/B of the unchanged-frame skip
class StepFacts {
    bool on_ = false, captured_ = false, primed_ = false, obs_current_ = false, cols_live_ = false, cols_stale_ = false, store_all_ = false;
    int want_ = 0, cur_ = 0;
    void forget() { primed_ = false; obs_current_ = false; }     // the slots describe nothing any more: so do their bytes
public:
    bool on() const { return on_; }
    bool cols_live() const { return cols_live_; }
    bool cols_stale() const { return cols_stale_; }
    int want() const { return want_; }
    int cur() const { return cur_; }
    void read(int32_t out[9]) const { const int32_t v[9] = {on_, want_, captured_, primed_, obs_current_, cur_, cols_live_, cols_stale_, store_all_}; std::memcpy(out, v, sizeof v); }
    void set_store_all(bool v) { store_all_ = v; }               // rcw_create

    // Which form a step takes (plan_step_form), in two halves with the slot buffers' allocation between them: plan() changes nothing, so a
    // refused or failed request leaves every fact as it was.  view_only: the cast kernel followed by the view kernel, no camera fill to fuse.
    struct Plan { const char* refused; int want; bool on, view_only; };
    Plan plan(int want, bool view_only, bool eligible, bool pays) const
    {
        const bool one = want == RCW_STEP_ONE_LAUNCH;
        if (view_only) return {one ? "the handle's learner view is set with RCW_VIEW_ONLY: a step is the cast kernel and the view kernel" : nullptr, want, false, true};
        if (one && !eligible) return {"this handle does not take the one-launch step (a camera view of 256 k, 128 or 64 rows — up to 8191 — without a top view, fewer than 2^29 view columns)", want, false, false};
        return {nullptr, want, want == RCW_STEP_TWO_LAUNCHES ? false : (one ? true : eligible && !captured_ && pays), false};
    }
    void take(const Plan& p)
    {
        if (p.on && p.want == RCW_STEP_ONE_LAUNCH) captured_ = false;
        if (p.view_only || p.on != on_) forget();                 // (a change of form, either way)
        on_ = p.on; want_ = p.want;
    }

    // A step, reset! or set_state's camera view begins: what it launches, and whether one launch may skip the unchanged frames.  Whatever
    // fails from here on leaves obs_current cleared.  capturing(), asked only where the one-launch form is on: that form keeps its place in
    // the slot buffers on the HOST, and a graph would replay one launch's pointers for ever.  A handle whose step is captured keeps the
    // two-launch form from then on (replays advance the state behind the library's back: its slots can never be trusted again).
    enum Path { kTwoLaunches, kOneLaunch, kPrime };
    struct Camera { Path path; bool was_current, keep; };
    template <typename Capturing>
    Camera camera_step(bool actions, bool masked, Capturing capturing)
    {
        const bool was_current = obs_current_ && primed_;
        obs_current_ = false;
        if (on_ && capturing()) { on_ = false; captured_ = true; forget(); }
        const Path path = !on_ ? kTwoLaunches : (actions && !masked && primed_ ? kOneLaunch : kPrime);
        return {path, was_current, path == kOneLaunch && was_current && !store_all_};
    }
    // ... and what it has launched (kTwoLaunches: nothing comes back).  One launch, skipped or not: every agent's frame is the new state's.
    void one_launch_queued() { cur_ ^= 1; obs_current_ = true; if (!cols_live_) cols_stale_ = true; }
    // (with a mask: the masked agents' descriptors are fresh — the fill behind it reads only those —, the others' as stale as before)
    void prime_cast_queued(bool masked) { if (!masked) { cols_stale_ = false; primed_ = true; } }
    // every agent painted and every slot primed — or, with a mask, exactly the agents repainted whose slots were rewritten: as it was
    void prime_fill_queued(const Camera& c, bool masked) { obs_current_ = primed_ && (!masked || c.was_current); }

    // rcw_bind_obs (also with the pointer it had: the caller may have written into the buffer), a RCW_VIEW_ONLY step (which does not paint
    // the camera view), rcw_update_camera_view before it paints — and behind its fill: every agent's current frame, which slot 0 holds
    void obs_unknown() { obs_current_ = false; }
    void camera_repainted() { if (on_ && primed_) obs_current_ = true; }
    // rcw_reset.  The seed is the HANDLE's: an agent that is done under auto_reset and NOT in the mask is re-sampled by its next action with
    // the new seed — but the one-launch step has already cast that agent's successors from a preview drawn with the old one: every agent's
    // slots are cast again by the next step, as a launch of its own.
    void reset(bool masked, bool new_seed, bool auto_reset) { if (masked && new_seed && auto_reset) forget(); }
    void columns_cast(bool masked = false) { if (!masked) cols_stale_ = false; }   // the cast kernel was queued: rcw_cast_rays, ensure_columns, a RCW_VIEW_ONLY step
    void columns_wanted() { cols_live_ = true; }                 // rcw_columns_device_ptr, a learner view switched on: every step refreshes the descriptors
    // rcw_set_time_limit: the slots were cast under the old limit (which agents the next action re-samples, whose successors are therefore a
    // preview's) — every agent's are cast again by the next step, as a launch of its own
    void time_limit_set() { forget(); }
    // rcw_snapshot_restore*, behind its gather and in front of its render: the restored agents' slots were cast from the state they had
    // before (and the others' successors may be previews of it) — every agent's are cast again by the next step, as a launch of its own —,
    // and no frame in dev.obs is known to be the one its slot 0 holds.  The descriptors stay as stale as they were: the masked render
    // behind it refreshes the restored agents' only, as rcw_reset's does.
    void restored() { forget(); obs_unknown(); }
};

// THE PER-AGENT ARRAYS OF A HANDLE, described ONCE (rcw_rules.hip, agent_arrays): per feature the list of its parts — an array each, [B] of
// `bytes` — and the bytes of its head, what lies in front of them and is not per agent (the statistics' table, the local map's offset
// table, the learner view's box tables).  Host values only, a function of SnapshotShape: the development build describes and carves without
// a device (rcw_dev_agent_arrays).  Everything else follows from the list:
//   the carve    carve_agent_arrays: the head, then the parts in list order, each on a multiple of 16 bytes.  A setter allocates the carve's
//                total and takes every pointer from its offsets; a feature of several buffers (the goal distance: field | words | counter,
//                the learner view: a buffer a part) carves each from its run of the list.
//   the table    rcw_handle::live, indexed by the part's id: where the array is and its bytes per agent, null while its feature is off.
//                The readouts (rcw_api.hip: copy_arrays, hand_out) and the archive's copy (launch_snapshot) look the arrays up there.
//   the record   of the state archive (include/rcw.h, "the state archive"): plan_snapshot takes the `archived` parts of every feature that is
//                on, in this order.  `tag` tells apart what the bytes alone do not (a learner view of 7 x 9 from one of 9 x 7, a bank's
//                layout index from a family's level).  key: FNV-1a over the table, the geometry, T, R and RCW_ABI_VERSION.
struct SnapshotShape {
    int32_t H = 0, W = 0, nd = 0, N = 0, Hc = 0;
    int32_t real64 = 0, reward_type = 0;
    int32_t goal = 0, seen = 0, stats = 0;                       // the goal distance, the seen map, episode statistics: on
    int32_t view_fmt = 0, view_layout = 0, view_C = 0, view_h = 0, view_w = 0, view_frames = 0;   // the learner view; view_fmt 0: off
    int32_t local_source = 0, local_size = 0, local_cells = 0;   // the local map; local_source 0: off
    int32_t source_kind = 0;                                     // RcwLayoutKind; 0: no layout source
    int32_t layouts = 0, levels = 0, first_level = 0;            // the source's range (validate_snapshot_row, the statistics' rows; not part of the record)
    int32_t guide = 0;                                           // the guide: on (its words are never archived: not part of the record)
    int32_t frontier = 0;                                        // the frontier: on (computed from the seen map, never archived: not part of the record)
    int32_t visit_sectors = 0, visit_flags = 0;                  // the visit map; visit_sectors 0: off.  visit_flags: RCW_VISIT_TABLE (the table is the head, not part of the record)
    int32_t start = 0;                                           // the start rule: on (the band is no part of the shape: it travels in the kernel's arguments)
};
constexpr int kSnapshotShapeWords = 23;                          // what travels through the 23-word development exports: everything but `guide`, `frontier`, the visit map's two and `start`
constexpr int kSnapshotVisitWords = 27;                          // ... and through rcw_dev_visit_plan: everything but `start`
// (a part's id, in the order of the features and, within one, of its list; kSnapViewStaging — the view kernels' frame under a k-frame stack —,
// kSnapSourceStatus, kSnapSourceMask, the guide's two words and everything of the frontier are never archived; everything of the visit
// map is; of the start rule the recorded counter and `placed` are, kSnapStartMask is not)
enum SnapshotField { kSnapPos, kSnapDir, kSnapGoal, kSnapReward, kSnapDone, kSnapEpisode, kSnapTileMap, kSnapEpisodeSteps, kSnapTruncated,
                     kSnapGoalField, kSnapGoalDistance, kSnapGoalStart, kSnapGoalProgress, kSnapGoalLast,
                     kSnapSeenCount, kSnapSeenNew, kSnapSeenGoal, kSnapSeenLast, kSnapSeenBits, kSnapSeenMap,
                     kSnapViewFrame, kSnapViewStack, kSnapViewLast, kSnapViewStaging, kSnapLocalImage,
                     kSnapSourceLast, kSnapSourceStatus, kSnapSourceLayout, kSnapSourceMask,
                     kSnapStatsFinished, kSnapStatsOutcome, kSnapStatsLength, kSnapStatsMoves, kSnapStatsLevel, kSnapStatsSpl, kSnapStatsEpisodes,
                     kSnapStatsPrevX, kSnapStatsPrevY, kSnapStatsLast, kSnapGuideAction, kSnapGuideHeading,
                     kSnapFrontierDistance, kSnapFrontierTiles, kSnapFrontierAction, kSnapFrontierHeading, kSnapFrontierLast, kSnapFrontierField,
                     kSnapVisitHere, kSnapVisitVisited, kSnapVisitFirst, kSnapVisitLevelHere, kSnapVisitLast, kSnapVisitMap,
                     kSnapStartLast, kSnapStartPlaced, kSnapStartMask, kSnapFieldCount };
enum AgentFeature { kFeatCore, kFeatGoal, kFeatSeen, kFeatView, kFeatLocal, kFeatSource, kFeatStats, kFeatGuide, kFeatFrontier, kFeatVisits, kFeatStart, kFeatCount };
constexpr SnapshotField kFeatureFirstId[kFeatCount + 1] = {kSnapPos, kSnapGoalField, kSnapSeenCount, kSnapViewFrame, kSnapLocalImage, kSnapSourceLast, kSnapStatsFinished, kSnapGuideAction, kSnapFrontierDistance, kSnapVisitHere, kSnapStartLast, kSnapFieldCount};
constexpr int kAgentMaxParts = 10;
struct AgentPart { SnapshotField id; const char* name; uint32_t bytes; uint64_t tag; bool archived; };
struct AgentArrays { int32_t n = 0; AgentPart part[kAgentMaxParts] = {}; uint64_t head = 0; };   // (n = 0: the feature is off)
struct AgentCarve { uint64_t off[kAgentMaxParts] = {}; uint64_t total = 0; };
struct LiveArray {
    void* ptr = nullptr;
    uint32_t bytes = 0;                // per agent
    template <typename T> T* as() const { return static_cast<T*>(ptr); }
};
constexpr int kSnapshotMaxSegments = kSnapFieldCount;
struct SnapshotSegment { SnapshotField field; const char* name; uint32_t bytes; uint64_t tag; };
struct SnapshotPlan {
    int32_t n = 0;
    SnapshotSegment seg[kSnapshotMaxSegments] = {};
    uint64_t row_bytes = 0, key = 0;
    int find(SnapshotField f) const { for (int k = 0; k < n; ++k) if (seg[k].field == f) return k; return -1; }
    uint64_t offset(int k) const { uint64_t o = 0; for (int j = 0; j < k; ++j) o += seg[j].bytes; return o; }   // of segment k in an exported row
};

// OWNERSHIP: every device buffer, pinned buffer, stream and event of a handle is a member of one of rcw_owned.h's types; nothing else frees
// them.  ~rcw_handle waits for all the handle's streams and then lets the members go in reverse order of declaration: the two STREAMS ARE
// DECLARED FIRST, so buffers and events go before the streams that used them.  A live handle gives a buffer up through replace_buffers().
struct rcw_handle {
    rcw_config cfg{};
    int32_t B = 0, device = 0, nchunks = 0;
    RcwHw hw{256, 160 * 1024, 32};     // the device's CUs, LDS bytes and wavefront slots a CU (hipDeviceProp_t: rcw_create)
    RcwPlan dev{};
    RcwStream own_stream, top_stream;  // (top_stream: the side stream of the two-kernel top view)
    hipStream_t stream = nullptr;      // the caller's (rcw_set_stream) or own_stream: not owned
    RcwEvent ev_start, ev_stop;
    // device allocations
    RcwBuf d_pos, d_dir, d_goal, d_reward, d_done, d_episode, d_episode_steps, d_truncated, d_tile_map, d_dir_table, d_ray_table, d_obs, d_col_h, d_col_c, d_err, d_status, d_top_view;
    // THE TABLE OF THE LIVE PER-AGENT ARRAYS, by id (above: "the per-agent arrays of a handle"): rcw_create writes the core state's entries, a
    // feature's setter its feature's — and clears them where it switches the feature off.  The features below keep the kernels' argument
    // structs and typed pointers, filled from the same carve; which parts a feature has and how they lie in its buffers is agent_arrays' word.
    LiveArray live[kSnapFieldCount];
    // two-kernel top view: planes / player pixels / tile codes in HBM, the side stream the draw kernel runs on
    RcwBuf d_top_plane, d_top_hdr, d_top_codes;
    // Several draw workgroups an agent (top_parts > 1) OR their bits into the agent's plane in HBM, and only rcw_top_store_kernel — which reads
    // every plane word exactly once — leaves the zero the next drawing needs: a drawing whose store did not follow (a failed launch in
    // between) leaves bits behind that every later frame would carry.  Set in front of such a
    // drawing, cleared behind its store's launch; a drawing that finds it set clears the planes first.
    bool top_plane_dirty = false;
    RcwEvent ev_top_fork, ev_top_join[8];   // (a join event per run of agents)
    RcwBuf d_actions, d_mask, d_in_goal, d_in_pos, d_in_dir;
    RcwBuf d_in_walls, d_in_wall_index;   // rcw_set_walls' staging: the layouts (in_walls_cap bytes, grow-only) and the agents' layout index (int32 [B])
    size_t in_walls_cap = 0;
    RcwPinned h_err, h_actions[2];     // the error word (int32_t); the staging ring of rcw_step (uint8_t)
    RcwEvent ev_actions[2];
    int action_slot = 0;
    struct Step : StepFacts { RcwBuf slot[2]; } step;   // (the one-launch step's two slot buffers: slot[cur()] is the one the next launch reads)
    // rcw_profile: HIP events around each kernel of a step (what bench.py's roofline block reads the fill kernel's duration from), four a
    // recorded step — start | after cast | after top view | after fill —, for the first kSlots steps since it was switched on
    struct Profile {
        static constexpr int kSlots = 256;
        bool on = false;
        int count = 0;
        std::vector<RcwEvent> ev;
    } prof;
    RcwBuf d_rays[4];                  // rcw_rays scratch (grow-only)
    size_t rays_cap[4] = {0, 0, 0, 0};
    // RCCL (loaded on demand): the observation gather
    void* comm = nullptr;              // ncclComm_t
    int32_t comm_rank = 0, comm_world = 0;
    RcwBuf d_gather_h, d_gather_c;     // gathered descriptors (B * world columns)
    bool real64 = false;            // world-unit type T = Float64 (cfg.world_unit_bits = 64)
    size_t real_size = sizeof(float);
    std::vector<float> dir_table;   // (2, nd)        T = Float32
    std::vector<float> ray_table;   // (N, 5, nd)
    std::vector<double> dir_table64;   //              T = Float64
    std::vector<double> ray_table64;
    // The learner view (rcw_set_learner_view*): what the caller set, the view kernels' arguments, the buffers.  frames = k > 1: `frame` is the
    // staging batch the view kernels write, `stack` the B * k frames the caller sees, `last_episode` each agent's episode counter as of its
    // last push (uint32 [B]); k = 1: `frame` is the view, the two are empty.  A buffer a part of the list; tab: the list's head, the box
    // tables (rows [h + 1], then columns [w + 1], then — depth formats — RcwView::dsum [Hc + 1]).
    struct LearnerView {
        struct Settings { int32_t fmt = RCW_VIEW_OFF, layout = RCW_VIEW_CHW, h = 0, w = 0, flags = 0, frames = 0; } set;
        RcwBuf frame, tab, stack, last_episode;
        RcwView view{};
        bool on() const { return set.fmt != RCW_VIEW_OFF; }
        bool only() const { return on() && (set.flags & RCW_VIEW_ONLY) != 0; }       // the step paints no camera view
    } learner;
    // The goal distance (rcw_set_goal_distance), THREE buffers: the UInt16 (H*W, B) field, the three Int32 (B) words — `words` points into
    // their carve — and each agent's episode counter as of the flood its field holds (uint32 [B]).  Empty while the feature is off.
    struct GoalDistance {
        RcwBuf field, word_buf, last_episode;
        RcwGoalWords words{};
        bool on() const { return field.get() != nullptr; }
    } goal;
    // The seen map (rcw_set_seen_map): ONE buffer, the carve of its list — the three Int32 (B) words, each agent's episode counter as of its
    // last clear, the packed seen bits (internal), the UInt8 (H*W, B) map; the pointers point into it.  Empty while the feature is off.
    struct SeenMap {
        RcwBuf buf;
        RcwSeenWords words{};
        uint32_t* last_episode = nullptr;
        uint32_t* bits = nullptr;
        uint8_t* map = nullptr;
        bool on() const { return buf.get() != nullptr; }
    } seen;
    // The local map (rcw_set_local_map): ONE buffer — the head is the offset table (S entries of the world-unit type), the one part the
    // UInt8 (S, S, B) images; the pointers point into it.  source = 0 and empty while the feature is off.  With RCW_LOCAL_SEEN the launch
    // reads seen.map as it is THEN: rcw_set_seen_map may have replaced it.
    struct LocalMap {
        RcwBuf buf;
        int32_t source = 0, size = 0, cells_per_tile = 0;
        const void* off = nullptr;
        uint8_t* img = nullptr;
        bool on() const { return buf.get() != nullptr; }
    } local;
    // The layout source (rcw_kernels.h: the wall bank, or the wall generator's mazes, caves or rooms).  INVARIANT: at most one source is live —
    // `dev.kind`, the only record of which —, and everything not of the live kind is empty or zero.  Every kind has `agents`, ONE buffer, the
    // carve of its list — recorded counter, recorded status, layout index, the mask — into which `dev.agents` points.  The bank alone has the packed layouts, the cumulative weights, and the pinned buffer and event through which the
    // weights reach `cum` (rcw_set_wall_bank_weights does not wait for the stream); of the bank the host keeps only its sizes: dev.agents.layouts
    // and the weights' sum.  A family's parameters travel as kernel arguments: dev.gen (the level rule, the maze's loops and grid), dev.caves, dev.rooms.
    struct LayoutSource {
        RcwBuf words, cum, agents;
        RcwPinned h_cum;
        RcwEvent ev_cum;
        uint64_t total_weight = 0;
        RcwLayoutSource dev{};
        bool is(RcwLayoutKind k) const { return dev.kind == k; }
        bool live() const { return !is(kLayoutNone); }
    } source;
    // Episode statistics (rcw_set_episode_stats): ONE buffer — the head is the table (UInt64, 8 (1 + rows)), then the carve of its list;
    // dev's pointers point into it.  rows / first: fixed when enabled (plan_episode_stats_rows).  Empty while the feature is off.
    struct EpisodeStats {
        RcwBuf buf;
        RcwEpisodeStats dev{};
        bool on() const { return buf.get() != nullptr; }
        size_t table_bytes() const { return (size_t)RCW_EPISODE_STATS_ROW_WORDS * (1 + (size_t)dev.rows) * sizeof(uint64_t); }
    } stats;
    // The guide (rcw_set_guide): ONE buffer, the carve of its list — UInt8 (B) action, Int32 (B) heading; `words` points into it.  It holds
    // no pointer into the goal distance: the launch reads goal.field as it is THEN (rcw_set_goal_distance may have replaced it).  Empty while
    // the feature is off — and never on while the goal distance is off.
    struct Guide {
        RcwBuf buf;
        RcwGuideWords words{};
        bool on() const { return buf.get() != nullptr; }
    } guide;
    // The frontier (rcw_set_frontier): ONE buffer, the carve of its list — the Int32 (B) distance and tiles, the UInt8 (B) action and Int32
    // (B) heading the guide's kernel writes from this field, each agent's episode counter as of its last flood, the UInt16 (H*W, B) field; the
    // pointers point into it.  It holds no pointer into the seen map: the launch reads seen.map and seen.words as they are THEN
    // (rcw_set_seen_map may have replaced them).  Empty while the feature is off — and never on while the seen map is off.
    struct Frontier {
        RcwBuf buf;
        RcwFrontierWords words{};
        RcwGuideWords advice{};
        uint32_t* last_episode = nullptr;
        uint16_t* field = nullptr;
        bool on() const { return buf.get() != nullptr; }
    } frontier;
    // The visit map (rcw_set_visit_map): ONE buffer — the head is the table (UInt32 (cells, 1 + rows); empty without RCW_VISIT_TABLE), then the
    // carve of its list: the four words, each agent's episode counter as of its last BEGIN, the UInt16 (cells, B) map; dev's pointers point
    // into it.  sectors / flags / rows / first: fixed when enabled (plan_visit_table_rows).  Empty while the feature is off.
    struct VisitMap {
        RcwBuf buf;
        RcwVisitMap dev{};
        int32_t flags = 0;
        bool on() const { return buf.get() != nullptr; }
        bool table() const { return dev.table != nullptr; }
        size_t table_bytes() const { return table() ? (size_t)dev.cells * (1 + (size_t)dev.rows) * sizeof(uint32_t) : 0; }
    } visits;
    // The start rule (rcw_set_start_distance): ONE buffer, the carve of its list — each agent's episode counter as of its last start under the
    // rule, the UInt8 (B) `placed`, the mask of the last launch; dev's pointers point into it.  lo / hi: the band, a kernel argument of every
    // launch — changing it allocates nothing and waits for nothing.  Empty while the feature is off.
    struct StartRule {
        RcwBuf buf;
        RcwStartRule dev{};
        int32_t lo = 0, hi = 0;
        bool on() const { return buf.get() != nullptr; }
    } start;
    // The state archive (rcw_set_snapshots): ONE allocation — every segment's rows ([rows][bytes], each part on a multiple of 16 bytes), then
    // the Int32 scratch (owner [rows], the row each agent takes [B], the host variants' staged indices [B]), then the filled flags (UInt8
    // [rows]).  plan: the record's layout as of the binding (plan_snapshot); arc[k]: segment k's rows.  Empty while the archive is off.
    struct Snapshots {
        RcwBuf buf;
        SnapshotPlan plan{};
        int32_t rows = 0;
        uint8_t* arc[kSnapshotMaxSegments] = {};
        int32_t* owner = nullptr;
        int32_t* sel = nullptr;
        int32_t* in_rows = nullptr;
        uint8_t* filled = nullptr;
        bool on() const { return buf.get() != nullptr; }
    } snaps;
    ~rcw_handle();
};

// What a render does to the k-frame stack (include/rcw.h, "the frame stack"): a step pushes, reset! / set_state / a new view or direction
// table refill the (masked) agents' slots, a re-render of the very same frames (rcw_set_step_form) leaves it alone.
// kStackRefillSameWorld: a refill behind which no agent's world differs (a new direction table): the frames are new, goal and walls are not.
enum StackOp { kStackPush, kStackRefill, kStackRefillSameWorld, kStackKeep };

// What rcw_set_learner_view_stack's arguments ask of this geometry — the kernels' RcwView (rows / cols: the caller's, once `tab` is on the
// device) and the box tables — or the refusal.  Host arithmetic only: no HIP call, and nothing of a handle changes.
struct ViewPlan {
    RcwView v{};
    std::vector<int32_t> tab;      // rows [h + 1], then columns [w + 1], then (depth formats) RcwView::dsum [Hc + 1]; empty: RCW_VIEW_OFF
};

// Development switches: only a build with -DRCW_DEV_SWITCHES (make dev -> librcw_hip_dev.so) reads them.
#ifdef RCW_DEV_SWITCHES
#define RCW_DEV_ENV(name) std::getenv(name)
#else
#define RCW_DEV_ENV(name) (static_cast<const char*>(nullptr))
#endif

// ---- rcw_rules.hip: the host-built tables, every rule and validation — no HIP call, nothing of a handle changes ------------------------
template <typename T>
void build_direction_table(int nd, std::vector<T>& out);          // (both for T = float and double)
template <typename T>
void build_ray_table(const rcw_config& c, T fov, const std::vector<T>& dirs, std::vector<T>& out);
void set_geometry(RcwPlan& d, const rcw_config* cfg, int32_t batch);
int top_view_rule(RcwPlan& d, const rcw_config* cfg, size_t B, const RcwHw& hw, int want_form, int want_runs, bool lenient);
int top_form_alone(const RcwPlan& d, bool split);
int top_form_alone(const RcwPlan& d);
int top_form_in_step(const RcwPlan& d);
bool step_one_launch_pays(const RcwDev& d);
int validate_walls(int H, int W, int B, const uint8_t* walls, int layouts, const int32_t* index, const uint8_t* mask, char* msg, size_t cap);
int validate_config(const rcw_config* c, int32_t batch);
int plan_learner_view(const rcw_config& cfg, const RcwDev& dev, int32_t format, int32_t layout, int32_t height, int32_t width, int32_t flags,
                      int32_t frames, ViewPlan* plan);
int plan_local_map(int32_t source, int32_t size, int32_t cells_per_tile, bool real64, std::vector<unsigned char>* table);
int plan_wall_bank_weights(const uint32_t* weights, int32_t layouts, uint32_t* cum, uint64_t* total);
int plan_wall_generator(int32_t H, int32_t W, int32_t levels, int32_t first_level);
int plan_wall_caves(int32_t H, int32_t W, int32_t smooth, int32_t levels, int32_t first_level);
int plan_wall_rooms(int32_t H, int32_t W, int32_t room, int32_t levels, int32_t first_level);
void agent_arrays(const SnapshotShape& sh, int feature, AgentArrays* out);
AgentCarve carve_agent_arrays(uint64_t head, const AgentPart* part, int n, uint64_t B);
void plan_snapshot(const SnapshotShape& sh, SnapshotPlan* plan);
const char* snapshot_plan_differs(const SnapshotPlan& bound, const SnapshotPlan& now);   // the first segment that differs, NULL: the same shape
int validate_snapshot_row(const SnapshotShape& sh, const SnapshotPlan& plan, const uint8_t* row, char* msg, size_t cap);
void plan_episode_stats_rows(RcwLayoutKind kind, int32_t layouts, int32_t levels, int32_t first_level, int32_t* rows, int32_t* first);
void plan_visit_table_rows(const SnapshotShape& sh, int32_t* rows, int32_t* first);   // the visit table's level rows: the statistics' rule under the byte cap
int check_start_band(int32_t lo, int32_t hi);                     // RCW_OK: 1 <= lo <= hi <= RCW_START_DISTANCE_MAX
int guide_promised(const rcw_config& cfg);                        // 1: position_increment + player_radius <= 0.5 in the world-unit type

// ---- rcw_step.hip: what a step, a reset or a re-render launches, and the resources those launches need ---------------------------------
hipError_t launch_top_view_alone(rcw_handle* h, const uint8_t* mask_dev);
hipError_t paint_camera(rcw_handle* h, const uint8_t* mask_dev, hipStream_t stream);
hipError_t launch_view(rcw_handle* h, const uint8_t* mask_dev, StackOp op);
hipError_t launch_goal_distance(rcw_handle* h, const uint8_t* mask_dev, StackOp op);
hipError_t launch_seen_map(rcw_handle* h, const uint8_t* mask_dev, StackOp op);
hipError_t launch_local_map(rcw_handle* h, StackOp op);
hipError_t launch_episode_stats(rcw_handle* h, const uint8_t* mask_dev, StackOp op);
hipError_t launch_guide(rcw_handle* h, StackOp op);
hipError_t launch_frontier(rcw_handle* h, const uint8_t* mask_dev, StackOp op);
hipError_t launch_visit_map(rcw_handle* h, const uint8_t* mask_dev, StackOp op);
hipError_t launch_layout_source(rcw_handle* h, bool force);
hipError_t launch_start_distance(rcw_handle* h, bool force);
hipError_t launch_step(rcw_handle* h, const uint8_t* actions_dev, const uint8_t* mask_dev, StackOp op);
hipError_t launch_snapshot(rcw_handle* h, const int32_t* rows_dev, const uint8_t* mask_dev, bool restore);
hipError_t replace_buffers(rcw_handle* h, std::initializer_list<RcwBuf*> old, std::initializer_list<RcwBuf*> fresh = {});
int plan_top_view(rcw_handle* h, int want_form, int want_runs, bool lenient);
int plan_step_form(rcw_handle* h, int want);
int ensure_columns(rcw_handle* h);

// ---- rcw_comm.hip: RCCL and the gathers -------------------------------------------------------------------------------------------------
void drop_comm(rcw_handle* h);                                    // (~rcw_handle's)

// ---- rcw_api.hip: the C ABI ---------------------------------------------------------------------------------------------------------------
int check_handle(rcw_handle* h);
