// Device-side view of one batch of SingleRoom agents and the kernel launchers.
// State is structure-of-arrays in HBM, resident for the handle's lifetime.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Per-direction ray table: for heading d the slice is 5 rows of N floats
//   [dx | dy | |1/dx| | |1/dy| | dir . ray]
// so lane i of the cast phase reads five coalesced floats (SR:214-221, SR:404).
#define RCW_TABLE_ROWS 5

// The kernels' argument block, passed by value to every kernel: only what device code reads goes in here.  A choice the host makes
// about a launch (a grid, a block size, which kernel) belongs to RcwPlan below, where no kernel can see it.
struct RcwDev {
    // geometry / config (all wave-uniform, live in SGPRs)
    int32_t B, H, W, N, nd, Hc;
    int32_t nwords;          // 32-bit words of one agent's tile_map (2 per UInt64 chunk)
    int32_t real64;          // world-unit type T: 0 = Float32, 1 = Float64 (SR:259); the *64 members below
    float radius, radius_sq; // player_radius_wu, fl(r*r)            (CD:18)
    float inc;               // position_increment_wu                (UT:16-17)
    float goal_reward;       // SR:82 one(R), R = Float32
    double goal_reward64;    // one(R) for the other reward types (converted on store)
    int32_t reward_type;     // RCW_REWARD_*: element type R of `reward` (SR:33, SR:266)
    float num;               // fl(camera_height_tile_wu * N)        (SR:406)
    float two_fov;           // fl(2 * semi_field_of_view_wu)        (SR:406)
    double radius64, radius_sq64, inc64, num64, two_fov64;   // the same five in Float64
    uint32_t floor_color, ceiling_color;
    uint32_t colour[4];      // indexed by RCW_COLOUR_*              (SR:293-296)
    int32_t tie_le;          // RCW_DDA_TIE_X_FIRST_ON_LE
    int32_t dist_pre;        // RCW_DDA_DIST_PRE_INCREMENT
    int32_t auto_reset;
    int32_t oob_empty;       // RCW_OOB_TREAT_EMPTY
    int64_t agent_id_offset;
    uint64_t seed;
    // state (SR:21-40), one entry per agent
    float2* pos;             // player_position_wu (T = Float32)
    double2* pos64;          // player_position_wu (T = Float64)
    int32_t* dir;            // player_direction_au
    int2* goal;              // goal_position (1-based i, j)
    void* reward;            // R[B]
    uint8_t* done;
    uint32_t* episode;       // resets seen (keys the generator)
    uint32_t* tile_map;      // BitArray{3}(2,H,W).chunks viewed as 32-bit words, [B][nwords]
    // constants
    const float2* dir_table; // directions_wu [nd]
    const float* ray_table;  // [nd][RCW_TABLE_ROWS][N]
    const double2* dir_table64;   // the two tables in Float64
    const double* ray_table64;
    // outputs
    uint32_t* obs;           // camera_view UInt32 (Hc, N, B)
    int32_t* col_h;          // (N, B) height_line_pu by image column
    uint8_t* col_c;          // (N, B) colour id by image column
    uint32_t* top_view;      // optional env.top_view UInt32 (H*pu, W*pu, B)  SR:302
    int32_t pu;              // pu_per_tu
    int32_t top_rp;          // player_radius_pu = wu_to_pu(player_radius_wu, pu)  SR:469 (host-computed in T)
    int32_t top_lds;         // write-once LDS bit-plane kernel: the number of buffers in its ring (1..3); 0: in-place fallback
    int32_t top_unit_px;     // the two-kernel top view's store kernel's unit: 256 rows of an image column (a whole 1 KiB chunk), 128 or 64
    int32_t top_flat;        // ... with rcw_top_store_flat_kernel (any pixel scale >= 9): the image columns a 256-pixel chunk may touch; 0: the unit kernels
    int32_t top_plane_words; // ... and the words of one agent's region of top_plane in that form
    int32_t top_parts;       // draw workgroups an agent (two-kernel form on the side-stream / stand-alone path with rcw_top_store_kernel): 1, or 2..4 for few big images
    int32_t top_rotate;      // rcw_top_store_flat_kernel's wavefront -> chunk assignment turns by this many slots from group to group (33; development: RCW_TOP_ROTATE)
    uint32_t* top_plane;     // [B][W*pu][H*pu/32] ray-line bit plane of every agent (two-kernel top view)
    int2* top_hdr;           // [B] the player's pixel (ip, jp), 1-based  SR:468
    uint2* top_codes;        // [B][W][H*pu/256] 2-bit fill codes of a chunk's tiles
    int32_t* err;            // sticky error word of the handle (0 = ok); never blocks a step
    int32_t* status;         // per-agent sticky status
};

// The episode time limit (include/rcw.h, rcw_set_time_limit): what its kernels read.  An argument of its OWN, behind RcwDev, of the kernels
// that need it — the *_limit_kernel instantiations of the step (taken only while max_steps > 0) and the reset / set_state kernels — and not
// three more members of RcwDev: a larger RcwDev moves the arguments of every kernel of the library, and the compiler then allocates their
// scalar registers differently (tools/isa_diff.py against the build before: 168 of 170 kernels changed, some in length).  This way every
// kernel a limit-less handle runs keeps its code to the byte.
struct RcwLimit {
    uint32_t* episode_steps; // [B] act! calls the agent's episode has taken
    uint8_t* truncated;      // [B] 0/1: episode_steps >= max_steps && !done, as of the agent's last step
    int32_t max_steps;       // max_episode_steps; 0: no limit — steps neither read nor write the two arrays
};

// The host's launch plan: the argument block plus the decisions of set_geometry and top_view_rule that only launchers read.  A kernel
// launch takes its RcwDev part (the conversion to the base); a value a kernel needs does not go here but in RcwDev.
struct RcwPlan : RcwDev {
    int32_t fill_grid;       // workgroups of the fill kernel (the moving window = fill_grid KiB x 4)
    int32_t fill_plain;      // 1: plain stores, 0: non-temporal
    int32_t fill_flat;       // development build only (RCW_FILL_FLAT): rcw_fill_flat_kernel also where rcw_fill_window_kernel<2 / 4> applies
    int32_t cast_block;      // threads per agent in the cast kernel (multiple of 64, <= 256)
    int32_t top_grid;        // workgroups of the (persistent) write-once top view kernel
    int32_t top_split;       // 1: the two-kernel top view (draw kernel -> planes in HBM -> moving-window store kernel)
    int32_t top_alone_split; // rcw_update_top_view alone (no camera fill beside it) also takes the two-kernel form, back to back
    int32_t top_runs;        // the batch is drawn and stored in this many runs of agents (store of run r beside the drawing of run r + 1)
    int32_t top_draw_first;  // inside a step the drawing stays on the handle's stream and the camera fill goes to the side stream
    int32_t top_fused;       // a step's camera fill and top-view drawing go in ONE launch (rcw_fill256_draw_kernel) instead of two streams
    int32_t top_draw_block;  // threads of a draw-kernel workgroup: 256; a lane per ray (up to 1024) when the plane leaves room for few workgroups on a CU
    int32_t top_draw_block_alone;   // ... in rcw_update_top_view alone: 64 / 128 for batches of tens of thousands of small images
    int32_t top_store_plain; // the two-kernel form's store kernel: 1 plain stores, 0 non-temporal
    int32_t top_store_grid;  // ... and its workgroups (the moving window = top_store_grid KiB x 4)
    RcwLimit limit;          // the time limit's argument block: launchers pick the *_limit_kernel twins by it and hand it to them
};

struct RcwRayOut {           // rcw_rays(): SR:29-31,39 for agents [first, first+count)
    int64_t* stop_ij;        // (2, N, count)
    int64_t* hit_dim;        // (N, count)
    void* dist;              // (N, count) in T
    void* dirs;              // (2, N, count) in T
};

// Host entry points: const RcwPlan& where the function (or one it calls) reads a launch decision, const RcwDev& where the geometry is enough.
size_t rcw_step_lds_bytes(const RcwDev& p);

// act!(env, a) = cast kernel (dynamics + rays + projection -> column descriptors) followed by
// the fill kernel (descriptors -> pixels).  actions == nullptr: render only (after reset /
// set_state); mask == nullptr: all agents.
hipError_t rcw_launch_cast(const RcwPlan& p, const uint8_t* actions_dev, const uint8_t* mask_dev,
                           hipStream_t s, int first = 0, int count = -1);   // agents [first, first + count); -1: to the end
hipError_t rcw_launch_fill(const RcwPlan& p, const int32_t* col_h, const uint8_t* col_c, uint32_t* frames,
                           long long total_cols, const uint8_t* mask_dev, hipStream_t s);
// update_top_view!(env) SR:446-483 for every (unmasked) agent; needs p.top_view
hipError_t rcw_launch_top_view(const RcwPlan& p, const uint8_t* mask_dev, hipStream_t s);
// LDS bytes of the write-once top view kernel for this geometry, and the one-off preparation (raises the
// kernel's dynamic LDS limit when the bit planes need more than 64 KiB); sets nothing on the device.
size_t rcw_top_view_lds_bytes(const RcwDev& p);
// the two-kernel top view: eligibility of a geometry, its HBM scratch sizes, and the two launches
int rcw_top_split_unit(const RcwPlan& p);   // rows of a store-kernel unit (256 / 128 / 64), 0: geometry not taken
int rcw_top_flat_cols(const RcwPlan& p);    // rcw_top_store_flat_kernel: columns a chunk may touch, 0: geometry not taken
int32_t rcw_top_plane_words(const RcwDev& p);
int rcw_fill_flat_cols(const RcwDev& p);   // rcw_fill_flat_kernel: columns a chunk may touch at this camera height, 0: not taken
const char* rcw_fill_kernel_name(const RcwPlan& p, long long total_cols);   // the kernel rcw_launch_fill takes
int rcw_fill_takes_256(const RcwPlan& p, long long total_cols);              // ... is rcw_fill256_kernel (what the fused launches build on)
int rcw_fill_window_columns(const RcwPlan& p, long long total_cols);         // ... 0: rcw_fill256_kernel, 1 / 2 / 4: rcw_fill_window_kernel<M>, -1: another one (the one-launch step takes the first four)
size_t rcw_top_plane_bytes(const RcwDev& p);
size_t rcw_top_codes_bytes(const RcwDev& p);
struct RcwHw { int cus, lds_per_cu, waves_per_cu; };       // what the top view's rule needs of the device (hipDeviceProp_t: multiProcessorCount, sharedMemPerBlock, maxThreadsPerMultiProcessor / 64)
int rcw_top_draw_per_cu(const RcwDev& p, int draw_block, int lds_per_cu = 160 * 1024, int waves = 28);   // draw workgroups resident on a CU together: by LDS, by the wavefront slots the camera fill leaves
hipError_t rcw_launch_top_draw(const RcwPlan& p, const uint8_t* mask_dev, int first, int count, hipStream_t s, int block = 0);    // agents [first, first + count); block: threads a workgroup, 0 = p.top_draw_block
hipError_t rcw_launch_top_store(const RcwPlan& p, const uint8_t* mask_dev, int first, int count, hipStream_t s);
// the one-launch step (round 6): eligibility of a geometry, the bytes of one of its two slot buffers ([B][5][N] packed column words + [B] bytes), the launch
int rcw_step_spec_eligible(const RcwPlan& p);
size_t rcw_step_spec_slot_bytes(const RcwDev& p);
hipError_t rcw_launch_step_spec(const RcwPlan& p, const uint8_t* actions_dev, const uint8_t* mask_dev, const uint16_t* slots_in,
                                uint16_t* slots_out, bool with_fill, bool cols, bool keep, hipStream_t s);   // cols: the step also leaves the current frame's (height, colour id) descriptors; keep: p.obs holds every agent's current frame — unchanged frames are not stored again
int rcw_fill_draw_fusable(const RcwPlan& p);   // a step's camera fill + top-view drawing in one launch: this geometry takes it
hipError_t rcw_launch_fill256_draw(const RcwPlan& p, const uint8_t* mask_dev, hipStream_t s);   // (fills p.obs from p.col_h / p.col_c, draws every agent)
hipError_t rcw_prepare_top_view(const RcwDev& p, int device);
hipError_t rcw_launch_reset(const RcwPlan& p, const uint8_t* mask_dev, hipStream_t s);   // (both also zero the masked agents' RcwLimit words)
hipError_t rcw_launch_set_state(const RcwPlan& p, const int2* goal, const void* pos /* float2* or double2* */,
                                const int32_t* dir, const uint8_t* mask_dev, hipStream_t s);
hipError_t rcw_launch_init_tile_map(const RcwDev& p, hipStream_t s);
// rcw_set_walls: walls UInt8 (H*W, layouts) and index Int32 (B) in DEVICE memory; the (masked) agents' WALL layer := their layout, GOAL layer := 0
hipError_t rcw_launch_set_walls(const RcwDev& p, const uint8_t* walls_dev, const int32_t* index_dev, const uint8_t* mask_dev, hipStream_t s);
hipError_t rcw_launch_rays(const RcwDev& p, int32_t first, int32_t count, RcwRayOut out,
                           hipStream_t s);
hipError_t rcw_launch_expand(const RcwPlan& p, const int32_t* col_h, const uint8_t* col_c,
                             int32_t count, uint32_t* frames, hipStream_t s);

// The learner view (rcw_set_learner_view, rcw_view.hip): uint8 RGB or gray and / or inverse depth, area-averaged to (h, w), computed from
// the column descriptors.  Output row r averages camera rows [rows[r], rows[r+1]), column c image columns [cols[c], cols[c+1]).
struct RcwView {
    int32_t C;               // channels: 1 (gray, depth), 3 (RGB), 2 (gray + depth), 4 (RGB + depth)
    int32_t hwc;             // layout: 0 = (B, C, h, w), 1 = (B, h, w, C)
    int32_t h, w;            // output size, 1 <= h <= Hc, 1 <= w <= N
    const int32_t* rows;     // [h + 1] floor(r * Hc / h)
    const int32_t* cols;     // [w + 1] floor(c * N / w)
    int32_t wide;            // a box's channel sums may pass 2^31: 64-bit sums and divisions
    int32_t full_ok;         // (h, w) = (Hc, N) and the geometry rcw_view_full_kernel takes
    int32_t depth;           // 1: the last of the C channels is the depth plane (C - 1 colour channels in front of it)
    const int32_t* dsum;     // depth: [Hc + 1] prefix sums of the ceiling / floor depth byte De(y) over camera rows, dsum[0] = 0
};
// the view of agents [0, count) of the descriptors col_h / col_c (N a agent) into out (count * C * h * w bytes); mask: NULL = all
hipError_t rcw_launch_view(const RcwPlan& p, const RcwView& v, const int32_t* col_h, const uint8_t* col_c, int32_t count,
                           const uint8_t* mask_dev, uint8_t* out, hipStream_t s);
// The view with a k-frame stack (frames = k > 1, layout CHW): the frame of agents [0, count) pushed into (refill: written to all of) their
// `frames` slots of stack; episode / last_episode: the agents' counters now / as of their previous push (updated); mask: NULL = all.
// At the sizes rcw_view_agent_kernel takes: rcw_view_agent_push_kernel, the one kernel that does both and leaves `staged` alone; otherwise
// rcw_launch_view into `staged` (count * C * h * w bytes) and rcw_view_push_kernel behind it.
hipError_t rcw_launch_view_stack(const RcwPlan& p, const RcwView& v, const int32_t* col_h, const uint8_t* col_c, int32_t count, int frames,
                                 const uint8_t* mask_dev, uint8_t* staged, uint8_t* stack, const uint32_t* episode, uint32_t* last_episode,
                                 bool refill, hipStream_t s);
int rcw_view_full_eligible(const RcwDev& p, int C, int hwc);   // the full-resolution kernel takes this geometry and layout

// The goal distance (rcw_set_goal_distance, rcw_goal_distance.hip): the three Int32 (B) words beside the UInt16 (H*W, B) field.
struct RcwGoalWords {
    int32_t* distance;       // field[player's tile], -1: unreachable or off the map
    int32_t* start_distance; // ... as of the start of the agent's episode
    int32_t* progress;       // what the last call brought the agent closer by
};
// One launch behind a step (refill = false: an agent whose episode counter differs from last_episode floods, every other one looks its tile
// up and takes progress = old - new) or behind reset / set_state / set_walls / enabling (refill = true: the agents of the mask — NULL: all —
// flood and take start_distance = distance, progress = 0; the others are left alone).  Reads p's state arrays, writes only its own buffers.
size_t rcw_goal_distance_lds_bytes(const RcwDev& p);
hipError_t rcw_launch_goal_distance(const RcwDev& p, int32_t B, const uint8_t* mask_dev, bool refill, uint16_t* field, const RcwGoalWords& words,
                                    uint32_t* last_episode, hipStream_t s);

// The seen map (rcw_set_seen_map, rcw_seen_map.hip): the three Int32 (B) words beside the UInt8 (H*W, B) map.
struct RcwSeenWords {
    int32_t* seen_count;     // non-zero entries of the agent's map
    int32_t* newly_seen;     // entries the last call turned from 0 to non-zero; 0 behind a clear
    int32_t* goal_seen;      // map[goal tile] != 0
};
// One launch behind a step (refill = false: an agent whose episode counter differs from last_episode is cleared and marked afresh, every
// other one is marked on top of what it has) or behind reset / set_state / set_walls / enabling (refill = true: the agents of the mask —
// NULL: all — are cleared and marked; the others are left alone).  seen_bits: the packed map, (H*W + 31) / 32 words an agent.  Reads p's
// state arrays and ray table, writes only its own buffers.
size_t rcw_seen_map_lds_bytes(const RcwDev& p);
hipError_t rcw_launch_seen_map(const RcwDev& p, int32_t B, const uint8_t* mask_dev, bool refill, uint8_t* map, uint32_t* seen_bits,
                               const RcwSeenWords& words, uint32_t* last_episode, hipStream_t s);

// The local map (rcw_set_local_map, rcw_local_map.hip): per agent an UInt8 (size, size) crop of its tile map — or, seen_map != NULL, of its
// seen map ([B][H*W]) — around its position, its heading up.  off: the offset table, `size` entries of the world-unit type in DEVICE memory
// (plan_local_map); out: [B][size*size], 4-byte aligned.  One launch, every agent; reads p's state arrays and direction table, writes only out.
size_t rcw_local_map_lds_bytes(const RcwDev& p, int32_t size, bool seen);
hipError_t rcw_launch_local_map(const RcwDev& p, int32_t B, const uint8_t* seen_map, const void* off, int32_t size, uint8_t* out, hipStream_t s);

// Episode statistics (rcw_set_episode_stats, rcw_episode_stats.hip): the seven per-agent words, the two private ones and the table.
struct RcwEpisodeWords {
    uint8_t* finished;       // 1 iff the last call closed the agent's record
    uint8_t* outcome;        // RCW_EPISODE_OPEN / SUCCESS / TRUNCATED
    uint32_t* length;        // step calls the record has lived through
    uint32_t* moves;         // ... after which the position differed
    int32_t* level;          // the layout as of the close, -1 while open or without a layout source
    int32_t* spl_q16;        // SPL * 65536 as of the close, -1 while open or where it is undefined
    uint32_t* episodes;      // records the agent has closed
};
struct RcwEpisodeStats {
    RcwEpisodeWords words;
    uint32_t* last_episode;  // [B] each agent's episode counter as of the beginning of its record
    void* prev_x;            // [B] its position behind the previous call, in the world-unit type, x and y apart
    void* prev_y;
    uint64_t* table;         // UInt64 (RCW_EPISODE_STATS_ROW_WORDS, 1 + rows)
    int32_t rows, first;     // the level rows: row 1 + k takes the closes with level == first + k
};
// One launch behind a step (refill = false: an agent whose episode counter differs from last_episode begins a record, a closed record stays
// frozen, an open one lives through the call and closes where done | truncated) or behind reset / set_state / set_walls / enabling (refill =
// true: the agents of the mask — NULL: all — begin, the others' `finished` is cleared).  An argument block of its OWN (the comment on
// RcwLimit): no kernel of a handle without the statistics changes.  layout, start_distance: as they are NOW, NULL where the handle has no
// layout source / no goal distance.  Reads p's state arrays and limit.truncated, writes only st's buffers.
hipError_t rcw_launch_episode_stats(const RcwDev& p, const RcwLimit& limit, const RcwEpisodeStats& st, const int32_t* layout,
                                    const int32_t* start_distance, const uint8_t* mask_dev, bool refill, hipStream_t s);

// The guide (rcw_set_guide, rcw_guide.hip): the two per-agent words.
struct RcwGuideWords {
    uint8_t* action;         // 1..4: what rcw_step_device takes as it stands
    int32_t* heading;        // the direction index the guide wants the agent to face, -1: no advice
};
// One launch, every agent: the rule of include/rcw.h ("the guide") on `field` — the goal distance's, [B][H*W] —, p's positions, headings and
// direction table as they are when it runs.  An argument block of its OWN (the comment on RcwLimit).  Reads only; writes only the two words.
hipError_t rcw_launch_guide(const RcwDev& p, int32_t B, const uint16_t* field, const RcwGuideWords& words, hipStream_t s);

// The frontier (rcw_set_frontier, rcw_frontier.hip): the two Int32 (B) words beside the UInt16 (H*W, B) field.
struct RcwFrontierWords {
    int32_t* distance;       // field[player's tile], -1: nothing left to explore from there, or off the map
    int32_t* tiles;          // the sources of the agent's last flood
};
// One launch directly behind the seen map's.  Behind a step (refill = false): an agent whose episode counter differs from last_episode, or
// whose newly_seen word is not 0, floods — the sources are the unseen tiles of `seen_map` next to a seen passable one —; every other one
// looks its tile up.  Behind reset / set_state / set_walls / a restore / enabling (refill = true): the agents of the mask — NULL: all —
// flood, the others are left alone.  An argument block of its OWN (the comment on RcwLimit).  Reads p's positions and counters, the seen
// map and its word; writes only field, words and last_episode.
size_t rcw_frontier_lds_bytes(const RcwDev& p);
hipError_t rcw_launch_frontier(const RcwDev& p, int32_t B, const uint8_t* mask_dev, bool refill, const uint8_t* seen_map, const int32_t* newly_seen,
                               uint16_t* field, const RcwFrontierWords& words, uint32_t* last_episode, hipStream_t s);

// The visit map (rcw_set_visit_map, rcw_visit_map.hip): the UInt16 (cells, B) map, the four per-agent words, the private counter and the
// table, cells = sectors * H * W.
struct RcwVisitMap {
    uint16_t* map;           // [B][cells] how often the agent has stood in each cell this episode, saturating at 65535
    int32_t* here;           // [B] the entry of the agent's cell after the call; 0: no cell
    int32_t* visited;        // [B] non-zero entries of the agent's map
    int32_t* first;          // [B] 1 iff the call counted a cell whose entry was 0; 0 behind a BEGIN
    uint32_t* level_here;    // [B] the table's entry of the agent's (row, cell) as of the end of the call; 0 without the table
    uint32_t* last_episode;  // [B] each agent's episode counter as of its last BEGIN
    uint32_t* table;         // UInt32 (cells, 1 + rows); NULL: no table
    int32_t sectors, cells;
    int32_t rows, first_level;   // the level rows: row 1 + k takes the counts with layout == first_level + k
};
// One launch behind a step (refill = false: an agent whose episode counter differs from last_episode gets BEGIN — its map cleared, then
// counted —, every other one COUNT at its pose) or behind reset / set_state / set_walls / enabling (refill = true: BEGIN for the agents of
// the mask — NULL: all —, the others are left alone); with a table a second, lane-per-agent launch (rcw_visit_table_read_kernel) that only
// reads follows and leaves level_here for every agent.  An argument block of its OWN (the comment on RcwLimit): no kernel of a handle
// without the visit map changes.  layout: as it is NOW, NULL where the handle has no layout source.  Reads p's positions, headings and
// counters, writes only vm's buffers.
hipError_t rcw_launch_visit_map(const RcwDev& p, int32_t B, const RcwVisitMap& vm, const int32_t* layout, const uint8_t* mask_dev, bool refill, hipStream_t s);

// THE LAYOUT SOURCES (rcw_wall_bank.hip): what gives an agent its walls at every start of an episode.  A handle has at most one — the wall
// bank (rcw_set_wall_bank) or one family of the wall generator: mazes (rcw_set_wall_generator), caves (rcw_set_wall_caves), rooms
// (rcw_set_wall_rooms) — behind ONE launch point, rcw_launch_layout_source.
enum RcwLayoutKind { kLayoutNone, kLayoutBank, kLayoutMazes, kLayoutCaves, kLayoutRooms };

// The per-agent arrays of every source and, of the bank, its layouts: what the kernels read and write, all in DEVICE memory.
struct RcwWallBank {
    int32_t layouts;             // the bank: L >= 1; a generator family: 0, words and cum NULL
    const uint32_t* words;       // [L][nwords] the layouts in the tile map's word format: WALL bits set, GOAL bits and the padding clear
    const uint32_t* cum;         // [L] cumulative weights, cum[L - 1] = the sum (1 .. 2^32 - 1)
    uint32_t* last_episode;      // [B] each agent's episode counter as of its last start under the source
    int32_t* status_seen;        // [B] ... and its status word as of then
    int32_t* layout;             // [B] the layout the agent's episode was given: the bank's index, a family's level or -1 (rcw_wall_layout)
    uint8_t* mask;               // [B] 1: the launch gave the agent a layout and a fresh state — the host re-renders these
};
// The level rule of the generator families and the maze's own parameters: kernel arguments, fixed at install.
struct RcwWallGen {
    uint32_t loops;              // mazes: a non-tree edge is opened where the high word of its draw is below this; caves, rooms: 0
    int32_t levels, first_level; // levels == 0: a layout of its own every episode; else level first_level + below(u, levels)
    uint64_t level_seed;
    int32_t ni, nj;              // the maze's cell grid (the caves' fallback too): (H - 1) / 2 by (W - 1) / 2, ni * nj <= kWallGenMaxCells; rooms: 0, 0
};
constexpr int kWallGenMaxCells = 4096;
struct RcwWallCaves {            // the caves' own two kernel arguments
    uint32_t fill;               // an interior tile is WALL in generation 0 where the high word of its draw is below this
    int32_t smooth;              // smoothing steps, 0 .. kWallCavesMaxSmooth
};
constexpr int kWallCavesMaxTiles = 4096;   // (H - 2)(W - 2): maps up to 66 x 66
constexpr int kWallCavesMaxSmooth = 8;
struct RcwWallRooms {            // the rooms' own three kernel arguments
    int32_t room;                // the least side of a room, >= 1
    uint32_t stop;               // a chamber other than the root is left whole where the high word of its stop draw is below this
    uint32_t doors;              // a wall gets a second door where the high word of its draw is below this
};
constexpr int kWallRoomsMaxRooms = 4096;   // Q = ceil((H - 2) / 2) ceil((W - 2) / 2): 130 x 130, 5 x 4097
constexpr int kWallRoomsMaxTiles = 65536;  // H W: a chamber's two corner tiles share one draw index
inline long long rcw_wall_rooms_bound(int H, int W) { return (long long)((H - 1) / 2) * (long long)((W - 1) / 2); }   // (ceil((H - 2) / 2) = (H - 1) / 2)

// The live source as its launcher reads it.  What is not of the live kind is zero: the bank has no gen / caves / rooms, a family only the
// per-agent arrays of `agents`, mazes no caves / rooms, and so on.
struct RcwLayoutSource {
    RcwLayoutKind kind;
    RcwWallBank agents;
    RcwWallGen gen;
    RcwWallCaves caves;
    RcwWallRooms rooms;
};
// One launch behind the core launches of a call that can move an episode counter, a wavefront an agent: an agent whose counter differs from
// last_episode (force: every agent) takes a layout of the live kind — drawn from the bank, or made in LDS — and is reset against it under its
// episode's own key (counter: what the launch in front left); mask[a] says who.  hipSuccess and no launch without a live source,
// hipErrorInvalidValue for a geometry past the live family's bound (the plan_wall_* rules refuse those first).
hipError_t rcw_launch_layout_source(const RcwPlan& p, const RcwLayoutSource& src, bool force, hipStream_t s);
// The layouts UInt8 (H*W, layouts) in device memory -> words; one launch, once per rcw_set_wall_bank.
hipError_t rcw_launch_wall_bank_pack(const RcwDev& p, const uint8_t* walls_dev, uint32_t* words_dev, int32_t layouts, hipStream_t s);
// The camera view (p.obs) of the agents with mask[a] != 0 from p.col_h / p.col_c, a workgroup an agent: the repaint behind
// rcw_launch_layout_source, whose mask is sparse — the camera fill's pixels, without its sweep over the whole batch.
hipError_t rcw_launch_wall_bank_paint(const RcwDev& p, const uint8_t* mask_dev, hipStream_t s);

// The start rule (rcw_set_start_distance, rcw_start_distance.hip): the three per-agent arrays.
struct RcwStartRule {
    uint32_t* last_episode;  // [B] each agent's episode counter as of its last start under the rule
    uint8_t* placed;         // [B] RCW_START_NOT_YET / IN_BAND / CLAMPED / KEPT: how the agent's last start went
    uint8_t* mask;           // [B] 1: the launch began an episode of the agent — the host re-renders these
};
// One launch directly behind rcw_launch_layout_source, a wavefront an agent: an agent whose counter differs from last_episode (force: every
// agent) floods from its goal in LDS and is moved to a tile of the band [lo, hi] drawn under its episode's key (include/rcw.h, "the start
// rule"); mask[a] says who.  An argument block of its OWN (the comment on RcwLimit): no kernel of a handle without the rule changes.  The band
// travels in the kernel's arguments.  Reads p's goals, counters and tile maps; writes p's positions and rule's arrays.
size_t rcw_start_distance_lds_bytes(const RcwDev& p);
hipError_t rcw_launch_start_distance(const RcwDev& p, const RcwStartRule& rule, uint32_t lo, uint32_t hi, bool force, hipStream_t s);

// THE STATE ARCHIVE (rcw_snapshot.hip): a record is a list of segments, each [B][bytes] live and [rows][bytes] in the archive.  The copy
// kernel's table, passed by value: at most kSnapshotKernelSegments a launch.  first_task: the segment's first wavefront task (rcw_snapshot_tasks
// of them each, numbered through the table); tasks: their sum.
constexpr int kSnapshotKernelSegments = 32;
struct RcwSnapshotSeg {
    uint8_t* live;               // the handle's array
    uint8_t* rows;               // the archive's
    uint32_t bytes;              // of one agent's part
    uint32_t first_task;
};
struct RcwSnapshotTable {
    int32_t n;
    uint32_t tasks;
    RcwSnapshotSeg seg[kSnapshotKernelSegments];
};
uint32_t rcw_snapshot_tasks(uint32_t bytes, int32_t B);
// Who takes which row: sel[a] = rows[a] (NULL: a) of the agents of the mask (NULL: all), -1 for the others and for an index outside [0, nrows)
// or (restore) an unfilled row — those agents' status words and the error word become RCW_ERR_INVALID_ARGUMENT.  A save marks the rows filled
// and leaves in owner (-1 everywhere before) the highest agent that saves into each.
hipError_t rcw_launch_snapshot_resolve(const RcwDev& p, int32_t B, const int32_t* rows_dev, const uint8_t* mask_dev, int32_t nrows, bool restore,
                                       uint8_t* filled, int32_t* owner, int32_t* sel, hipStream_t s);
// The copy of the table's segments, live -> rows (restore = false; owner: only the row's owner writes it) or rows -> live (owner NULL).
hipError_t rcw_launch_snapshot_copy(const RcwSnapshotTable& t, int32_t B, const int32_t* sel, const int32_t* owner, bool restore, int grid_cap, hipStream_t s);
