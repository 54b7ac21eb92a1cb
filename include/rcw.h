/*
 * rcw.h — C ABI of librcw_hip: batched SingleRoom step/render on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE path of RayCastWorlds.jl: the SingleRoom
 * step/render hot path.  The reference has no FFI of its own on this path (it is
 * Julia calling Julia), so each entry point below cites the reference method it
 * replaces (paths relative to the reference tree; SR = src/single_room.jl).
 * The Julia-side binding a maintainer would add is shown in INTEGRATION.md and
 * shipped in julia/BatchedSingleRoom.jl.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types.
 *   - Every call returns RCW_OK (0) or a negative RCW_ERR_* code; the message for the
 *     last failure on the calling thread is available from rcw_last_error().
 *   - One caller thread per handle (the reference is single threaded).  All work of a
 *     handle is ordered on one HIP stream.  rcw_step, rcw_reset and rcw_set_state may
 *     return before the GPU has finished; every getter and rcw_sync() waits.
 *   - There is NO CPU fallback in this library: rcw_create fails with
 *     RCW_ERR_NO_DEVICE when no gfx950 device is usable.
 *   - Indices handed over the boundary are the reference's: tiles are 1-based (i, j),
 *     actions are 1..4, directions are 0..num_directions-1.
 *   - Batched layouts are the reference's single-agent (column-major) layouts with a
 *     trailing batch axis, i.e. what a Julia caller would unsafe_wrap:
 *       camera_view  UInt32 (H_cam, N, B)          SR:300
 *       tile_map     BitArray{3}(2, H, W).chunks   SR:54   -> UInt64 (nchunks, B)
 *       position     Float32 (2, B)                SR:24
 *       rays         Int64 (2, N, B), Int64 (N, B), Float32 (N, B), Float32 (2, N, B)
 *                                                   SR:29-31,39
 */
#ifndef RCW_H
#define RCW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCW_ABI_VERSION 4

#if defined(__GNUC__)
#define RCW_API __attribute__((visibility("default")))
#else
#define RCW_API
#endif

/* ---- error codes ------------------------------------------------------------------ */
#define RCW_OK                    0
#define RCW_ERR_INVALID_ARGUMENT -1  /* NULL pointer, bad size, bad config value          */
#define RCW_ERR_INVALID_ACTION   -2  /* action outside 1..4 (stands in for @assert SR:140) */
#define RCW_ERR_NO_DEVICE        -3  /* no usable gfx950 device / HIP runtime failure      */
#define RCW_ERR_OUT_OF_MEMORY    -4
#define RCW_ERR_OUT_OF_BOUNDS    -5  /* a tile index left the map (Julia: BoundsError at
                                        collision_detection.jl:35 or inside cast_ray)      */
#define RCW_ERR_HIP              -6  /* any other HIP error; text in rcw_last_error()      */
#define RCW_ERR_UNSUPPORTED      -7
/* A per-agent status WARNING (rcw_status), not an error: no call fails on it and the handle's error word stays clear.
 * sample_empty_position (utils.jl:23-37) gave up after max_tries = 1024*H*W occupied draws and reset!(world) placed the player
 * on the last — occupied — tile drawn; the reference @warns there (utils.jl:34) and goes on.  Only a map without an empty tile
 * (3x3: the one interior tile is the goal) gets here. */
#define RCW_WARN_SAMPLER_GAVE_UP  1

/* ---- objects, actions (SR:16-19) --------------------------------------------------- */
#define RCW_NUM_OBJECTS 2
#define RCW_WALL        1
#define RCW_GOAL        2
#define RCW_NUM_ACTIONS 4
#define RCW_ACTION_MOVE_FORWARD  1   /* SR:486 get_action_names */
#define RCW_ACTION_MOVE_BACKWARD 2
#define RCW_ACTION_TURN_LEFT     3
#define RCW_ACTION_TURN_RIGHT    4

/* Column colour ids used by the compact per-column descriptor (SR:417-429). */
#define RCW_COLOUR_WALL_DIM_1 0
#define RCW_COLOUR_WALL_DIM_2 1
#define RCW_COLOUR_GOAL_DIM_1 2
#define RCW_COLOUR_GOAL_DIM_2 3

/* The three choices inside the un-vendored dependencies that the reference's own tests
 * do not pin (DESIGN.md "parity unpinned").  They live here, in ONE
 * place, so a maintainer with a Julia toolchain can flip them without touching code;
 * tests/golden/discriminators.json holds poses where the two readings of each differ and
 * julia/make_reference_fixtures.jl dumps what the real package computes for them.
 * A fourth unpinned piece has no switch: the direction table (SR:65-69) is built with the C
 * library's cos / sin, Julia uses its own implementations — both < 1 ulp in Float64, so a
 * last-bit difference is possible (plausible for T = Float64, ~1e-8 per entry for Float32).
 * rcw_set_direction_table[64] lets the caller hand over Julia's table. */
#define RCW_DDA_TIE_X_FIRST_ON_LT 0  /* step in x when side_x <  side_y (default)          */
#define RCW_DDA_TIE_X_FIRST_ON_LE 1  /* step in x when side_x <= side_y                    */
#define RCW_DDA_DIST_SIDE_MINUS_DELTA 0 /* distance = side - delta after the step (default) */
#define RCW_DDA_DIST_PRE_INCREMENT    1 /* distance = side before it was incremented       */
#define RCW_NORMALIZE_INV_NORM_TIMES 0  /* inv(norm(v)) * v  (StaticArrays 1.2, default)    */
#define RCW_NORMALIZE_DIVIDE         1  /* v / norm(v)                                      */

/* What a move does when is_player_colliding (collision_detection.jl:30-35) would index a
 * tile off the map.  The reference raises BoundsError there — and this is reachable at the
 * defaults: walking along +x (heading 0) or +y (heading nd/4) in exact 1/8 steps reaches
 * x = H - 1 - 1/8, which does not collide (strict `<`, CD:18); the next forward move tests
 * x = H - 1, whose tile is H, and reads tile H + 1.
 *   RCW_OOB_ERROR        the faulting agent is left exactly as it was (as the Julia world is
 *                        after the exception), its status word and the handle's error word
 *                        are set to RCW_ERR_OUT_OF_BOUNDS (reported by the next
 *                        rcw_sync/getter, cleared by rcw_clear_error); other agents and
 *                        later steps are not affected.
 *   RCW_OOB_TREAT_EMPTY  tiles off the map count as empty; no error (the move above is then
 *                        simply blocked by the wall tile). */
#define RCW_OOB_ERROR       0
#define RCW_OOB_TREAT_EMPTY 1

/* R of SingleRoom(; R = ...) SR:266: the element type of world.reward / world.goal_reward (SR:33-34).  The
 * reference only ever stores zero(R) (SR:81, SR:131, SR:170-186) and goal_reward = one(R) (SR:82) in it. */
#define RCW_REWARD_FLOAT32 0   /* default */
#define RCW_REWARD_FLOAT64 1
#define RCW_REWARD_INT32   2
#define RCW_REWARD_INT64   3

/* Mirrors the keyword arguments of SingleRoom(; ...) SR:258-272 and the colour
 * constants SR:288-296.  Fill with rcw_config_default() and then override. */
typedef struct rcw_config {
    int32_t  abi_version;             /* RCW_ABI_VERSION                                   */
    int32_t  height_tile_map_tu;      /* SR:260  default 8  (x axis, index i)              */
    int32_t  width_tile_map_tu;       /* SR:261  default 16 (y axis, index j)              */
    int32_t  num_directions;          /* SR:262  default 128                               */
    int32_t  num_rays;                /* SR:268  default 512 (= camera view width)         */
    int32_t  height_camera_view_pu;   /* SR:271  default 256                               */
    int32_t  pu_per_tu;               /* SR:269  default 32 (pixels per tile of the top view) */
    float    player_radius_wu;        /* SR:263  default 1/8, must be in (0, 0.5)          */
    float    position_increment_wu;   /* SR:264  default 1/8                               */
    float    semi_field_of_view_wu;   /* SR:267  default Float32(2/3)                      */
    float    camera_height_tile_wu;   /* SR:270  default 1                                 */
    float    goal_reward;             /* SR:82   one(R) for R = Float32; other R: goal_reward_f64 */
    uint32_t floor_color;             /* SR:291  0x00404040                                */
    uint32_t ceiling_color;           /* SR:292  0x00FFFFFF                                */
    uint32_t wall_dim_1_color;        /* SR:293  0x00808080                                */
    uint32_t wall_dim_2_color;        /* SR:294  0x00c0c0c0                                */
    uint32_t goal_dim_1_color;        /* SR:295  0x00800000                                */
    uint32_t goal_dim_2_color;        /* SR:296  0x00c00000                                */
    int32_t  dda_tie_break;           /* RCW_DDA_TIE_*                                     */
    int32_t  dda_distance;            /* RCW_DDA_DIST_*                                    */
    int32_t  normalize_mode;          /* RCW_NORMALIZE_*                                   */
    int32_t  auto_reset;              /* 0 (reference behaviour: none) | 1: an agent whose
                                         `done` is set is re-sampled by the NEXT step call
                                         (its action is ignored, reward 0, done false)     */
    int64_t  agent_id_offset;         /* global id of local agent 0 (multi-GPU sharding);
                                         keys the reset RNG so results do not depend on
                                         how agents are sharded                            */
    int32_t  reward_type;             /* RCW_REWARD_*: R of SingleRoom(; R = ...) SR:266; the reward array
                                         (rcw_reward_typed, rcw_reward_device_ptr) has this element type  */
    int32_t  out_of_bounds;           /* RCW_OOB_ERROR (default, reference behaviour) |
                                         RCW_OOB_TREAT_EMPTY                               */
    int32_t  render_top_view;         /* 1: every reset/step also renders the top view
                                         (update_top_view! SR:446-483); default 0 — the
                                         reference always does, but it is a debug view, not the
                                         observation, and it doubles the bytes per step          */
    int32_t  world_unit_bits;         /* T of SingleRoom(; T = ...) SR:259: 32 (Float32, default) or 64
                                         (Float64).  With 64 the four world-unit parameters are
                                         taken from the *_f64 fields below (convert(T, 2/3) is
                                         not the Float32 value widened), positions / rays / tables
                                         cross the boundary as double (the *64 entry points), and
                                         every Float32 operation of the path becomes the same
                                         Float64 operation.  R (reward_type) is independent of T. */
    double   player_radius_wu_f64;    /* SR:263 convert(Float64, 1/8)                           */
    double   position_increment_wu_f64;
    double   semi_field_of_view_wu_f64;
    double   camera_height_tile_wu_f64;
    double   goal_reward_f64;         /* SR:82 one(R) for R = Float64 / Int32 / Int64 (converted to R)     */
    int32_t  reserved[2];
} rcw_config;

typedef struct rcw_handle rcw_handle;   /* opaque */

/* Reference defaults of SingleRoom(; ...) SR:258-272, SR:288-296. */
RCW_API int rcw_config_default(rcw_config* cfg);

/* SingleRoom(; kwargs...) SR:258-324 for `batch` independent agents on HIP device
 * `device` (>= 0).  Allocates structure-of-arrays state, the per-(direction, ray) table
 * (SR:65-69, SR:214-221) and the UInt32 (H_cam, N, B) observation batch in HBM.
 * The initial state is rcw_reset(h, NULL, seed). */
RCW_API int rcw_create(const rcw_config* cfg, int32_t batch, int32_t device, uint64_t seed,
               rcw_handle** out);
RCW_API int rcw_destroy(rcw_handle* h);

/* Replace the direction table directions_wu (SR:65-69) by a caller-computed one
 * (Float32 (2, num_directions)), e.g. Julia's own cos/sin, and rebuild the ray table. */
RCW_API int rcw_set_direction_table(rcw_handle* h, const float* directions_wu);

/* Use a caller-owned HIP stream (hipStream_t passed as void*); NULL restores the
 * handle's own stream.  The caller keeps the stream alive. */
RCW_API int rcw_set_stream(rcw_handle* h, void* hip_stream);
/* The stream the handle's work is ordered on (hipStream_t as void*), e.g. to make it wait for the
 * producer of device-resident actions or to order a consumer of the observations behind a step. */
RCW_API int rcw_get_stream(rcw_handle* h, void** hip_stream);
/* Render into a caller-owned DEVICE buffer of B*N*H_cam UInt32 instead of the
 * library's (NULL restores it).  Takes effect at the next render; does not synchronise, so a
 * caller can alternate two buffers while the previous frame batch is still being consumed. */
RCW_API int rcw_bind_obs(rcw_handle* h, void* device_ptr);

/* RCW.reset!(env) SR:326-331 -> SR:110-137 for the agents whose mask byte is non-zero
 * (mask == NULL: all).  Sampling is done on the device with a counter-based generator
 * keyed (seed, global agent id, episode number): goal uniform on interior tiles
 * (SR:120), player uniform on empty tiles by rejection (utils.jl:23-58) at the tile
 * centre (SR:125), heading uniform on 0..nd-1 (SR:128); reward 0, done false
 * (SR:131-132); rays cast and camera view rendered (SR:134, SR:329).
 * The stream is the build's own (Julia's RNG streams are not reproducible across
 * Julia versions): parity with the reference is in distribution only. */
RCW_API int rcw_reset(rcw_handle* h, const uint8_t* mask_host, uint64_t seed);

/* Inject the post-reset state the reference would have after SR:118-132 (this is how
 * "identical seeds" is realised): goal_ij Int32 (2, B) 1-based,
 * position_wu Float32 (2, B), direction_au Int32 (B); mask as above.  Clears the old
 * goal bit, sets the new one, zeroes reward/done, casts and renders. */
RCW_API int rcw_set_state(rcw_handle* h, const int32_t* goal_ij, const float* position_wu,
                  const int32_t* direction_au, const uint8_t* mask_host);

/* Float64 worlds (cfg.world_unit_bits = 64): the same calls with double arrays.  The Float32
 * forms return RCW_ERR_UNSUPPORTED on a Float64 handle and vice versa. */
RCW_API int rcw_set_state64(rcw_handle* h, const int32_t* goal_ij, const double* position_wu,
                            const int32_t* direction_au, const uint8_t* mask_host);
RCW_API int rcw_position64(rcw_handle* h, double* out_host /* (2, B) */);
RCW_API int rcw_rays64(rcw_handle* h, int32_t first, int32_t count, int64_t* stop_ij, int64_t* hit_dimension,
                       double* distance_wu, double* directions_wu);
RCW_API int rcw_set_direction_table64(rcw_handle* h, const double* directions_wu);
RCW_API int rcw_ray_table64(rcw_handle* h, double* out_host);
RCW_API int rcw_direction_table64(rcw_handle* h, double* out_host);

/* RCW.act!(env, action) SR:333-340 (minus update_top_view!) for every agent:
 * dynamics SR:139-191 -> cast_rays! SR:195-231 -> update_camera_view! SR:374-444.
 * actions: UInt8 (B), values 1..4, in HOST memory.  Any value outside 1..4 returns
 * RCW_ERR_INVALID_ACTION and NO agent is mutated (@assert SR:140). */
RCW_API int rcw_step(rcw_handle* h, const uint8_t* actions_host);
/* Same with actions already in DEVICE memory (stream-ordered, no host round trip).  Each
 * agent's action is checked on the device by the workgroup that steps it: an agent given a
 * value outside 1..4 is NOT stepped (its state and frame stay as they were), its status
 * word and the handle's error word are set to RCW_ERR_INVALID_ACTION, and the other agents
 * step normally — what a loop `for (env, a) in zip(envs, actions) act!(env, a)` over
 * reference worlds leaves behind, except that agents after the faulting one also run.
 * The error is returned by the next rcw_sync()/getter and cleared by rcw_clear_error. */
RCW_API int rcw_step_device(rcw_handle* h, const uint8_t* actions_device);

/* The three renderers of the reference as separate calls, for every agent, stream-ordered like rcw_step:
 *   rcw_cast_rays            RCW.cast_rays!(world) SR:195-231: recompute the rays (and with them the compact
 *                            column descriptors) from the current state; no pixel is written.
 *   rcw_update_camera_view   RCW.update_camera_view!(env) SR:374-444: refill camera_view from the stored ray
 *                            results, without casting (as in the reference, whose update_*_view! never cast).
 *   rcw_update_top_view      RCW.update_top_view!(env) SR:446-483 (needs cfg.render_top_view).
 * rcw_step / rcw_reset / rcw_set_state already do all of them; these exist because the reference exports them. */
RCW_API int rcw_cast_rays(rcw_handle* h);
RCW_API int rcw_update_camera_view(rcw_handle* h);
RCW_API int rcw_update_top_view(rcw_handle* h);

RCW_API int rcw_sync(rcw_handle* h);
RCW_API int rcw_clear_error(rcw_handle* h);

/* RLBase.state(env) SR:576: the camera view batch, aliased — the pointer is stable for
 * the handle's lifetime (or until rcw_bind_obs).  The buffer is the library's between calls: after every step it
 * equals the reference's camera_view for every agent, and a step may leave untouched the frames of agents whose view
 * it did not change (the one-launch step does not store them again).  A caller that writes into the buffer calls
 * rcw_update_camera_view or rcw_bind_obs before the next step; rcw_bind_obs — also with the pointer the handle already
 * has — makes the next step store every frame, so callers that alternate two buffers get every step written in full.
 * With a learner view set with RCW_VIEW_ONLY (below) steps do not write it: it holds the last frames rendered until
 * rcw_update_camera_view. */
RCW_API int rcw_obs_device_ptr(rcw_handle* h, void** device_ptr);
/* Copy frames of agents [first, first+count) to host: UInt32 (H_cam, N, count). */
RCW_API int rcw_obs_copy(rcw_handle* h, uint32_t* out_host, int32_t first, int32_t count);
/* env.top_view SR:302 (needs cfg.render_top_view = 1): UInt32 (H*pu, W*pu, B), column-major,
 * as update_top_view! SR:446-483 leaves it: draw_tile_map! SR:342-372 (tile colours
 * 0x00FFFFFF wall / 0x00FF0000 goal / 0x00000000 free SR:288, grid 0x00cccccc), one line per
 * ray to its stop point SR:473-477 (0x00808080) and the player circle SR:480 (0x00c0c0c0).
 * The line and circle rasterisers belong to SimpleDraw 0.3 (un-vendored): Bresenham / midpoint
 * circle are ASSUMED — parity unpinned. */
RCW_API int rcw_top_view_device_ptr(rcw_handle* h, void** device_ptr);
RCW_API int rcw_top_view_copy(rcw_handle* h, uint32_t* out_host, int32_t first, int32_t count);
/* RLBase.reward SR:583 / RLBase.is_terminated SR:584.  rcw_reward serves R = Float32 handles; rcw_reward_typed
 * copies B elements of the handle's R (cfg.reward_type) whatever it is; the device array behind
 * rcw_reward_device_ptr has that element type too. */
RCW_API int rcw_reward(rcw_handle* h, float* out_host /* (B) */);
RCW_API int rcw_reward_typed(rcw_handle* h, void* out_host /* (B) of R */);
RCW_API int rcw_done(rcw_handle* h, uint8_t* out_host /* (B) */);
RCW_API int rcw_reward_device_ptr(rcw_handle* h, void** device_ptr);
RCW_API int rcw_done_device_ptr(rcw_handle* h, void** device_ptr);
/* ---- the episode time limit (this build's addition: the reference has none) ----------------------------------------------
 * SingleRoom ends an episode at the goal only.  rcw_set_time_limit puts the limit almost every RL loop wants around it where `done` is
 * decided, on the device, at no host synchronisation.  State: episode_steps (UInt32 (B)) and truncated (UInt8 (B), 0/1), allocated by
 * rcw_create and zero there; their device pointers are stable for the handle's lifetime.  The ABI is additive: RCW_ABI_VERSION and
 * rcw_config are what they were.
 *   rcw_set_time_limit(h, L)   L = 0: no limit (the default, the reference's behaviour); L > 0: the limit; L < 0:
 *                              RCW_ERR_INVALID_ARGUMENT.  Every call — stream-ordered — zeroes every agent's episode_steps and truncated
 *                              (the limit counts from the call) and makes the one-launch step cast every agent's successors again, as a
 *                              change of the step's form does (they were cast under the old limit).  The step's form, the observation
 *                              and every other state stay as they are.
 *   rcw_time_limit             the current L.
 *   rcw_episode_steps / rcw_truncated                 host copies; they wait for the stream, like rcw_done.
 *   rcw_episode_steps_device_ptr / rcw_truncated_device_ptr   the arrays where they live, rewritten by steps in stream order.
 * While L > 0, rcw_step / rcw_step_device do for each agent, in this order:
 *   1  invalid device action   the agent is not stepped (rcw_step_device): episode_steps and truncated keep their values, and the
 *                              agent is not restarted even if it is done or truncated.
 *   2  restart                 under cfg.auto_reset an agent whose `done` OR `truncated` is set is re-sampled by this call exactly as a
 *                              done agent is: the action is ignored, reset!(world) runs with the handle's seed, the episode counter
 *                              (rcw_episode) goes up by one, reward 0, done false — and episode_steps = 0, truncated = 0.
 *   3  ordinary step           act! as ever.  If it raised (RCW_OOB_ERROR: the agent is left exactly as it was) the two words stay too.
 *                              Otherwise episode_steps += 1 — a blocked move and the step that reaches the goal count —, then
 *                              truncated = (episode_steps >= L && !done): termination wins on the step where both happen.
 *                              Without cfg.auto_reset nothing restarts: the counter keeps counting and the flag is recomputed by every
 *                              step, as the reference's `done` is.
 * So truncated == (episode_steps >= L && !done) after every call while L > 0; episode_steps at the done / truncated step is the
 * episode's length.  rcw_reset and rcw_set_state / rcw_set_state64 zero both words of the agents in their mask and leave the others';
 * rcw_cast_rays, rcw_update_camera_view, rcw_update_top_view, rcw_set_direction_table*, rcw_set_step_form, the learner-view calls and
 * every getter do not touch them.  With L = 0 steps neither read nor write the two arrays (they run the kernels they ran before the
 * limit existed): both stay zero.  What follows without more: the learner view's frame stack refills on a truncation restart (the
 * episode counter moved); a replayed HIP graph of a step counts and truncates like any step (nothing about the limit lives on the
 * host but L, which the kernels read as an argument) — and therefore keeps the L it was CAPTURED with: capture again after
 * rcw_set_time_limit. */
RCW_API int rcw_set_time_limit(rcw_handle* h, int32_t max_episode_steps);
RCW_API int rcw_time_limit(rcw_handle* h, int32_t* out);
RCW_API int rcw_episode_steps(rcw_handle* h, uint32_t* out_host /* (B) */);
RCW_API int rcw_truncated(rcw_handle* h, uint8_t* out_host /* (B) */);
RCW_API int rcw_episode_steps_device_ptr(rcw_handle* h, void** device_ptr);
RCW_API int rcw_truncated_device_ptr(rcw_handle* h, void** device_ptr);
/* ---- wall layouts (this build's addition: the reference builds the wall ring SR:57-60 and nothing else) ------------------------
 * The WALL layer of world.tile_map is per agent, and everything that reads it — cast_ray, is_player_colliding, the top view, the
 * sampler — takes whatever it holds.  rcw_set_walls writes it: corridors, rooms, mazes, a different layout per agent.  The ABI is
 * additive: RCW_ABI_VERSION and rcw_config are what they were.
 *   walls_host          UInt8 (H*W, layouts): tile (i, j), 1-based, of layout m at m*H*W + (i-1) + H*(j-1) — the tile map's own linear
 *                       order; non-zero = WALL.
 *   layout_index_host   Int32 (B): agent a takes layout index[a].  NULL only with layouts == 1 (every agent takes it) or layouts == B
 *                       (agent a takes layout a).
 *   mask_host           as in rcw_reset: the agents the call touches (NULL: all).
 * Validated on the host before anything is queued; a refusal — RCW_ERR_INVALID_ARGUMENT, the message names the layout and the tile —
 * leaves the handle untouched: a NULL walls_host or layouts < 1; a NULL index with another number of layouts; an index outside
 * 0..layouts-1 (of an agent in the mask); a layout whose ring tile (i or j on the border, SR:57-60) is not a wall — the ring is what
 * ends every ray's march —; a layout with fewer than two free interior tiles (a goal and a player must fit).  Layouts are NOT checked
 * for reachability: a goal the agent cannot reach is what the time limit is for.
 * Effect, stream-ordered, for the agents in the mask: the WALL layer becomes the layout and the GOAL layer is cleared; then the agents
 * are reset exactly as rcw_reset(h, mask, <the handle's current seed>) resets them — goal and pose drawn against the new walls, episode
 * counter + 1, reward 0, done false, the time limit's two words zeroed, rays cast, camera view / top view / learner view rendered, the
 * frame stack refilled.  After the call every agent is in a valid post-reset world; a caller who wants a chosen state follows with
 * rcw_set_state, whose host validation (interior tile, inside the room) does NOT know the walls: a goal or a pose it puts into a wall is
 * the caller's.  The walls persist through every later rcw_reset, rcw_set_state and device-side restart (done or truncated under
 * cfg.auto_reset) until the next rcw_set_walls.
 * reset!(world) with walls — the one change of rule, and none on a ring-only map: after the old goal bit is cleared (SR:118) the goal
 * pair is drawn (two draws, SR:120) and drawn AGAIN (two more draws) while the drawn tile's WALL bit is set, at most 1024*H*W redraws
 * (the sampler's own max_tries, utils.jl:23); after that it keeps the last pair and sets RCW_WARN_SAMPLER_GAVE_UP.  Then the player's
 * tile (rejection on any bit, as ever) and the heading.  No interior tile of a ring-only map is a wall: no redraw, the same draw
 * indices, every sequence what it was. */
RCW_API int rcw_set_walls(rcw_handle* h, const uint8_t* walls_host, int32_t layouts,
                          const int32_t* layout_index_host, const uint8_t* mask_host);
/* ---- the goal distance (this build's addition: the reference's only signal is the reward of 1 at the goal) ------------------------
 * Opt-in per handle: the shortest-path distance to the goal through the walls, kept on the device for every agent behind every call
 * that moves an agent, a goal or a wall — what potential-based shaping, SPL and a distance-map target need, at no host
 * synchronisation.  A handle that never enables it runs exactly the kernels it ran before.  The ABI is additive: RCW_ABI_VERSION and
 * rcw_config are what they were.
 * For agent a, with `walls` the WALL layer of its tile map, g its goal tile (rcw_goal) and t the player's tile — wu_to_tu of its
 * position (utils.jl:5): floor(x) + 1, floor(y) + 1, the same in Float64 worlds —:
 *   field            UInt16 (H*W, B), tile (i, j), 1-based, of agent a at a*H*W + (i-1) + H*(j-1) — the tile map's own linear order, the
 *                    one rcw_set_walls takes.  The breadth-first distance in tiles from g, moving between tiles that share an edge and
 *                    whose WALL bit is clear; the GOAL bit plays no part.  field[g] = 0; walls and tiles that cannot be reached hold
 *                    0xFFFF; if g itself is a wall (rcw_set_state put it there, or the sampler gave up) every entry is 0xFFFF.
 *                    rcw_create bounds H*W + 2H <= 65280, so every real distance is below 0xFFFF.
 *   distance         Int32 (B): field[t], or -1 where that is 0xFFFF or t is off the map (the kernel checks and never reads outside
 *                    the field).
 *   start_distance   Int32 (B): distance as of the start of the agent's current episode — SPL is success * l / max(p, l) with l this
 *                    word and p the path taken.
 *   progress         Int32 (B): what the last call brought the agent closer by, in tiles; positive means closer.
 * What each call does to them — stream-ordered on the handle's stream, behind everything the call already queues:
 *   rcw_set_goal_distance(h, 1)   allocates, computes the field of every agent, distance from it, start_distance = distance,
 *                                 progress = 0; on a handle that has it, the same again.  An allocation failure leaves what was there.
 *   rcw_set_goal_distance(h, 0)   frees it (RCW_OK also where there was none).  On a handle with the guide on (rcw_set_guide, which
 *                                 reads the field) it switches the guide off too.
 *   rcw_reset, rcw_set_state, rcw_set_state64, rcw_set_walls
 *                                 for the agents in the call's mask: field recomputed, distance new, start_distance = distance,
 *                                 progress = 0; an agent outside the mask keeps every byte of its field and its three words.
 *                                 rcw_set_state does not move the episode counter: the mask decides here, not the counter.
 *   rcw_step, rcw_step_device     an agent the call restarted (its episode counter, rcw_episode, differs from the one recorded at its
 *                                 last flood: done or truncated under cfg.auto_reset): field recomputed against the new goal, distance
 *                                 new, start_distance = distance, progress = 0.  Every other agent: progress = old - new if both
 *                                 distances are >= 0, else 0; distance = new; start_distance kept.  The rule needs no knowledge of the
 *                                 action: an invalid device action, a raising move under RCW_OOB_ERROR, a turn and a blocked move
 *                                 leave the tile — progress 0.
 *   rcw_cast_rays, rcw_update_camera_view, rcw_update_top_view, rcw_set_direction_table*, rcw_set_step_form, rcw_set_time_limit, the
 *   learner-view calls and every getter   nothing.
 * A replayed HIP graph of a step works like any step: nothing about this alternates on the host, the recorded episode counter lives on the
 * device.  The device pointers are stable until the next rcw_set_goal_distance.  The kernel (one launch, rcw_goal_distance_kernel) runs
 * behind the step's own and OUTSIDE rcw_profile's events: cast_ms + top_view_ms + fill_ms is what it was.
 *   rcw_goal_distance_enabled            0 / 1.
 *   rcw_goal_distance                    host copies of the three words (any pointer may be NULL); waits for the stream as rcw_done does.
 *   rcw_goal_distance_device_ptr         the three arrays where they live (any pointer may be NULL).
 *   rcw_goal_distance_field              the fields of agents [first, first+count) to host memory, H*W UInt16 each (waits for the stream).
 *   rcw_goal_distance_field_device_ptr   the field batch in DEVICE memory.
 * The last four return RCW_ERR_UNSUPPORTED on a handle that has not enabled it. */
RCW_API int rcw_set_goal_distance(rcw_handle* h, int32_t enable);
RCW_API int rcw_goal_distance_enabled(rcw_handle* h, int32_t* out);
RCW_API int rcw_goal_distance(rcw_handle* h, int32_t* distance /* (B) */, int32_t* start_distance /* (B) */, int32_t* progress /* (B) */);
RCW_API int rcw_goal_distance_device_ptr(rcw_handle* h, void** distance, void** start_distance, void** progress);
RCW_API int rcw_goal_distance_field(rcw_handle* h, int32_t first, int32_t count, void* out_host /* UInt16 (H*W, count) */);
RCW_API int rcw_goal_distance_field_device_ptr(rcw_handle* h, void** ptr);
/* ---- the seen map (this build's addition: the tiles each agent's view rays have crossed since its episode began) -----------------------
 * Opt-in per handle: what a coverage / exploration bonus, a "goal in sight" signal and a fog-of-war observation need, kept on the device
 * at no host synchronisation.  A handle that never enables it runs exactly the kernels it ran before.  The ABI is additive:
 * RCW_ABI_VERSION and rcw_config are what they were.
 * For agent a, bits(t) of tile t is what its tile map holds NOW: the WALL bit | the GOAL bit << 1.
 *   map          UInt8 (H*W, B), tile (i, j), 1-based, of agent a at a*H*W + (i-1) + H*(j-1) — the tile map's own linear order, the one
 *                rcw_set_walls and the goal-distance field use.  0 = not seen in the agent's current episode; otherwise 1 + bits(t) as of
 *                the call that first saw it: 1 free, 2 wall, 3 goal; 4 appears only where rcw_set_state put a goal into a wall.
 *   seen_count   Int32 (B): the number of non-zero entries of the agent's map.
 *   newly_seen   Int32 (B): the number of entries the last call turned from 0 to non-zero; 0 after any call that started the agent's
 *                map afresh.
 *   goal_seen    Int32 (B): 1 if map[goal tile] is non-zero, else 0; 0 when the goal is off the map.
 * "Seen" is exactly what the camera saw.  For the agent's current pose a call takes each of the handle's N rays — the rows of the ray
 * table for its heading, as cast_rays! does (SR:195-231) — and marks every tile RayCaster.cast_ray's march visits with the handle's
 * dda_tie_break, from the player's tile (wu_to_tu of its position) through the stop tile, both included; dda_distance plays no part in
 * which tiles are visited.  A player whose tile is off the map, or whose position is NaN, marks nothing; a player standing on an obstacle
 * tile marks that tile alone.  Every map the library accepts has the wall ring, so every ray stops on the map; the kernel nonetheless
 * never reads or writes outside the agent's H*W entries, and what it marks for a ray that left the map is unspecified.  Float64 worlds
 * march in Float64.
 * What each call does — stream-ordered on the handle's stream, behind everything the call already queues:
 *   rcw_set_seen_map(h, 1)        allocates; every agent's map is cleared and marked from its current pose: seen_count is the result,
 *                                 newly_seen = 0, goal_seen is set.  On a handle that has it, the same again.  An allocation failure
 *                                 leaves what was there.
 *   rcw_set_seen_map(h, 0)        frees it (RCW_OK also where there was none).  On a handle with the frontier on (rcw_set_frontier, which
 *                                 floods over the map): RCW_ERR_UNSUPPORTED, and nothing changes — switch the frontier off first.
 *   rcw_reset, rcw_set_state, rcw_set_state64, rcw_set_walls
 *                                 the agents in the call's mask are cleared and marked from the new pose against the new world,
 *                                 newly_seen = 0, and the episode counter is recorded; an agent outside the mask keeps every byte and
 *                                 its three words.  The mask decides, not the episode counter.
 *   rcw_step, rcw_step_device     an agent the call restarted (its episode counter, rcw_episode, differs from the one recorded at its
 *                                 last clear: done or truncated under cfg.auto_reset) is cleared and marked from the new pose,
 *                                 newly_seen = 0, and the counter is recorded.  Every other agent is marked from its pose after the step:
 *                                 newly_seen = the tiles that were 0 before, seen_count += newly_seen, goal_seen may go 0 -> 1 and never
 *                                 back within an episode.  The rule needs no knowledge of the action: an invalid device action, a raising
 *                                 move under RCW_OOB_ERROR and a blocked move leave the pose — newly_seen 0; a turn can see new tiles.
 *   rcw_cast_rays, rcw_update_camera_view, rcw_update_top_view, rcw_set_direction_table*, rcw_set_step_form, rcw_set_time_limit, the
 *   learner-view and goal-distance calls and every getter   nothing.  A new direction table takes effect at the next marking.
 * A replayed HIP graph of a step marks like any step: nothing about this alternates on the host, the recorded episode counter lives on
 * the device.  The device pointers are stable until the next rcw_set_seen_map.  The kernel (one launch, rcw_seen_map_kernel) runs behind
 * the step's own and OUTSIDE rcw_profile's events: cast_ms + top_view_ms + fill_ms is what it was.
 *   rcw_seen_map_enabled            0 / 1.
 *   rcw_seen_words                  host copies of the three words (any pointer may be NULL); waits for the stream as rcw_done does.
 *   rcw_seen_words_device_ptr       the three arrays where they live (any pointer may be NULL).
 *   rcw_seen_map                    the maps of agents [first, first+count) to host memory, H*W UInt8 each (waits for the stream).
 *   rcw_seen_map_device_ptr         the map batch in DEVICE memory.
 * The last four return RCW_ERR_UNSUPPORTED on a handle that has not enabled it. */
RCW_API int rcw_set_seen_map(rcw_handle* h, int32_t enable);
RCW_API int rcw_seen_map_enabled(rcw_handle* h, int32_t* out);
RCW_API int rcw_seen_words(rcw_handle* h, int32_t* seen_count /* (B) */, int32_t* newly_seen /* (B) */, int32_t* goal_seen /* (B) */);
RCW_API int rcw_seen_words_device_ptr(rcw_handle* h, void** seen_count, void** newly_seen, void** goal_seen);
RCW_API int rcw_seen_map(rcw_handle* h, int32_t first, int32_t count, void* out_host /* UInt8 (H*W, count) */);
RCW_API int rcw_seen_map_device_ptr(rcw_handle* h, void** ptr);
/* ---- the local map (this build's addition: an agent-centred, heading-up crop of the map) ---------------------------------------------
 * Opt-in per handle: the "egocentric map" input of a mapping-based navigation agent, computed on the device from the engine's own
 * position, heading, direction table and tiles, at no host synchronisation.  A handle that never enables it runs exactly the kernels it
 * ran before.  The ABI is additive: RCW_ABI_VERSION and rcw_config are what they were.
 * Per agent one UInt8 (S, S) image, row-major: cell (row q, column c) of agent a at a*S*S + q*S + c; the batch is (B, S, S), the agent
 * stride S*S bytes, unpadded.  size S in 1..RCW_LOCAL_MAX_SIZE, cells_per_tile r in 1..RCW_LOCAL_MAX_CELLS_PER_TILE (a cell is 1/r of a
 * tile wide), and the source:
 *   RCW_LOCAL_WORLD   the agent's tile map as it is NOW;
 *   RCW_LOCAL_SEEN    its seen map; the handle must have enabled the seen map first, else RCW_ERR_UNSUPPORTED.
 * A cell holds the seen map's alphabet, for both sources: 0 = outside the map (RCW_LOCAL_SEEN: or not seen), otherwise 1 + bits(t):
 * 1 free, 2 wall, 3 goal, 4 a goal in a wall.
 * The geometry is exact, in the handle's world-unit type T, every operation rounded once:
 *   off[k] = (T)(2k + 1 - S) / (T)(2r), k = 0..S-1   the cell centres' offsets from the agent, in tiles;
 *   (px, py) the agent's position, (d1, d2) entry player_direction_au of the direction table the handle holds — whatever
 *   rcw_set_direction_table or its 64 twin last put there, unit or not; the lateral axis is rotate_minus_90 of it, (d2, -d1), as in the
 *   ray table (SR:193);
 *   cell (q, c): ahead = off[S-1-q] — row 0 is the farthest ahead —, lateral = off[S-1-c] — column 0 is on the +lateral side, the side
 *   of ray 0 = dir + fov * lateral axis (which fills the camera view's LAST image column: SR:431 mirrors) —,
 *       wx = (px + ahead*d1) + lateral*d2        wy = (py + ahead*d2) - lateral*d1          (in exactly this association)
 *   fx = floor(wx), fy = floor(wy), compared in T: if 0 <= fx < H and 0 <= fy < W the cell shows tile t = (int)fx + H*(int)fy, that is
 *   tile (i, j) = (fx+1, fy+1) in the order rcw_set_walls and the seen map use: RCW_LOCAL_WORLD 1 + its two bits, RCW_LOCAL_SEEN map[t].
 *   Otherwise, and for any NaN, 0.  Nothing outside the agent's H*W entries is read for any position, NaN, +-Inf and far off the map
 *   included.
 * What each call does — stream-ordered on the handle's stream, behind everything the call already queues (the seen map's launch too):
 *   rcw_set_local_map(h, source, size, cells_per_tile)
 *                                 source = 0 frees it (RCW_OK also where there was none).  Otherwise allocates and computes every agent's
 *                                 image at once; on a handle that has one, the new parameters replace the old (and the device pointer).  A
 *                                 bad value: RCW_ERR_INVALID_ARGUMENT, the handle as it was.  An allocation failure leaves what was there.
 *   rcw_step, rcw_step_device, rcw_reset, rcw_set_state, rcw_set_state64, rcw_set_walls, rcw_set_direction_table, rcw_set_direction_table64,
 *   rcw_set_seen_map(h, 1)        every agent's image is computed again from the state behind the call.  The function is stateless: an agent
 *                                 outside a mask gets the same bytes again; there is no mask and no episode logic.
 *   rcw_set_seen_map(h, 0)        while the source is RCW_LOCAL_SEEN: RCW_ERR_UNSUPPORTED (switch the local map off first), nothing changes.
 *   every other call              nothing.
 * A replayed HIP graph of a step computes the images like any step.  The device pointer is stable until the next rcw_set_local_map.  The
 * kernel (one launch, rcw_local_map_kernel) runs last and OUTSIDE rcw_profile's events.
 *   rcw_local_map_info            the three parameters (any pointer may be NULL); zeros while it is off.
 *   rcw_local_map_device_ptr      the image batch in DEVICE memory.
 *   rcw_local_map_copy            the images of agents [first, first+count) to host memory, S*S bytes each (waits for the stream).
 * The last two return RCW_ERR_UNSUPPORTED on a handle that has not enabled it. */
#define RCW_LOCAL_WORLD 1
#define RCW_LOCAL_SEEN 2
#define RCW_LOCAL_MAX_SIZE 128
#define RCW_LOCAL_MAX_CELLS_PER_TILE 16
RCW_API int rcw_set_local_map(rcw_handle* h, int32_t source, int32_t size, int32_t cells_per_tile);
RCW_API int rcw_local_map_info(rcw_handle* h, int32_t* source, int32_t* size, int32_t* cells_per_tile);
RCW_API int rcw_local_map_device_ptr(rcw_handle* h, void** device_ptr);
RCW_API int rcw_local_map_copy(rcw_handle* h, uint8_t* out_host /* (S*S, count) */, int32_t first, int32_t count);
/* ---- the wall bank (this build's addition: a wall layout drawn on the device at every start of an episode) ---------------------------
 * Opt-in per handle.  rcw_set_walls gives an agent one layout, which then stays through every later reset and device-side restart: under
 * cfg.auto_reset the agent replays one maze for the whole run.  A handle with a bank holds L layouts on the device, each checked as
 * rcw_set_walls checks one (ring present, at least two free interior tiles), and UInt32 weights w[0..L-1] (NULL: all 1) whose sum lies in
 * 1 .. 2^32 - 1; cum[k] = w[0] + ... + w[k].  An agent BEGINS AN EPISODE whenever its episode counter moves: rcw_reset, a done or
 * truncated restart under cfg.auto_reset, and the call that installs the bank.  With g = agent_id_offset + a the agent's global id and e
 * its counter before the increment:
 *   key = the episode key of (seed, g, e)             csrc/rcw_rng.h: the key the reset of that episode already uses
 *   u   = draw number 2^63 of that key                (the reset's own draw indices count from 0 and stay below 4 + 3*1024*H*W)
 *   k   = the smallest index with cum[k] > floor(u * cum[L-1] / 2^64)
 *   WALL layer := layout k, GOAL layer cleared, wall_layout[a] := k; then reset!(world) exactly as under "wall layouts" above against the
 *   new walls — the same key, draw indices from 0 —: goal (redrawn while on a wall), player tile, heading, reward 0, done false, the
 *   time limit's two words zeroed; counter = e + 1 (once).
 * The result is a pure function of (seed, global id, episode, bank): not of the sharding, the step form, or the walls the agent had.  A
 * layout of weight 0 is never drawn.  Every draw index a handle without a bank uses is untouched: such a handle draws what it drew before
 * and launches exactly the kernels it launched before.  The ABI is additive: RCW_ABI_VERSION and rcw_config are what they were.
 * What each call does — stream-ordered on the handle's stream:
 *   rcw_set_wall_bank             walls_host UInt8 (H*W, L) in rcw_set_walls' order (non-zero = wall), L = layouts, weights_host UInt32 (L)
 *                                 or NULL.  Validated on the host before anything is queued: a refusal (RCW_ERR_INVALID_ARGUMENT: a bad
 *                                 layout — the message names the layout and the tile —, layouts < 0, weights whose sum is 0 or above
 *                                 2^32 - 1) leaves the handle untouched, an allocation failure leaves what was there.  Installs the bank
 *                                 (replacing one that was there) and restarts EVERY agent under the rule with the handle's current seed, as
 *                                 rcw_reset(h, NULL, seed) would: the counters go up by one, everything is rendered, the features refilled.
 *                                 layouts == 0 or walls_host == NULL switches the bank off (RCW_OK also where there was none): the agents
 *                                 keep the walls they have, and the handle is an ordinary walled handle again.
 *   rcw_set_wall_bank_weights     new weights for the installed bank (NULL: all 1), stream-ordered WITHOUT waiting for the stream: they
 *                                 hold from each agent's next episode start, no agent is touched — the call a prioritised-replay caller
 *                                 makes every few updates.  A sum of 0 or above 2^32 - 1: RCW_ERR_INVALID_ARGUMENT, the old weights stay.
 *   rcw_reset                     the agents of the mask begin an episode: a layout each, by the rule, with the seed the call gives.
 *   rcw_step, rcw_step_device     an agent the step restarted (done or truncated under cfg.auto_reset) takes a layout by the rule: the
 *                                 reset the step made against the old walls is discarded without a trace, the agent's rays are cast and
 *                                 its views rendered again, and goal distance, seen map, local map, learner view and frame stack follow
 *                                 the new maze.  No host synchronisation; a replayed HIP graph of a step draws layouts like any step.
 *   rcw_set_state, rcw_set_state64   do not move the counter: the layout stays.
 *   rcw_set_walls                 RCW_ERR_UNSUPPORTED while the handle has a bank, nothing changes: switch the bank off first.
 *   rcw_set_direction_table*, rcw_set_time_limit, rcw_set_step_form, the feature switches, the getters   nothing.
 * The bank's kernel (one launch, rcw_wall_bank_kernel) and the re-render of the agents it restarted (the masked cast, then their camera
 * view by rcw_wall_bank_paint_kernel — or, with a top view, the masked fill) run behind the step's own launches and
 * OUTSIDE rcw_profile's events (with RCW_VIEW_ONLY: in front of the view kernel, inside cast_ms).  Of the bank the host keeps its sizes only.
 *   rcw_wall_bank_info            L and the weights' sum (either pointer may be NULL); zeros while the bank is off.
 *   rcw_wall_layout               host copy of each agent's current layout index, Int32 (B); waits for the stream as rcw_done does.
 *   rcw_wall_layout_device_ptr    the same array in DEVICE memory, stable until the next rcw_set_wall_bank.
 * rcw_set_wall_bank_weights returns RCW_ERR_UNSUPPORTED on a handle without a bank, the two getters on a handle with neither a bank nor
 * a wall generator (below).  rcw_set_wall_bank is refused (RCW_ERR_UNSUPPORTED) while the handle has a wall generator. */
RCW_API int rcw_set_wall_bank(rcw_handle* h, const uint8_t* walls_host /* (H*W, L) */, int32_t layouts, const uint32_t* weights_host /* (L) or NULL */);
RCW_API int rcw_set_wall_bank_weights(rcw_handle* h, const uint32_t* weights_host /* (L) or NULL */);
RCW_API int rcw_wall_bank_info(rcw_handle* h, int32_t* layouts, uint64_t* total_weight);
RCW_API int rcw_wall_layout(rcw_handle* h, int32_t* out_host /* (B) */);
RCW_API int rcw_wall_layout_device_ptr(rcw_handle* h, void** device_ptr);
/* ---- the wall generator (this build's addition: a new maze made on the device at every start of an episode) ---------------------------
 * Opt-in per handle.  The bank above draws from a finite set the host built; a handle with a generator makes the layout itself, in the
 * kernel that gives it out, from one 64-bit key — a fresh maze every episode, or a seeded range of levels to train or evaluate on.
 * A MAZE FROM ONE KEY  maze(m, H, W, loops), H, W >= 5, with draw(m, n) the counter-based draw number n of key m (csrc/rcw_rng.h):
 *   cells   the tiles with odd 0-based (i, j) inside the ring: ni = (H-1)/2, nj = (W-1)/2 (integer division), C = ni nj, cell c = ci nj + cj
 *           on tile (2ci+1, 2cj+1).  With an even H or W the last interior row or column stays wall.
 *   edges   the east edge of cell c has id 2c, exists where cj+1 < nj, and its passage tile is (2ci+1, 2cj+2); the south edge has id 2c+1,
 *           exists where ci+1 < ni, passage tile (2ci+2, 2cj+1).
 *   order   every edge has the order word w(id) = (draw(m, id) & 0xFFFFFFFFFFF00000) | id.  Ids stay below 2^20: the words are distinct.
 *   tree    the minimum spanning tree of the cell grid under w.  It is unique, so it does not depend on the algorithm that finds it
 *           (the device runs Boruvka rounds in LDS, rcw_wall_generator_layout below sorts the edges and runs Kruskal).
 *   loops   a non-tree edge is opened too where (draw(m, 2C + id) >> 32) < loops; loops is UInt32, 0 gives a perfect maze.
 *   Every tile is WALL except the cells and the passage tiles of tree edges and opened edges.  The layout is connected and ring-closed by
 *   construction and has at least 7 free interior tiles: always valid as rcw_set_walls wants one.
 * THE KEY OF AN EPISODE  With g = agent_id_offset + a the agent's global id and e its episode counter before the increment:
 *   key = the episode key of (seed, g, e), u = draw number 2^63 of that key (the bank's draw index: generator and bank exclude each other).
 *   levels == 0   m = u, wall_layout[a] = -1: every episode gets a maze of its own.
 *   levels >= 1   l = first_level + floor(u * levels / 2^64), m = the episode key of (level_seed, l, 0), wall_layout[a] = l: the maze is a
 *                 function of (level_seed, l, H, W, loops) alone.  Requires first_level >= 0 and first_level + levels <= 2^31 - 1.
 * After that the rule is exactly the bank's: the WALL layer becomes the maze, the GOAL layer is cleared, reset!(world) runs against the new
 * walls under `key` from draw 0, the time limit's words are zeroed, the counter ends at e + 1 (once).  The result is a pure function of
 * (seed, g, e, parameters): not of the sharding, the step form, or the walls the agent had.  A handle without a generator draws and
 * launches exactly what it did before.  The ABI is additive: RCW_ABI_VERSION and rcw_config are what they were.
 *   rcw_set_wall_generator        enable != 0: installs the generator and restarts EVERY agent under the rule with the handle's current seed,
 *                                 as rcw_set_wall_bank does (counters + 1, everything rendered, the features refilled).  Validated on the
 *                                 host before anything is queued, a refusal leaves the handle untouched: RCW_ERR_INVALID_ARGUMENT for H or
 *                                 W below 5 or a bad level range; RCW_ERR_UNSUPPORTED for C > 4096 (maps beyond 129 x 129: the message names
 *                                 the bound) and while a bank is on — rcw_set_wall_bank is likewise refused while the generator is on:
 *                                 switch one off first.  enable == 0 switches it off (RCW_OK also where there was none): the walls stay.
 *                                 The parameters are kernel arguments fixed at install: a captured step replays correctly.
 *   rcw_reset, rcw_step, rcw_step_device, rcw_set_state*, the feature switches   as with a bank: an agent that begins an episode takes a
 *                                 maze by the rule, goal distance, seen map, local map, learner view and frame stack follow it;
 *                                 rcw_set_state* keeps the maze.  rcw_set_walls: RCW_ERR_UNSUPPORTED while the generator is on.
 *   rcw_wall_generator_info       the parameters (any pointer may be NULL); zeros while the generator is off.
 *   rcw_wall_layout, rcw_wall_layout_device_ptr   also serve a handle with a generator: l, or -1.
 *   rcw_wall_generator_key        handle-less, pure host arithmetic: the maze key m and the level (-1 with levels == 0) of episode `episode`
 *                                 (the counter before the increment) of global agent `global_agent` under `seed`.
 *   rcw_wall_generator_layout     handle-less, pure host arithmetic: maze(maze_key, H, W, loops) as UInt8 (H*W) in rcw_set_walls' order
 *                                 (1 = wall) — what the agent's WALL layer holds; the replay and evaluation tool of a caller.
 *                                 RCW_ERR_INVALID_ARGUMENT for H or W below 5, or edge ids of 2^20 and more. */
RCW_API int rcw_set_wall_generator(rcw_handle* h, int32_t enable, uint32_t loops, int32_t levels, int32_t first_level, uint64_t level_seed);
RCW_API int rcw_wall_generator_info(rcw_handle* h, int32_t* enabled, uint32_t* loops, int32_t* levels, int32_t* first_level, uint64_t* level_seed);
RCW_API int rcw_wall_generator_key(uint64_t seed, int32_t global_agent, uint32_t episode, int32_t levels, int32_t first_level, uint64_t level_seed,
                                   uint64_t* maze_key, int32_t* level);
RCW_API int rcw_wall_generator_layout(int32_t H, int32_t W, uint64_t maze_key, uint32_t loops, uint8_t* out_host /* (H*W), rcw_set_walls' order */);
/* ---- the wall generator: caves (this build's addition: a second family of layouts behind the generator's launch point) -------------------
 * Opt-in per handle.  The generator above makes one kind of world: one-tile corridors on the odd sub-grid.  Caves are open space with
 * irregular walls and pockets: a seeded random fill, smoothed by a cellular automaton, pruned to one connected region.
 * A CAVE FROM ONE KEY  cave(m, H, W, fill, smooth), H, W >= 5, with draw(m, n) of csrc/rcw_rng.h; tiles are 0-based (i, j) with index
 * t = i + H j, the tile map's own order.  The rule does not depend on the algorithm (the device propagates labels in LDS,
 * rcw_wall_caves_layout below flood-fills with a queue).
 *   ring     every tile with i in {0, H-1} or j in {0, W-1} is WALL, at every stage.
 *   gen 0    an interior tile t is WALL where (draw(m, 2^62 + t) >> 32) < fill.  fill is UInt32 as loops is: 0 gives an empty room,
 *            2^32 - 1 all wall.  Indices from 2^62 cannot meet the maze's, which stay below 2^21: the fallback uses the same m.
 *   smooth   `smooth` times, 0 <= smooth <= 8, synchronously (every interior tile reads generation g and writes g + 1): a tile is WALL in
 *            g + 1 where at least 5 of the 9 tiles of its 3 x 3 neighbourhood, itself included, are WALL in g; the ring counts as WALL.
 *   regions  the 4-connected components of free tiles.  The one with the most tiles is kept; of several largest, the one that holds the
 *            smallest tile index t.  Every other free tile becomes WALL.
 *   fallback need = max(7, ((H-2)(W-2)) / 4) (integer division).  Where the kept region has fewer than `need` tiles, or there is none,
 *            the layout is maze(m, H, W, 0) instead, exactly as the generator's rule defines it.
 *   So a layout is always connected and ring-closed with at least 7 free interior tiles: valid as rcw_set_walls wants one.  Small maps
 *   mostly fall back: at fill 0.40, smooth 2 nearly every 5 x 7 level is a maze, about a quarter of the 8 x 8 ones, none at 32 x 32.
 * THE KEY OF AN EPISODE is the generator's, unchanged (key, u, levels == 0: m = u and wall_layout -1; levels >= 1: l, m = the episode key of
 * (level_seed, l, 0), wall_layout l): rcw_wall_generator_key serves both families.  After that the rule is the bank's, word for word.
 * The ABI is additive: RCW_ABI_VERSION, rcw_config and every existing export are what they were; a handle without caves launches what
 * it launched.
 *   rcw_set_wall_caves            enable != 0: installs the caves and restarts EVERY agent under the rule with the handle's current seed, as
 *                                 rcw_set_wall_generator does.  Validated on the host before anything is queued, a refusal leaves the
 *                                 handle untouched: RCW_ERR_INVALID_ARGUMENT for H or W below 5, smooth outside 0 .. 8 or a bad level
 *                                 range; RCW_ERR_UNSUPPORTED for more than 4096 interior tiles ((H-2)(W-2): maps beyond 66 x 66; the message
 *                                 names the bound) and while a bank or the maze generator is on.  enable == 0 switches them off (RCW_OK
 *                                 also where there were none): the walls stay.  The parameters are kernel arguments fixed at install: a
 *                                 captured step replays correctly.
 *   while caves are on            rcw_set_wall_bank, rcw_set_wall_generator(enable != 0) and rcw_set_walls: RCW_ERR_UNSUPPORTED, nothing
 *                                 changes (rcw_set_wall_generator(h, 0, ...) is RCW_OK and changes nothing either).  rcw_set_state* keeps
 *                                 the layout.  rcw_wall_layout* serve l, or -1.  rcw_wall_generator_info reports enabled = 1, loops = 0
 *                                 and the level parameters.
 *   rcw_wall_caves_info           enabled, fill, smooth (any pointer may be NULL); zeros while caves are off.
 *   rcw_wall_caves_layout         handle-less, pure host arithmetic: cave(key, H, W, fill, smooth) as UInt8 (H*W) in rcw_set_walls' order
 *                                 (1 = wall); *fell_back (may be NULL) = 1 where the layout is the maze.  The refusals of a geometry
 *                                 and of smooth are rcw_set_wall_caves'. */
RCW_API int rcw_set_wall_caves(rcw_handle* h, int32_t enable, uint32_t fill, int32_t smooth, int32_t levels, int32_t first_level, uint64_t level_seed);
RCW_API int rcw_wall_caves_info(rcw_handle* h, int32_t* enabled, uint32_t* fill, int32_t* smooth);
RCW_API int rcw_wall_caves_layout(int32_t H, int32_t W, uint64_t key, uint32_t fill, int32_t smooth, uint8_t* out_host /* (H*W), rcw_set_walls' order */,
                                  int32_t* fell_back);
/* ---- the wall generator: rooms (this build's addition: a third family of layouts behind the generator's launch point) --------------------
 * Opt-in per handle.  Rectangular rooms of different sizes joined by doorways, layouts.four_rooms' topology made anew every episode: the
 * interior is split recursively by walls with one or two doors.  No fallback and no prune: connected by construction from 5 x 5.
 * ROOMS FROM ONE KEY  rooms(m, H, W, room, stop, doors), H, W >= 5, with draw(m, n) and below(u, r) of csrc/rcw_rng.h; tiles are 0-based
 * (i, j) with index t = i + H j.  room is Int32 >= 1 (a room's least side); stop and doors are UInt32 probability words as loops and fill
 * are.  The ring is WALL, the interior starts free.  A CHAMBER is a rectangle of interior tiles [i0..i1] x [j0..j1], bounds inclusive; the
 * root is [1..H-2] x [1..W-2]; i0 and j0 are always odd.  A chamber's draws have the indices n + k, n = 2^61 + 8 ((t0 << 16) | t1) with
 * t0 = i0 + H j0, t1 = i1 + H j1 (so H W <= 65536): distinct rectangles, distinct indices, all in [2^61, 2^61 + 2^35) — away from the
 * maze's (below 2^21), the caves' (from 2^62), the layout draw (2^63) and reset_agent's (from 0).  One chamber:
 *   walls    row walls R = { even i : i0 + room <= i <= i1 - room }, empty unless j1 > j0; column walls C = { even j : j0 + room <= j <=
 *            j1 - room }, empty unless i1 > i0.  Both empty: the chamber is a room.
 *   stop     a chamber other than the root is left whole, a room, where (draw(m, n + 1) >> 32) < stop.
 *   side     only one of R, C non-empty: that one.  Both: cut across the longer side — a row wall where i1 - i0 > j1 - j0, a column wall
 *            where it is shorter, on a tie a row wall where bit 63 of draw(m, n) is set.
 *   line     s = the below(draw(m, n + 2), |S|)-th element of the chosen set S, ascending.
 *   doors    the wall covers the chamber's whole span on line s: positions lo .. hi (j0 .. j1 for a row wall, i0 .. i1 for a column wall).
 *            Door candidates are lo, lo + 2, ... (odd): cnt = (hi - lo) / 2 + 1 of them.  The first door is at lo + 2 below(draw(m, n + 3),
 *            cnt); where (draw(m, n + 4) >> 32) < doors a second one at lo + 2 below(draw(m, n + 5), cnt), which may coincide with the
 *            first.  Every other tile of the span on line s becomes WALL.
 *   children the rectangles on either side of line s.
 *   Walls lie on even lines and doors on odd positions, so a later perpendicular wall ends on an even position: it never blocks a door and
 *   never overlaps an earlier wall.  The layout is connected and ring-closed, has at least 7 free interior tiles, every room side is at
 *   least `room`, and it does not depend on the order the chambers are taken in (the device cuts every chamber of a depth in one round,
 *   rcw_wall_rooms_layout below walks depth first off a stack).  Every room holds an (odd, odd) tile: at most
 *   Q = ceil((H - 2) / 2) ceil((W - 2) / 2) rooms.
 * THE KEY OF AN EPISODE is the generator's, unchanged: rcw_wall_generator_key serves this family too (levels, first_level, level_seed,
 * wall_layout).  After the layout the rule is the bank's, word for word.  The ABI is additive: RCW_ABI_VERSION, rcw_config and every
 * existing export are what they were; a handle without rooms launches what it launched.
 *   rcw_set_wall_rooms            enable != 0: installs the rooms and restarts EVERY agent under the rule with the handle's current seed, as
 *                                 rcw_set_wall_generator does.  Validated on the host before anything is queued, a refusal leaves the
 *                                 handle untouched: RCW_ERR_INVALID_ARGUMENT for H or W below 5, room < 1 or a bad level range;
 *                                 RCW_ERR_UNSUPPORTED for Q > 4096 (130 x 130 and 5 x 4097 are the largest; the message names the bound)
 *                                 or H W > 65536, and while a bank, the maze generator or caves are on.  enable == 0 switches them off
 *                                 (RCW_OK also where there were none): the walls stay.  The parameters are kernel arguments fixed at
 *                                 install: a captured step replays correctly.
 *   while rooms are on            rcw_set_wall_bank, rcw_set_walls, rcw_set_wall_generator(enable != 0) and rcw_set_wall_caves(enable != 0):
 *                                 RCW_ERR_UNSUPPORTED, nothing changes (their enable == 0 forms are RCW_OK and change nothing either).
 *                                 rcw_set_state* keeps the layout.  rcw_wall_layout* serve l, or -1.  rcw_wall_generator_info reports
 *                                 enabled = 1, loops = 0 and the level parameters.
 *   rcw_wall_rooms_info           enabled, room, stop, doors (any pointer may be NULL); zeros while rooms are off.
 *   rcw_wall_rooms_layout         handle-less, pure host arithmetic: rooms(key, H, W, room, stop, doors) as UInt8 (H*W) in rcw_set_walls'
 *                                 order (1 = wall); *rooms (may be NULL) = the number of rooms.  The refusals of a geometry and of room
 *                                 are rcw_set_wall_rooms'. */
RCW_API int rcw_set_wall_rooms(rcw_handle* h, int32_t enable, int32_t room, uint32_t stop, uint32_t doors, int32_t levels, int32_t first_level,
                               uint64_t level_seed);
RCW_API int rcw_wall_rooms_info(rcw_handle* h, int32_t* enabled, int32_t* room, uint32_t* stop, uint32_t* doors);
RCW_API int rcw_wall_rooms_layout(int32_t H, int32_t W, uint64_t key, int32_t room, uint32_t stop, uint32_t doors, uint8_t* out_host /* (H*W), rcw_set_walls' order */,
                                  int32_t* rooms);
/* ---- episode statistics (this build's addition: how the episodes ended, per agent and per level, kept on the device) ------------------
 * Opt-in per handle: what a "record episode statistics" wrapper keeps — length, outcome, level and SPL of every finished episode, and
 * their sums over the batch and per level, which prioritised level replay (rcw_set_wall_bank_weights) and a train / test split of the
 * generators' levels are computed from — at no host synchronisation.  A handle that never enables it runs exactly the kernels it ran
 * before.  The ABI is additive: RCW_ABI_VERSION and rcw_config are what they were.  Every stored quantity is an integer: the table does
 * not depend on the order in which agents are added to it.
 * Per-agent words, device arrays of B entries each:
 *   finished   UInt8    1 iff the LAST call closed this agent's record
 *   outcome    UInt8    RCW_EPISODE_OPEN 0, RCW_EPISODE_SUCCESS 1 (done), RCW_EPISODE_TRUNCATED 2
 *   length     UInt32   step calls the record has lived through (below)
 *   moves      UInt32   those calls after which the agent's position differed
 *   level      Int32    as of the close: rcw_wall_layout's word of the agent on a handle with a layout source, else -1; -1 while open
 *   spl_q16    Int32    as of the close (below); -1 while open or where SPL is undefined
 *   episodes   UInt32   records this agent has closed since the statistics were enabled
 * and, private, the episode counter as of the record's beginning and the position behind the previous call.
 * BEGIN(a): length = moves = 0, outcome = 0, finished = 0, level = -1, spl_q16 = -1, the private position = the agent's position, the
 * private counter = rcw_episode's; episodes stays.
 * Behind rcw_step / rcw_step_device, for every agent, the first of these that applies:
 *   1  restart   the episode counter differs from the private one (a done or truncated restart under cfg.auto_reset): BEGIN.  The
 *                restarting call does not count into length: a record is never closed by the call that began it.
 *   2  frozen    outcome != 0: finished = 0, the private position follows the agent, nothing else.  The words keep the finished episode
 *                until the agent begins another; without cfg.auto_reset a finished agent walks on and is not recorded again until a
 *                reset.
 *   3  open      length += 1; moves += 1 where either value of the position differs from the private one AS A BIT PATTERN; the private
 *                position follows; then, where done | truncated, the record CLOSES, and otherwise finished = 0.
 * A close: outcome = done ? 1 : 2, level as above, episodes += 1, finished = 1, the SPL word, the adds into the table.
 * The rule needs no knowledge of the action: an invalid device action or a raising move under RCW_OOB_ERROR counts into length and not
 * into moves.  So on a handle with a time limit length == episode_steps at the close for every agent that did not fault (a faulting call
 * leaves episode_steps as it was and still counts here).
 * SPL word: defined iff the goal distance is enabled at the close and l = start_distance[a] >= 1.  Truncated and defined: 0.  Success
 * and defined, with INC = position_increment_wu widened to double (position_increment_wu_f64 on a Float64 handle), every operation in
 * IEEE Float64 and in this order: p = (double)moves * INC; q = floor((65536.0 * (double)l) / fmax(p, (double)l)) — SPL = l / max(p, l) in
 * 16.16 fixed point, 65536 where the path was no longer than the tile distance.  Enabling the goal distance in the middle of an episode
 * makes l the distance at that moment: the order of enabling is the caller's.
 * The table: UInt64 (RCW_EPISODE_STATS_ROW_WORDS, 1 + rows), row r at 8 r.  Columns: 0 episodes, 1 successes, 2 truncations, 3 sum_length,
 * 4 sum_moves, 5 spl_episodes (closes with SPL defined), 6 sum_spl_q16, 7 reserved (0).  Row 0 takes every close of the batch, row 1 + k
 * the closes with k = level - first and 0 <= k < rows.  first and rows are fixed when the statistics are enabled, from the live layout
 * source: a wall bank of L layouts: first 0, rows L; a generator family with levels > 0: first first_level, rows levels; no source, or
 * levels == 0: rows 0.  A count above RCW_EPISODE_STATS_MAX_ROWS gives rows 0, not an error: row 0 always works.
 * What each call does — stream-ordered on the handle's stream, behind everything the call already queues:
 *   rcw_set_episode_stats(h, 1)   allocates, zeroes the table and `episodes`, BEGIN for every agent; on a handle that has it, the same
 *                                 again.  An allocation failure leaves what was there.
 *   rcw_set_episode_stats(h, 0)   frees it (RCW_OK also where there was none).
 *   rcw_reset, rcw_set_state, rcw_set_state64, rcw_set_walls
 *                                 BEGIN for the agents in the call's mask — the mask decides, not the counter; an open record that is
 *                                 abandoned is dropped, not counted — and finished = 0 for every agent (no call but a step closes
 *                                 anything).  Nothing else of an agent outside the mask changes.
 *   rcw_set_wall_bank, rcw_set_wall_generator, rcw_set_wall_caves, rcw_set_wall_rooms (install, replace or remove)
 *                                 RCW_ERR_UNSUPPORTED while the statistics are on, nothing changes: the row count would change under
 *                                 the table.  Switch the statistics off first (as rcw_set_seen_map(h, 0) under a seen-source local map).
 *   rcw_episode_stats_clear       zeroes the table WITHOUT waiting for the stream and touches no per-agent word: what a replay loop
 *                                 calls after it has read the table.
 *   rcw_set_wall_bank_weights, rcw_set_time_limit, rcw_set_step_form, the direction-table, learner-view, goal-distance, seen-map and
 *   local-map calls, the renderers and every getter   nothing.
 * A replayed HIP graph of a step records like any step: everything about this lives on the device.  Capture again after enabling or
 * disabling, as with the other features.  The kernel (one launch, rcw_episode_stats_kernel) runs behind the goal distance's and OUTSIDE
 * rcw_profile's events.
 *   rcw_episode_stats_info               enabled, rows, first (any pointer may be NULL); zeros while off.
 *   rcw_episode_stats                    host copies of the seven words (any pointer may be NULL); waits for the stream as rcw_done does.
 *   rcw_episode_stats_device_ptr         the seven arrays where they live (any pointer may be NULL), stable until the next
 *                                        rcw_set_episode_stats.
 *   rcw_episode_stats_table              the table to host memory, 8 (1 + rows) UInt64 (waits for the stream).
 *   rcw_episode_stats_table_device_ptr   the table in DEVICE memory.
 * The last four and rcw_episode_stats_clear return RCW_ERR_UNSUPPORTED on a handle that has not enabled it. */
#define RCW_EPISODE_OPEN 0
#define RCW_EPISODE_SUCCESS 1
#define RCW_EPISODE_TRUNCATED 2
#define RCW_EPISODE_STATS_ROW_WORDS 8
#define RCW_EPISODE_STATS_MAX_ROWS 65536
RCW_API int rcw_set_episode_stats(rcw_handle* h, int32_t enable);
RCW_API int rcw_episode_stats_info(rcw_handle* h, int32_t* enabled, int32_t* rows, int32_t* first);
RCW_API int rcw_episode_stats(rcw_handle* h, uint8_t* finished /* (B) */, uint8_t* outcome /* (B) */, uint32_t* length /* (B) */, uint32_t* moves /* (B) */,
                              int32_t* level /* (B) */, int32_t* spl_q16 /* (B) */, uint32_t* episodes /* (B) */);
RCW_API int rcw_episode_stats_device_ptr(rcw_handle* h, void** finished, void** outcome, void** length, void** moves, void** level, void** spl_q16,
                                         void** episodes);
RCW_API int rcw_episode_stats_table(rcw_handle* h, uint64_t* out_host /* (8, 1 + rows) */);
RCW_API int rcw_episode_stats_table_device_ptr(rcw_handle* h, void** ptr);
RCW_API int rcw_episode_stats_clear(rcw_handle* h);
/* ---- the guide (this build's addition: each agent's shortest-path action, kept on the device) ------------------------------------------
 * Opt-in per handle, on a handle that has the goal distance on: the action that follows the agent's shortest path to its goal, written
 * behind every call that moves an agent, a goal or a wall — the label imitation learning and DAgger need on the states the learner
 * visits, an upper-bound baseline for the SPL table, a way to walk to a state worth saving — at no host synchronisation.  The action
 * array can be handed to rcw_step_device as it stands, or mixed with a policy's on the device.  A handle that never enables it runs
 * exactly the kernels it ran before.  The ABI is additive: RCW_ABI_VERSION and rcw_config are what they were.
 * Per-agent words, device arrays of B entries each:
 *   action     UInt8    always in 1..4
 *   heading    Int32    the 0-based direction index the guide wants the agent to face, -1 where it has no advice
 * THE RULE.  T is the handle's world-unit type; every operation is done in T and rounded once, no fused multiply-add.  For agent a:
 * (x, y) its position, d its 0-based heading (rcw_direction), D[k] = (D1, D2) the handle's direction table as it stands (nd entries),
 * inc = position_increment_wu, F the agent's goal-distance field, 0-based tile (i, j) at i + H*j.
 *   1  i = floor(x), j = floor(y).  Where x or y is not finite, or (i, j) is off the map, or f = F[i, j] is 0xFFFF or 0 — no path, or
 *      the agent stands on the goal tile —: heading = -1, action = 3 (a turn on the spot).  F is read only behind the bounds check.
 *   2  n = the first of (i-1, j), (i+1, j), (i, j-1), (i, j+1) that lies on the map and has F[n] == f - 1.  A flood's field always has
 *      one where f >= 1; on a field that has none (rcw_guide_rule takes any) the result is that of 1.
 *   3  ct = (T(i) + 0.5, T(j) + 0.5), the centre of the agent's tile; cn the centre of n; e the agent's offset from ct ACROSS the axis of
 *      travel: y - ct.y where n differs in i, else x - ct.x.  The target p is cn where |e| <= inc, else ct: re-centre in the corridor
 *      first, then go — the player's circle never clips a corner it cannot pass.
 *   4  v = (p.x - x, p.y - y); s[k] = fl(fl(D1[k] * v.x) + fl(D2[k] * v.y)); heading = the smallest k of the largest s[k].  An argmax
 *      over the table as it is (rcw_set_direction_table may have installed any), not an atan2: rounded products compare the same
 *      everywhere.  A NaN s[k] never wins; where every s[k] is NaN, heading = 0.
 *   5  delta = (heading - d) mod nd.  0: action 1 (forward).  1 .. nd / 2 (integer division): action 3 (turn left, d + 1).  Otherwise
 *      action 4 (turn right).  The guide never moves backwards and never looks at collisions.
 * THE PROMISE, for position_increment_wu + player_radius_wu <= 0.5 (the sum in T) and the table rcw_create builds: an agent that follows
 * `action` from a start l tiles from its goal arrives within (l + 1) * (nd / 2 + 2 * ceil(1 / inc)) steps.  Outside that the words are
 * still defined and still exact — an agent whose circle cannot come within inc of a corridor's axis may just never arrive.
 * rcw_guide_info says which case a handle is in.
 * What each call does to the words — stream-ordered on the handle's stream, directly behind the goal distance's launch where that runs:
 *   rcw_set_guide(h, 1)           RCW_ERR_UNSUPPORTED on a handle without the goal distance.  Allocates and computes every agent's
 *                                 words; on a handle that has it, the same again.  An allocation failure leaves what was there.
 *   rcw_set_guide(h, 0)           frees them (RCW_OK also where there were none).
 *   rcw_set_goal_distance(h, 1)   (again) every agent's words from the new field.
 *   rcw_set_goal_distance(h, 0)   switches the guide off too.
 *   rcw_step, rcw_step_device, rcw_reset, rcw_set_state, rcw_set_state64, rcw_set_walls, the install and the restarts of the wall
 *   bank and of every generator family, rcw_set_direction_table*, rcw_snapshot_restore*
 *                                 every agent's words from the state the call leaves (the words are a pure function of field,
 *                                 position, heading and table: an agent outside the call's mask keeps the values it had).
 *   rcw_snapshot_save*, rcw_cast_rays, rcw_update_camera_view, rcw_update_top_view, rcw_set_step_form, rcw_set_time_limit, the
 *   learner-view, seen-map, local-map and statistics calls and every getter   nothing.
 * The words are no part of the state archive's record: a row is exchangeable between handles with and without the guide, and every
 * shape's key is what it was.  A replayed HIP graph of a step works like any step: nothing about this alternates on the host.  Capture
 * again after enabling or disabling.  The kernel (one launch, rcw_guide_kernel) runs OUTSIDE rcw_profile's events.
 *   rcw_guide_info         enabled; promised = 1 where inc + r <= 0.5 in T (either pointer may be NULL).
 *   rcw_guide              host copies of the two words (either pointer may be NULL); waits for the stream as rcw_done does.
 *   rcw_guide_device_ptr   the two arrays where they live (either pointer may be NULL), stable until the next rcw_set_guide.
 *   rcw_guide_rule         handle-less, needs no device: the rule for ONE agent on the host.  field UInt16 (H*W) in the order above,
 *                          H*W <= 65535; (x, y) as doubles, converted to T = Float32 (world_unit_bits 32) or Float64 (64), as is
 *                          position_increment; direction in 0 .. nd - 1; directions_wu (2, nd) in T, rcw_direction_table's layout.
 *                          Anything else — a NULL pointer included — is RCW_ERR_INVALID_ARGUMENT.
 * rcw_guide and rcw_guide_device_ptr return RCW_ERR_UNSUPPORTED on a handle that has not enabled it. */
RCW_API int rcw_set_guide(rcw_handle* h, int32_t enable);
RCW_API int rcw_guide_info(rcw_handle* h, int32_t* enabled, int32_t* promised);
RCW_API int rcw_guide(rcw_handle* h, uint8_t* action /* (B) */, int32_t* heading /* (B) */);
RCW_API int rcw_guide_device_ptr(rcw_handle* h, void** action, void** heading);
RCW_API int rcw_guide_rule(int32_t H, int32_t W, const void* field /* UInt16 (H*W) */, double x, double y, int32_t world_unit_bits, int32_t direction,
                           int32_t nd, const void* directions_wu /* (2, nd) in T */, double position_increment, uint8_t* action, int32_t* heading);
/* ---- the frontier (this build's addition: each agent's way to the nearest unseen tile, kept on the device) -----------------------------
 * Opt-in per handle, on a handle that has the seen map on: the boundary between what an agent has seen and what it has not, how far away
 * it is and which action leads there — a frontier-following expert for imitation or DAgger, the "explore until goal_seen, then follow the
 * guide" baseline a partially observing agent can match, a frontier-distance shaping term, an "exploration complete" signal — at no host
 * synchronisation.  A handle that never enables it runs exactly the kernels it ran before.  The ABI is additive: RCW_ABI_VERSION and
 * rcw_config are what they were.
 * THE DEFINITION.  For agent a, M its seen map, UInt8 (H*W) in the tile map's linear order (tile (i, j), 0-based, at i + H*j):
 *   passable(t)  <=>  M[t] is 1 or 3 (a seen free tile, a seen goal tile)
 *   source(t)    <=>  M[t] == 0 and some edge neighbour of t THAT LIES ON THE MAP is passable.  Tiles (H-1, j) and (0, j+1) are adjacent
 *                     in linear order and are no neighbours.
 * Per-agent state, device arrays:
 *   field      UInt16 (H*W, B), in the seen map's order.  A source holds 0.  A passable tile holds the least number of edge moves to a
 *              source, moving through passable tiles only; the last move enters the source, so a passable tile next to a source holds 1.
 *              Every other tile holds 0xFFFF: seen walls (2, 4), unseen tiles that are no sources, passable tiles from which no source
 *              can be reached.  A breadth-first level is a set: the values do not depend on the order in which a flood visits tiles.
 *   distance   Int32 (B)   field at the player's tile (floor x, floor y); -1 where that is 0xFFFF, or the tile is off the map, or x or y is
 *                          not finite (the kernel checks and never reads outside the field)
 *   tiles      Int32 (B)   the number of sources as of the agent's last flood
 *   action     UInt8 (B)   always in 1..4
 *   heading    Int32 (B)   the 0-based direction index to face; -1 where distance is -1 or the agent is off the map
 * action and heading are THE GUIDE'S RULE ("the guide" above, steps 1-5, verbatim) applied to this field in place of the goal distance's
 * — the same kernel, launched on this field.  The one definition makes that rule work unchanged: an agent always stands on a tile it has
 * seen, so its own entry is at least 1; one tile from the frontier it is told to face the unseen tile; facing it makes the view rays cross
 * it, the seen map changes, and the field is flooded again.  (An agent placed ON a source by rcw_set_state would hold 0 and be told to
 * turn on the spot, as on the goal tile; the seen map's launch in front marks the player's tile, so no call leaves an agent there.)
 * WHAT -1 MEANS: nothing left to explore from here.  distance == -1 on a seen free tile p says no source is reachable from p through
 * passable tiles.  Then every free tile q that is 4-connected to p through free tiles has been seen: walk a path of free tiles from p to q;
 * if some tile on it were unseen, the first such tile would have a seen free — passable — predecessor on the path, so it would be a source,
 * reachable from p along the seen part of the path.  And every tile next to such a q has been seen too: an unseen one would be a source
 * one move from q.  So the agent's whole component and its rim are on the map.
 * NO BOUND ON ARRIVAL IS PROMISED.  Observed on 13 x 13 generated mazes with loops 0.1, nd 16, 8 rays, position_increment =
 * player_radius = 0.25, agents that follow `action` until distance == -1 or until they touch their goal: 16 agents of the CPU reference
 * (tests/test_frontier_spec.py, which allows 2,000 steps) took 333 steps at most; of 256 agents on the device (tests/test_gpu_frontier.py,
 * which allows 4,000) 8 were still exploring after 500 steps and none after 1,000.  A direction table without an axis-aligned heading
 * (nd 7) may never get there — the limit the guide's promise states.
 * What each call does — stream-ordered on the handle's stream, directly behind the seen map's launch, with no host wait:
 *   rcw_set_frontier(h, 1)        RCW_ERR_UNSUPPORTED on a handle without the seen map.  Allocates, floods every agent and computes all
 *                                 words; on a handle that has it, the same again.  An allocation failure leaves what was there.
 *   rcw_set_frontier(h, 0)        frees it (RCW_OK also where there was none).
 *   rcw_set_seen_map(h, 1)        (again) every agent is flooded again from the new map, and the words follow.
 *   rcw_set_seen_map(h, 0)        while the frontier is on: RCW_ERR_UNSUPPORTED, nothing changes (the local map's rule for RCW_LOCAL_SEEN).
 *   rcw_reset, rcw_set_state, rcw_set_state64, rcw_set_walls
 *                                 the agents of the call's mask are flooded again; the others keep field, distance and tiles.  action and
 *                                 heading, a pure function of field, pose and table, are computed again for every agent.
 *   rcw_step, rcw_step_device     an agent is flooded again if and only if its episode counter differs from the one recorded at its last
 *                                 flood, or the seen map's newly_seen word of this call is not 0; every other agent gets only distance
 *                                 re-read at its new tile.  action and heading for every agent.  This covers the install and the restarts
 *                                 of the wall bank and of every generator family: the features run once behind the final world.
 *   rcw_set_direction_table*      action and heading only.
 *   rcw_snapshot_restore*         field and words are NO part of the record.  Behind the restore's render the agents of the mask are
 *                                 flooded again from the restored seen map; action and heading for every agent.
 *   rcw_set_time_limit, the learner-view, goal-distance, guide, local-map and statistics calls, rcw_snapshot_save* and every getter
 *                                 nothing.
 * A replayed HIP graph of a step behaves like any step: nothing about this alternates on the host, the recorded episode counter lives on
 * the device.  Capture again after enabling or disabling.  The launches (rcw_frontier_kernel, then the guide's kernel) run OUTSIDE
 * rcw_profile's events.
 *   rcw_frontier_info               enabled.
 *   rcw_frontier                    host copies of distance, tiles, action, heading (any pointer may be NULL); waits for the stream as
 *                                   rcw_done does.
 *   rcw_frontier_device_ptr         the four arrays where they live (any pointer may be NULL), stable until the next rcw_set_frontier.
 *   rcw_frontier_field              agents [first, first + count) of the field to the host; waits for the stream.
 *   rcw_frontier_field_device_ptr   the field where it lives.
 *   rcw_frontier_rule               handle-less, needs no device: the flood for ONE agent on the host.  seen_map UInt8 (H*W) in the order
 *                                   above — any byte above 4 counts as a wall —, field_out UInt16 (H*W), *tiles_out the number of sources.
 *                                   H, W >= 1 and H*W <= 65535; anything else — a NULL pointer included — is RCW_ERR_INVALID_ARGUMENT.
 * The readouts return RCW_ERR_UNSUPPORTED on a handle that has not enabled it. */
RCW_API int rcw_set_frontier(rcw_handle* h, int32_t enable);
RCW_API int rcw_frontier_info(rcw_handle* h, int32_t* enabled);
RCW_API int rcw_frontier(rcw_handle* h, int32_t* distance /* (B) */, int32_t* tiles /* (B) */, uint8_t* action /* (B) */, int32_t* heading /* (B) */);
RCW_API int rcw_frontier_device_ptr(rcw_handle* h, void** distance, void** tiles, void** action, void** heading);
RCW_API int rcw_frontier_field(rcw_handle* h, int32_t first, int32_t count, void* out_host /* UInt16 (H*W, count) */);
RCW_API int rcw_frontier_field_device_ptr(rcw_handle* h, void** ptr);
RCW_API int rcw_frontier_rule(int32_t H, int32_t W, const uint8_t* seen_map /* (H*W) */, void* field_out /* UInt16 (H*W) */, int32_t* tiles_out);
/* ---- the visit map (this build's addition: how often each agent has stood where it stands, kept on the device) ------------------------
 * Opt-in per handle: the visit count of count-based exploration — the episodic count N_ep(s) that RIDE and AGAC scale their bonus by
 * (1 / sqrt N_ep), that BeBold / NovelD gate theirs by (N_ep == 1), the plain beta / sqrt N bonus — and, optionally, the cumulative count
 * per level shared by every agent that plays it, at no host synchronisation.  The seen map is no visit count: it records what the rays
 * crossed, not where the agent was, and holds a flag.  A handle that never enables it runs exactly the kernels it ran before.  The ABI is
 * additive: RCW_ABI_VERSION and rcw_config are what they were.
 * PARAMETERS, fixed when the feature is enabled: sectors, 1 <= sectors <= RCW_VISIT_MAX_SECTORS and sectors <= num_directions; flags, whose
 * only bit is RCW_VISIT_TABLE; cells = sectors * H * W.
 * THE CELL of agent a: its tile t = i + H*j with (i, j) = (floor x, floor y), the floor taken in the world-unit type (wu_to_tu minus
 * one); its sector s = (d * sectors) / nd by integer division, d its 0-based direction index — the index, not the table's vectors: a new
 * direction table changes nothing —; its cell c = s*H*W + t.  An agent has NO CELL where x or y is not finite or the tile is off the map
 * (the kernel checks and never indexes outside the map).
 * Per-agent state, device arrays:
 *   map         UInt16 (cells, B), agent a's at a*cells; within a sector the tile map's own linear order (the seen map's)
 *   here        Int32 (B)    the entry of the agent's cell after the call; 0 where it has no cell
 *   visited     Int32 (B)    the number of non-zero entries of the agent's map
 *   first       Int32 (B)    1 iff the call counted a cell whose entry was 0; 0 otherwise, and 0 behind a BEGIN
 *   level_here  UInt32 (B)   with the table: below; 0 on a handle without it
 *   (private)   the agent's episode counter as of its last BEGIN
 * COUNT(a), for an agent with a cell:   v = map[c]; first = (v == 0); map[c] = min(v + 1, 65535); visited += first; here = map[c].
 *           Without a cell: here = first = 0, and nothing else happens.
 * BEGIN(a): every entry of the agent's map becomes 0, visited becomes 0; COUNT at the current pose; then first = 0 and the counter is
 *           recorded.
 * THE TABLE (with RCW_VISIT_TABLE): UInt32 (cells, 1 + rows), row r at r*cells.  rows and first_level follow episode statistics' rule from
 * the layout source that is live when the feature is enabled (rows = the bank's layouts, or a family's `levels` with first_level; 0
 * without a source, with levels == 0 or above RCW_EPISODE_STATS_MAX_ROWS); where cells * (1 + rows) * 4 would pass
 * RCW_VISIT_TABLE_MAX_BYTES, rows = 0 — no error: row 0 always works.  Every COUNT of an agent with a cell — the one inside a BEGIN
 * too, and whether or not the map entry saturated — adds 1 to table[0][c] and to table[1 + k][c], k = layout - first_level, where
 * 0 <= k < rows; layout is rcw_wall_layout's word of the agent as it is behind the call.  Entries wrap modulo 2^32.  All adds are integer
 * adds: the table does not depend on the order in which agents are processed.
 *   level_here[a] = table[r][c] AS OF THE END OF THE CALL, after every agent's adds, r = 1 + k where k is in range, else 0 — so it does
 *           not depend on that order either, and two agents that share a row and a cell read the same value.  It is read again for EVERY
 *           agent (0 for one without a cell) behind every step and every reset / set_state / set_walls, the agents outside such a call's
 *           mask included: their own entry may have grown.
 * What each call does — stream-ordered on the handle's stream behind everything the call already queues, with no host wait:
 *   rcw_set_visit_map(h, 1, sectors, flags)
 *                                 allocates, zeroes the table, BEGIN for every agent.  On a handle that has it: the same again, with the
 *                                 new parameters.  An allocation failure leaves what was there.
 *   rcw_set_visit_map(h, 0, ...)  frees it (RCW_OK also where there was none).
 *   rcw_step, rcw_step_device     an agent whose episode counter differs from the recorded one — a done or truncated restart under
 *                                 auto_reset, with or without a layout source — gets BEGIN; every other agent COUNT at its pose after the
 *                                 step.  The action is not looked at: a blocked move, a turn, an invalid device action count the cell the
 *                                 agent is on; a done agent without auto_reset is counted like any other.
 *   rcw_reset, rcw_set_state, rcw_set_state64, rcw_set_walls
 *                                 BEGIN for the agents of the call's mask; every other agent keeps every byte of its map and here, visited
 *                                 and first.  The mask decides, not the counter.
 *   rcw_set_wall_bank, rcw_set_wall_generator, rcw_set_wall_caves, rcw_set_wall_rooms (install, replace or remove)
 *                                 with RCW_VISIT_TABLE: RCW_ERR_UNSUPPORTED, and nothing changes (the level rows were counted from the
 *                                 live source: the statistics' rule).  Without the table: an install restarts every agent, so BEGIN for
 *                                 every agent; a removal does nothing (what the seen map does).
 *   rcw_visit_table_clear         zeroes the table without waiting for the stream; no per-agent word is touched.
 *   rcw_snapshot_restore*         map, the four words and the private counter are part of the record: the restored agents hold the
 *                                 save's, and nothing is counted.  The table is no part of a record and is not rolled back.
 *   rcw_set_direction_table*, rcw_set_step_form, rcw_set_time_limit, the renderers, every other feature's calls and every getter
 *                                 nothing.
 * A replayed HIP graph of a step counts like any step: the recorded counter lives on the device.  Capture again after enabling or
 * disabling.  The launches (rcw_visit_map_kernel and, with the table, rcw_visit_table_read_kernel) run OUTSIDE rcw_profile's events.
 *   rcw_visit_map_info            enabled, sectors, flags, rows, first_level (any pointer may be NULL); zeros while off.
 *   rcw_visit_words               host copies of here, visited, first, level_here (any pointer may be NULL); waits for the stream as
 *                                 rcw_done does.
 *   rcw_visit_words_device_ptr    the four arrays where they live (any pointer may be NULL), stable until the next rcw_set_visit_map.
 *   rcw_visit_map                 agents [first, first + count) of the map to the host; waits for the stream.
 *   rcw_visit_map_device_ptr      the map where it lives.
 *   rcw_visit_table               the table, UInt32 (cells, 1 + rows), to the host; waits for the stream.
 *   rcw_visit_table_device_ptr    the table where it lives.
 *   rcw_visit_cell                handle-less, needs no device: the cell rule for ONE agent on the host; *cell = -1: no cell.  H, W >= 1
 *                                 with 8 H W < 2^31, nd >= 1, 0 <= direction < nd, 1 <= sectors <= min(RCW_VISIT_MAX_SECTORS, nd),
 *                                 world_unit_bits 32 (x and y are rounded to Float32 first) or 64; anything else — a NULL pointer included —
 *                                 is RCW_ERR_INVALID_ARGUMENT.
 * The readouts return RCW_ERR_UNSUPPORTED on a handle that has not enabled it, the three table calls also on one without the table. */
#define RCW_VISIT_MAX_SECTORS 8
#define RCW_VISIT_TABLE 1
#define RCW_VISIT_TABLE_MAX_BYTES (256u * 1024u * 1024u)
RCW_API int rcw_set_visit_map(rcw_handle* h, int32_t enable, int32_t sectors, int32_t flags);
RCW_API int rcw_visit_map_info(rcw_handle* h, int32_t* enabled, int32_t* sectors, int32_t* flags, int32_t* rows, int32_t* first_level);
RCW_API int rcw_visit_words(rcw_handle* h, int32_t* here /* (B) */, int32_t* visited /* (B) */, int32_t* first /* (B) */, uint32_t* level_here /* (B) */);
RCW_API int rcw_visit_words_device_ptr(rcw_handle* h, void** here, void** visited, void** first, void** level_here);
RCW_API int rcw_visit_map(rcw_handle* h, int32_t first, int32_t count, void* out_host /* UInt16 (cells, count) */);
RCW_API int rcw_visit_map_device_ptr(rcw_handle* h, void** ptr);
RCW_API int rcw_visit_table(rcw_handle* h, uint32_t* out_host /* (cells, 1 + rows) */);
RCW_API int rcw_visit_table_device_ptr(rcw_handle* h, void** ptr);
RCW_API int rcw_visit_table_clear(rcw_handle* h);
RCW_API int rcw_visit_cell(int32_t H, int32_t W, int32_t nd, int32_t sectors, double x, double y, int32_t world_unit_bits, int32_t direction, int32_t* cell);

/* ---- the start rule (this build's addition: each episode's player placed by its path distance to the goal) --------------------------------
 * reset!(world) SR:110-137 draws the player uniformly on any empty tile.  With interior walls that can be a tile the goal cannot be reached
 * from, and it leaves no handle on the one curriculum knob navigation benchmarks share: the geodesic distance between start and goal.
 * rcw_set_start_distance keeps a BAND [lo, hi] of shortest-path distances on the handle; from then on every episode that starts places its
 * player on a tile of that band, on the device, with no host synchronisation.  It needs no goal distance (the kernel floods for itself in LDS) and a handle
 * that never enables it launches exactly what it launched before.  The ABI is additive: RCW_ABI_VERSION and rcw_config are what they were.
 * THE RULE, for an agent a that began episode e in the call (its counter moved to e + 1), behind reset!'s draws — or the layout source's
 * restart — which have written goal, pose and heading.  Integers only:
 *   1. F is the breadth-first field from the goal tile through the agent's walls, exactly as "the goal distance" above defines it: moves are
 *      4-neighbour and look at WALL bits only, F[goal] = 0, walls and unreached tiles hold 0xFFFF, a goal inside a wall reaches nothing.
 *   2. E is the tiles t, in the tile map's linear order t = (i - 1) + H (j - 1), with lo <= F[t] <= hi.  E not empty: outcome
 *      RCW_START_IN_BAND.
 *   3. E empty: D is the largest real distance in F.  D >= 1: E is the tiles with F[t] == D, outcome RCW_START_CLAMPED (lo >= 1, so this is
 *      D < lo: the band lies beyond the reachable space and is clamped to the farthest tiles).  D == 0 or nothing reached: outcome
 *      RCW_START_KEPT — the pose reset! drew stays, as do the agent's status word and everything else.
 *   4. IN_BAND, CLAMPED: n = |E|, r = below(draw(key, 2^63 + 2^62), n) with key = the episode key of (seed, agent_id_offset + a, e); the
 *      player goes to the centre of the r-th tile of E in ascending t, (T)(i - 0.5), (T)(j - 0.5) as reset! writes a tile's centre.  Heading,
 *      goal, reward, done, the counter, the status word and the time limit's words stay.  (Draw 2^63 + 2^62 meets no other draw on the
 *      episode key: reset!'s own indices count from 0 and stay below 2^31, the layout sources take 2^63.)
 *   5. placed[a] = outcome, UInt8; RCW_START_NOT_YET (0): no episode of the agent has begun under the rule.
 * A pure function of (seed, global agent id, episode, walls, goal, band): a shard equals its slice of the batch, and rcw_start_rule replays
 * it on the host.  BAND: 1 <= lo <= hi <= RCW_START_DISTANCE_MAX; hi = RCW_START_DISTANCE_MAX means "no upper bound", and (1, max) is the
 * plain "start where the goal can be reached" guarantee.  Anything else is RCW_ERR_INVALID_ARGUMENT and changes nothing.
 * WHAT EACH CALL DOES
 *   rcw_set_start_distance(h, 1, lo, hi)
 *                                 on a handle without it: allocates, records the counters as they are, placed = 0.  NO AGENT MOVES and no
 *                                 frame changes: the rule holds from the next start of an episode.  On a handle that has it: only the band
 *                                 changes — no allocation, no wait; the band is a kernel argument of the launches that follow, so the change
 *                                 is stream-ordered.  A captured HIP graph of a step keeps the band it was captured with.
 *   rcw_set_start_distance(h, 0, ...)
 *                                 frees it (RCW_OK also where there was none).
 *   rcw_step, rcw_step_device     behind the step (and the layout source's kernel, if any): an agent whose counter differs from the recorded
 *                                 one — a done or truncated restart under auto_reset — is placed; those agents are cast and painted once
 *                                 more through the masked path, once, in both step forms, with RCW_VIEW_ONLY and with a top view; then
 *                                 every feature runs once and finds the placed pose (start_distance is the placed tile's distance).
 *   rcw_reset, rcw_set_walls      the agents of the call's mask (their counters moved) are placed before the call's render.
 *   rcw_set_wall_bank, rcw_set_wall_generator, rcw_set_wall_caves, rcw_set_wall_rooms (install)
 *                                 every agent restarts on a layout of the source and is placed on it.
 *   rcw_set_state, rcw_set_state64
 *                                 nothing: the caller's pose stands, no counter moves.
 *   rcw_snapshot_save / restore*  the recorded counter and placed are part of the record (the mask is not): an agent restored into a running
 *                                 episode is not placed again.  A handle with the rule has a shape key of its own.
 *   every other call              nothing.
 * The launch (rcw_start_distance_kernel) and the masked re-render behind it run OUTSIDE rcw_profile's events — but for a handle whose learner
 * view is set with RCW_VIEW_ONLY: there the kernel and the masked cast lie between the step's cast and its view kernel, and count into
 * cast_ms (as the layout source's kernel does).
 *   rcw_start_distance_info       enabled, lo, hi (any pointer may be NULL); zeros while off.
 *   rcw_start_distance            host copy of placed; waits for the stream as rcw_done does.
 *   rcw_start_distance_device_ptr placed where it lives, stable until the rule is switched off.
 *   rcw_start_rule                handle-less, needs no device: steps 1 to 4 for ONE agent on the host.  walls UInt8 (H*W), non-zero = WALL, in
 *                                 the tile map's order; (gi, gj) the goal, 1-based; key the episode key.  *tile: the chosen t (0-based), -1
 *                                 with RCW_START_KEPT; *outcome: 1..3.  H, W >= 1 with H W <= 65535 and a valid band; anything else — a NULL
 *                                 pointer included — is RCW_ERR_INVALID_ARGUMENT.  It looks at neighbours by (row, column) and so takes maps
 *                                 without a wall ring too; the device floods by linear index and relies on the ring every map of a handle
 *                                 has (rcw_set_walls refuses one without): the two agree on ringed maps, which is what a handle can hold.
 * The two readouts return RCW_ERR_UNSUPPORTED on a handle that has not enabled it. */
#define RCW_START_DISTANCE_MAX 65534
#define RCW_START_NOT_YET 0
#define RCW_START_IN_BAND 1
#define RCW_START_CLAMPED 2
#define RCW_START_KEPT 3
RCW_API int rcw_set_start_distance(rcw_handle* h, int32_t enable, int32_t lo, int32_t hi);
RCW_API int rcw_start_distance_info(rcw_handle* h, int32_t* enabled, int32_t* lo, int32_t* hi);
RCW_API int rcw_start_distance(rcw_handle* h, uint8_t* placed_host /* (B) */);
RCW_API int rcw_start_distance_device_ptr(rcw_handle* h, void** placed);
RCW_API int rcw_start_rule(const uint8_t* walls /* (H*W) */, int32_t H, int32_t W, int32_t gi, int32_t gj, uint64_t key, int32_t lo, int32_t hi,
                           int32_t* tile, int32_t* outcome);

/* ---- The state archive (this build's addition: the reference has no checkpoint) -------------------------------------------------------
 * `rows` agent RECORDS kept on the device and owned by the handle: save scatters the records of the masked agents into rows, restore
 * gathers rows back into the masked agents and renders them again — what ALE's cloneState / restoreState and Procgen's get_state /
 * set_state give, for every agent at once and without leaving the device.  Both take per-agent row indices, so several agents may restore
 * from one row.  A handle that never calls rcw_set_snapshots allocates and launches exactly what it did before.
 *
 * A record is a list of SEGMENTS, one per per-agent array; it holds everything the next step of an agent reads that a render does not
 * compute again:
 *   always             pos (pos64 for T = Float64), dir, goal, reward (in R), done, episode, tile_map, episode_steps, truncated
 *   goal distance      field, distance, start_distance, progress, and the flood's private episode counter
 *   seen map           seen_count, newly_seen, goal_seen, the private episode counter, the packed bits, the map
 *   learner view       the frame (k = 1), or the k-frame stack and its private episode counter
 *   local map          the image (stored, not computed again: its bytes are what they were at the save)
 *   layout source      the source's private episode counter and the agents' layout index / level
 *   episode statistics the seven words, the previous position (x, y), the private episode counter
 *   visit map          here, visited, first, level_here, the private episode counter, the map (its tag carries `sectors`); not the table
 * A record does NOT hold
 *   the camera view, the column descriptors, the one-launch step's slots, the top view        a restore renders them again;
 *   the agents' status words and the layout source's record of them                           the agent SLOT's error log, like the
 *                                                                                             handle's error word: they stay the slot's;
 *   the layout source's transient mask, the episode statistics' table                         a launch's scratch; a log of the batch;
 *   any setting of the handle — seed, time limit, bank and weights, generator parameters,     these are the handle's as of the restore.
 *   direction table —
 *   the guide's two words                                                                     a restore computes them again: a row fits
 *                                                                                             a handle with or without the guide;
 *   the frontier's field and words                                                            a restore floods the restored agents again
 *                                                                                             from the restored seen map: a row fits a
 *                                                                                             handle with or without the frontier;
 * If row r was saved from agent j and is restored into agent i, agent i holds j's world; its next episode starts under i's global id and
 * the copied episode counter.
 *
 *   rcw_set_snapshots(h, rows)   binds the archive to the handle's SHAPE as of now — which features are on, the learner view's format, size
 *                                and k, the local map's size, the kind of the layout source — and allocates `rows` records, 0 ..
 *                                RCW_SNAPSHOT_MAX_ROWS, none of them filled; 0 frees the archive.  Again: bound anew, and empty.  A failed
 *                                allocation returns RCW_ERR_OUT_OF_MEMORY and the old archive stays.  Waits for the stream.
 *   rcw_snapshot_info            rows, the bytes of a record as rcw_snapshot_rows_copy hands it out, and the shape key: a 64-bit hash
 *                                (FNV-1a) of the segment table, the geometry, T, R and RCW_ABI_VERSION.  Any pointer may be NULL.  Without
 *                                an archive: rows 0 and the record the handle's shape would have now.
 * A save or restore of a handle whose shape is no longer the archive's returns RCW_ERR_UNSUPPORTED, names the first segment that differs
 * and changes nothing.
 *   rcw_snapshot_save / rcw_snapshot_restore (h, rows_host, mask_host)
 *                                rows_host Int32 (B): agent a's row; NULL: row a, which needs rows >= B.  mask_host UInt8 (B) or NULL:
 *                                every agent.  The host checks the masked agents' indices — in 0 .. rows - 1; restore: a filled row; save:
 *                                distinct rows — and a violation returns RCW_ERR_INVALID_ARGUMENT, names the agent and changes nothing.
 *                                They wait for the stream (the staging of their arguments; restore also reads which rows are filled).
 *   rcw_snapshot_save_device / rcw_snapshot_restore_device (h, rows_device, mask_device)
 *                                the same with both arrays in DEVICE memory (either may be NULL as above): stream-ordered, no host wait,
 *                                capturable like rcw_step_device.  A masked agent whose index is out of range — or, restore, names an
 *                                unfilled row — is left exactly as it was; its status word and the handle's error word become
 *                                RCW_ERR_INVALID_ARGUMENT (as an invalid action's become RCW_ERR_INVALID_ACTION; rcw_clear_error clears
 *                                them), and the other agents are served.  Two masked agents MAY save into one row: it then holds the whole
 *                                record of the higher-numbered agent, never a mixture.
 * A save launches the scatter alone.  A restore launches the gather and then casts and paints the masked agents from the state they now
 * hold; the flood, the seen map, the stack, the local map and the statistics are the record's.
 *   rcw_snapshot_filled          UInt8 (rows) to host memory: 1 where a save or a load has filled the row.  Waits for the stream.
 *   rcw_snapshot_rows_copy       rows [first, first + count) to host memory, row_bytes each: the segments in the table's order, unpadded
 *                                (an unfilled row reads as zeros).  Waits for the stream; a sticky device error comes back instead of
 *                                the rows (rcw_clear_error first).
 *   rcw_snapshot_rows_load       ... and back, into rows [first, first + count) of an archive whose shape key is `shape_key` (another key,
 *                                or a handle whose shape is no longer the archive's: RCW_ERR_UNSUPPORTED).  For every row the host checks the fields a kernel INDEXES with — goal an interior
 *                                tile, direction in 0 .. nd - 1, position finite and inside the room, the map's border WALL bits set and
 *                                its padding clear, the layout index in the live source's range — and a violation returns
 *                                RCW_ERR_INVALID_ARGUMENT, names row and field, and nothing is loaded.  EVERYTHING ELSE IS TRUSTED, as
 *                                rcw_set_walls trusts its caller: rows are the output of rcw_snapshot_rows_copy, not a format to write.
 *                                The rows count as filled.  Waits for the stream.
 * All but rcw_set_snapshots and rcw_snapshot_info return RCW_ERR_UNSUPPORTED on a handle without an archive. */
#define RCW_SNAPSHOT_MAX_ROWS 1048576
RCW_API int rcw_set_snapshots(rcw_handle* h, int32_t rows);
RCW_API int rcw_snapshot_info(rcw_handle* h, int32_t* rows, uint64_t* row_bytes, uint64_t* shape_key);
RCW_API int rcw_snapshot_save(rcw_handle* h, const int32_t* rows_host /* (B) or NULL */, const uint8_t* mask_host /* (B) or NULL */);
RCW_API int rcw_snapshot_restore(rcw_handle* h, const int32_t* rows_host /* (B) or NULL */, const uint8_t* mask_host /* (B) or NULL */);
RCW_API int rcw_snapshot_save_device(rcw_handle* h, const int32_t* rows_device, const uint8_t* mask_device);
RCW_API int rcw_snapshot_restore_device(rcw_handle* h, const int32_t* rows_device, const uint8_t* mask_device);
RCW_API int rcw_snapshot_filled(rcw_handle* h, uint8_t* out_host /* (rows) */);
RCW_API int rcw_snapshot_rows_copy(rcw_handle* h, int32_t first, int32_t count, void* out_host /* (row_bytes, count) */);
RCW_API int rcw_snapshot_rows_load(rcw_handle* h, int32_t first, int32_t count, const void* in_host /* (row_bytes, count) */, uint64_t shape_key);
/* world.player_position_wu SR:24, world.player_direction_au SR:25, world.goal_position SR:32 */
RCW_API int rcw_position(rcw_handle* h, float* out_host /* (2, B) */);
RCW_API int rcw_direction(rcw_handle* h, int32_t* out_host /* (B) */);
RCW_API int rcw_goal(rcw_handle* h, int32_t* out_host /* (2, B), 1-based */);
RCW_API int rcw_episode(rcw_handle* h, uint32_t* out_host /* (B): resets seen by each agent */);
/* Per-agent sticky status: 0, RCW_ERR_OUT_OF_BOUNDS (see RCW_OOB_ERROR),
 * RCW_ERR_INVALID_ACTION (rcw_step_device) or — a warning, where no error is recorded —
 * RCW_WARN_SAMPLER_GAVE_UP (utils.jl:34).  Does not fail on a set error word, so it can
 * be used to find the faulting agents. */
RCW_API int rcw_status(rcw_handle* h, int32_t* out_host /* (B) */);
/* world.tile_map SR:22 as BitArray{3}(2, H, W).chunks per agent: UInt64 (nchunks, B),
 * nchunks = rcw_tile_map_num_chunks(). Bit (o-1) + 2(i-1) + 2H(j-1), LSB first. */
RCW_API int rcw_tile_map_num_chunks(rcw_handle* h, int32_t* out);
RCW_API int rcw_tile_map_chunks(rcw_handle* h, uint64_t* out_host);
/* world.ray_stop_position_tu / ray_hit_dimension / ray_distance_wu / ray_directions_wu
 * SR:29-31,39 for agents [first, first+count), recomputed from the current state by a
 * cast-only kernel (the step itself does not spend HBM bandwidth on them).
 * Any output pointer may be NULL. */
RCW_API int rcw_rays(rcw_handle* h, int32_t first, int32_t count,
             int64_t* stop_ij /* (2, N, count) */, int64_t* hit_dimension /* (N, count) */,
             float* distance_wu /* (N, count) */, float* directions_wu /* (2, N, count) */);
/* Compact per-column descriptor of the current frames, indexed by image column k
 * (k = N - i + 1, SR:431): height_line_pu SR:408-411 (Int32, saturated) and colour id.
 * In the two-launch step these arrays are what the cast kernel hands to the fill kernel, refreshed by every step.  The one-launch
 * step (RCW_STEP_ONE_LAUNCH below) does not need them and every store of its casting workgroups costs the launch more than its bytes:
 * it refreshes them only for a caller that holds the device pointers — from the first rcw_columns_device_ptr call on, every step of
 * the handle does —; otherwise rcw_columns, the gathers and rcw_update_camera_view recast the current state (the cast kernel,
 * no action, ~10 us at 4096 agents x 256 columns) in front of their read, on demand. */
RCW_API int rcw_columns(rcw_handle* h, int32_t first, int32_t count,
                int32_t* height_line_pu /* (N, count) */, uint8_t* colour_id /* (N, count) */);
RCW_API int rcw_columns_device_ptr(rcw_handle* h, void** height_line_pu, void** colour_id);
/* Expand descriptors (DEVICE pointers, e.g. gathered from another GPU) into frames
 * UInt32 (H_cam, N, count) in DEVICE memory, with this handle's colours and H_cam:
 * the receiving side of the compact observation gather. */
RCW_API int rcw_expand_columns(rcw_handle* h, const int32_t* height_line_pu_device,
                       const uint8_t* colour_id_device, int32_t count, void* frames_device);

/* ---- the learner view: a uint8 observation a learner consumes, rendered from the column descriptors -----------------------
 * Opt-in per handle.  Once set, every rcw_reset / rcw_set_state / rcw_step / rcw_step_device also renders it, on the handle's
 * stream behind the camera view (a masked reset or set_state: the masked agents only); a handle that never sets it runs what it
 * ran before.  Pixel contract (exact, integer), with H = height_camera_view_pu, N = num_rays and the frame of agent b as the
 * camera view holds it (image column k, row y, row 0 at the top):
 *   size (h, w) with 1 <= h <= H and 1 <= w <= N (no up-sampling); output row r covers rows [floor(r H / h), floor((r+1) H / h)),
 *   output column c covers columns [floor(c N / w), floor((c+1) N / w)) — never empty, not all of one size;
 *   RCW_VIEW_RGB8: R = (p >> 16) & 0xFF, G = (p >> 8) & 0xFF, B = p & 0xFF of each pixel p, each channel (S + floor(n/2)) / n over
 *                  the box's n pixels (S their sum: round half up);
 *   RCW_VIEW_GRAY8: Y = (77 R + 150 G + 29 B + 128) >> 8 of each pixel, averaged the same way (reference colours: ceiling 255,
 *                  floor 64, walls 128 / 192, goal 39 / 58);
 *   at (h, w) = (H, N) the RGB view is the camera view's bytes, transposed to rows first.  The handle's configured colours apply.
 * The depth plane (bit 2 of the format: "a depth plane D follows the colour planes").  RCW_VIEW_DEPTH8: C = 1, D alone; RCW_VIEW_RGBD8
 * (= RCW_VIEW_RGB8 | 4): C = 4, R, G, B, D; RCW_VIEW_GRAYD8 (= RCW_VIEW_GRAY8 | 4): C = 2, Y, D.  Format 3 and every value from 7 up:
 * RCW_ERR_INVALID_ARGUMENT.  D is inverse depth, exact in integers.  For image column k of an agent let hl be its height_line_pu (the
 * descriptor rcw_columns hands out) and pad its column padding (hl >= H - 1: 0; otherwise min((H - hl) / 2, H), rounded down): rows
 * [0, pad) show the ceiling, [pad, H - pad) the column's colour, the rows from max(pad, H - pad) on the floor — the rule the colour
 * planes follow.  Pixel (y, k) has an inverse depth of u pixels,
 *   u = min(max(hl, 0), H)           where pad <= y < H - pad (the colour's rows: the height of the column's line, clipped),
 *   u = H - 2 min(y, H - 1 - y)      on the ceiling and floor rows: the height a line would need for y to be its first or last row,
 *                                    i.e. the inverse depth of the ceiling or floor point seen through that pixel,
 * and the full-size byte is D(y, k) = (255 u + floor(H / 2)) / H, rounded down: 255 = at or nearer than the distance at which a wall
 * fills the column, 0 = infinitely far.  At reduced sizes D is averaged over the same boxes with the same rounding as the colour
 * channels, (S + floor(n/2)) / n.  What follows: D(y, k) = D(H - 1 - y, k) wherever pad <= H / 2; a column with pad = 0 is one value;
 * the colour planes of RCW_VIEW_RGBD8 / RCW_VIEW_GRAYD8 are byte for byte the RCW_VIEW_RGB8 / RCW_VIEW_GRAY8 view.  Approximately (the
 * integer rule above is the contract) D / 255 = d0 / perpendicular distance, clipped at 1, with d0 = camera_height_tile_wu * num_rays
 * / (2 semi_field_of_view_wu * H) — camera_height_tile_wu / (2 semi_field_of_view_wu) where the view is as high as it is wide, as
 * height_line_pu counts square pixels of a view num_rays wide.  Layouts, sizes, flags, the frame stack and every rule below about when
 * the view is written are those of the colour formats with this C.
 * Layouts: RCW_VIEW_CHW (B, C, h, w) or RCW_VIEW_HWC (B, h, w, C), C order (Julia sees (w, h, C, B) / (C, w, h, B)); gray and depth
 * have C = 1 and both layouts are the same bytes.
 * RCW_VIEW_ONLY: a step is the cast kernel followed by the view kernel — the UInt32 camera view is NOT written by steps (see
 * rcw_obs_device_ptr; rcw_update_camera_view renders it on demand), the step takes two launches (rcw_step_form) and
 * rcw_set_step_form(h, RCW_STEP_ONE_LAUNCH) returns RCW_ERR_UNSUPPORTED.  The top view, if enabled, is rendered as before.
 * The frame stack (rcw_set_learner_view_stack, frames = k, 1 <= k <= RCW_VIEW_MAX_FRAMES): the view batch is uint8 (B, k C, h, w), C
 * order; channel s C + c is channel c of frame slot s, slot 0 the OLDEST frame and slot k - 1 the newest, and each slot holds exactly
 * the bytes the single-frame view of that state holds.  k > 1 requires RCW_VIEW_CHW (RCW_VIEW_HWC: RCW_ERR_UNSUPPORTED); k = 1 is
 * rcw_set_learner_view in every respect (kernels, launches, buffer, bytes).  The stack follows each agent's episode on the device:
 *   setting the view                          all k slots of every agent hold the view of the current state;
 *   rcw_reset / rcw_set_state / _set_state64  all k slots of every agent the call touches (its mask, not the episode counter, decides)
 *     (and rcw_set_direction_table*)          hold the new frame; an agent outside the mask keeps every byte;
 *   rcw_step / rcw_step_device                one push per agent per call: an agent whose episode counter (rcw_episode) differs from the
 *                                             value recorded at its previous push — auto_reset re-sampled it in this step — has all k
 *                                             slots set to the new frame; otherwise slot s takes slot s + 1 (s = 0 .. k - 2) and slot
 *                                             k - 1 the new frame.  The step in which an agent reaches its goal is an ordinary push (the
 *                                             terminal frame is the newest slot; the restart follows one step later, as `done` does);
 *                                             an agent whose device action is invalid is not stepped, yet its unchanged frame is pushed;
 *   rcw_cast_rays, rcw_update_camera_view, rcw_update_top_view, rcw_expand_columns_view (single-frame), rcw_set_step_form and every
 *   getter                                    do not touch the stack.
 * A replay of a captured step is a push like any other: nothing about the stack alternates on the host, and the device pointer is
 * stable until the next rcw_set_learner_view*.  RCW_VIEW_ONLY changes nothing of this.
 *   rcw_set_learner_view         allocates the B*C*h*w bytes and renders the current state into them at once; RCW_VIEW_OFF
 *                                frees them.  A bad argument or an allocation failure leaves the previous view as it was.
 *   rcw_set_learner_view_stack   the same with `frames` slots an agent (B*frames*C*h*w bytes); frames outside 1..RCW_VIEW_MAX_FRAMES:
 *                                RCW_ERR_INVALID_ARGUMENT.  rcw_set_learner_view is this call with frames = 1.
 *   rcw_learner_view_info        the current settings (format RCW_VIEW_OFF and zeros when there is none).
 *   rcw_learner_view_stack       the current number of frame slots, 0 when there is no view.
 *   rcw_learner_view_device_ptr  the view batch (the whole stack) in DEVICE memory, aliased: stable until the next rcw_set_learner_view*.
 *   rcw_learner_view_copy        agents [first, first+count) to host memory, frames*C*h*w bytes each (waits for the stream).
 *   rcw_expand_columns_view      the handle's learner view (format, layout, size) of `count` agents' descriptors in DEVICE memory
 *                                (e.g. gathered from other GPUs) into view_device (count*C*h*w bytes), stream-ordered like
 *                                rcw_expand_columns. */
#define RCW_VIEW_OFF   0
#define RCW_VIEW_RGB8  1
#define RCW_VIEW_GRAY8 2
#define RCW_VIEW_DEPTH8 4  /* bit 2: a depth plane follows the colour planes */
#define RCW_VIEW_RGBD8  5  /* RCW_VIEW_RGB8 | RCW_VIEW_DEPTH8 */
#define RCW_VIEW_GRAYD8 6  /* RCW_VIEW_GRAY8 | RCW_VIEW_DEPTH8 */
#define RCW_VIEW_CHW   0
#define RCW_VIEW_HWC   1
#define RCW_VIEW_ONLY  1   /* flag: no camera view in the step */
#define RCW_VIEW_MAX_FRAMES 16
RCW_API int rcw_set_learner_view(rcw_handle* h, int32_t format, int32_t layout, int32_t height, int32_t width, int32_t flags);
RCW_API int rcw_set_learner_view_stack(rcw_handle* h, int32_t format, int32_t layout, int32_t height, int32_t width, int32_t flags,
                                       int32_t frames);
RCW_API int rcw_learner_view_stack(rcw_handle* h, int32_t* frames);
RCW_API int rcw_learner_view_info(rcw_handle* h, int32_t* format, int32_t* layout, int32_t* height, int32_t* width,
                                  int32_t* flags);
RCW_API int rcw_learner_view_device_ptr(rcw_handle* h, void** device_ptr);
RCW_API int rcw_learner_view_copy(rcw_handle* h, uint8_t* out_host, int32_t first, int32_t count);
RCW_API int rcw_expand_columns_view(rcw_handle* h, const int32_t* height_line_pu_device, const uint8_t* colour_id_device,
                                    int32_t count, void* view_device);

/* ---- multi-GPU: the observation gather north_star names, for a host without torch (Julia) ---------------
 * Agents shard by rank (cfg.agent_id_offset); stepping needs no communication.  The only exchange is the
 * optional all-gather of the observation batch over RCCL (xGMI inside a node).  librccl is loaded at run time
 * (dlopen of librccl.so.1 — the copy already in the process if there is one) the first time a comm call is
 * made, so single-GPU users do not need it.
 *   rcw_comm_unique_id   ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to the other ranks
 *                        (a file, a socket, MPI, Julia's Distributed — the transport is the caller's).
 *   rcw_comm_init        ncclCommInitRank on the handle's device; collective over all `world` ranks.
 *   rcw_gather_columns   ncclAllGather of the compact descriptors (5 bytes per column) on the handle's stream:
 *                        height_line_pu Int32 (N, B*world) and colour id UInt8 (N, B*world) in DEVICE memory,
 *                        rank r's agents at [r*B, (r+1)*B).
 *   rcw_gather_observations   the GLOBAL observation batch UInt32 (H_cam, N, B*world) in caller-owned DEVICE
 *                        memory on every rank.  RCW_GATHER_COLUMNS: gather descriptors, expand to pixels locally
 *                        (rcw_expand_columns) — 5 bytes per column over the links instead of 4*H_cam;
 *                        RCW_GATHER_FRAMES: ncclAllGather of the pixels themselves.
 * All of them are stream-ordered behind the step that produced the frames and return without waiting. */
#define RCW_UNIQUE_ID_BYTES 128
#define RCW_GATHER_COLUMNS 0
#define RCW_GATHER_FRAMES  1
RCW_API int rcw_comm_unique_id(void* out_id /* RCW_UNIQUE_ID_BYTES */);
RCW_API int rcw_comm_init(rcw_handle* h, const void* unique_id, int32_t rank, int32_t world);
RCW_API int rcw_comm_destroy(rcw_handle* h);
RCW_API int rcw_comm_info(rcw_handle* h, int32_t* rank, int32_t* world /* 0, 0 before rcw_comm_init */);
RCW_API int rcw_gather_columns(rcw_handle* h, int32_t* height_line_pu_all_device, uint8_t* colour_id_all_device);
RCW_API int rcw_gather_observations(rcw_handle* h, int32_t mode, void* frames_all_device);

/* Device buffers for a host that has no GPU array package of its own (the gather outputs above, rcw_bind_obs,
 * rcw_expand_columns): plain hipMalloc / hipFree on the handle's device, and a copy to host memory that is
 * ordered behind the handle's stream (it waits for the work enqueued so far, then copies). */
RCW_API int rcw_device_malloc(rcw_handle* h, uint64_t bytes, void** device_ptr);
RCW_API int rcw_device_free(rcw_handle* h, void* device_ptr);
RCW_API int rcw_memcpy_to_host(rcw_handle* h, void* dst_host, const void* src_device, uint64_t bytes);

/* The (direction, ray) table the kernels use, for inspection and parity tests:
 * Float32 (N, 5, num_directions) = per direction [dx | dy | |1/dx| | |1/dy| | dir.ray]. */
RCW_API int rcw_ray_table(rcw_handle* h, float* out_host);
RCW_API int rcw_direction_table(rcw_handle* h, float* out_host /* (2, nd) */);

/* HIP-event timing on the handle's stream (what bench.py reads the kernel time from). */
RCW_API int rcw_timer_start(rcw_handle* h);
RCW_API int rcw_timer_stop(rcw_handle* h, float* elapsed_ms);

/* Per-kernel timing: while enabled, HIP events bracket the cast kernel, the top view kernel (when
 * cfg.render_top_view) and the fill kernel of each step (at most 256 steps are recorded).
 * rcw_profile_read returns their mean durations over the recorded steps (top_view_ms = 0 without it).
 * With the two-kernel top view (RCW_TOP_VIEW_TWO_KERNELS below) top_view_ms is its store kernel — the one that
 * writes the image; its drawing runs inside the camera fill's launch (or, at camera heights other than 256 rows, on a
 * side stream beside it): inside fill_ms.  Where the camera fill is the shorter of the two (big images) it is the FILL
 * that goes to the side stream: fill_ms then runs from the cast kernel's end to the fill's end beside the drawing, and
 * top_view_ms from there to the step's end; cast_ms + top_view_ms + fill_ms is the whole step in every case. */
RCW_API int rcw_profile(rcw_handle* h, int32_t enable);
RCW_API int rcw_profile_read(rcw_handle* h, float* cast_ms, float* top_view_ms, float* fill_ms, int32_t* steps);

/* Which form of update_top_view! (SR:446-483) the handle's geometry takes — all write the same pixels:
 *   RCW_TOP_VIEW_NONE         cfg.render_top_view = 0
 *   RCW_TOP_VIEW_IN_PLACE     tiles, then lines and circle drawn over them in HBM (images beyond the LDS bit planes)
 *   RCW_TOP_VIEW_ONE_KERNEL   write-once: bit planes in LDS, draw and store groups of one persistent kernel
 *   RCW_TOP_VIEW_TWO_KERNELS  write-once, inside rcw_step / rcw_reset / rcw_set_state: the drawing (bit planes -> HBM) in the
 *                             camera fill's own launch, then the moving-window store kernel; rcw_update_top_view alone
 *                             takes draw -> store back to back where that is the faster one (rcw_update_top_view_form).
 *                             Geometries: H*pu a multiple of 256 rows with pu_per_tu in {8, 16, ..., 256} and a player
 *                             circle of <= 32 rows (rcw_top_store_kernel), any pu_per_tu >= 9 with H*pu a multiple of 4
 *                             and >= 42 rows (rcw_top_store_flat_kernel), 8-pixel tiles with H*pu a multiple of 64 or 32
 *                             (rcw_top_store_units_kernel).  Taken at every batch size where the camera view is 256
 *                             rows high (one launch for fill + drawing); at other camera heights the drawing needs the
 *                             handle's side stream, and the form is taken from 256 MiB of top view a step (below that
 *                             the one-kernel form is faster) unless rcw_set_top_view_form asks for it */
enum { RCW_TOP_VIEW_NONE = 0, RCW_TOP_VIEW_IN_PLACE = 1, RCW_TOP_VIEW_ONE_KERNEL = 2, RCW_TOP_VIEW_TWO_KERNELS = 3 };
RCW_API int rcw_top_view_form(rcw_handle* h, int32_t* form);
/* ... and the form rcw_update_top_view takes when it is called ALONE (update_top_view!(env) outside a step, SR:446): nothing runs
 * beside the drawing then.  Where the step takes the two-kernel form the stand-alone call takes it too (draw -> store back to back)
 * for images from 256 x 256 px, for pixel scales that are no multiple of 4 and for tiles below 16 px — measured faster, round 5 —;
 * the one-kernel form keeps images below 256 x 256 px at 16, 20, 24, ... px a tile, and every geometry that is not the two-kernel
 * form's; RCW_TOP_VIEW_IN_PLACE where the bit planes do not fit in LDS. */
RCW_API int rcw_update_top_view_form(rcw_handle* h, int32_t* form);
/* Choose the form instead of the rule above (all forms write the same pixels; this is a performance choice, e.g. the
 * one-kernel form for a caller that does not want the handle's side stream, or the two-kernel form for a small batch):
 * form = 0 restores the automatic choice, else RCW_TOP_VIEW_IN_PLACE / ONE_KERNEL / TWO_KERNELS; RCW_ERR_UNSUPPORTED when
 * the geometry cannot take it (the handle then keeps the automatic choice).  runs = 0: automatic; 1..8: the two-kernel
 * form draws and stores the batch in that many runs of agents.  Waits for the handle's stream; reallocates the form's
 * scratch in HBM.  The library reads no environment variable other than RCW_RCCL_LIBRARY: what used to be development
 * switches (RCW_TOP_SPLIT, RCW_TOP_RUNS, ...) exists only in the development build (make dev -> librcw_hip_dev.so), whose knobs override
 * what the rules compute and select nothing this library cannot reach. */
RCW_API int rcw_set_top_view_form(rcw_handle* h, int32_t form, int32_t runs);
/* How many launches a step — RCW.act!(env, a) SR:333-340 — takes; both forms leave the same state and the same pixels:
 *   RCW_STEP_TWO_LAUNCHES  the cast kernel (dynamics SR:139-191, cast_rays! SR:195-231, the columns of update_camera_view!
 *                          SR:401-429 as compact descriptors), then the fill kernel (SR:431-440) — the reference's own order.
 *   RCW_STEP_ONE_LAUNCH    the frame of the NEXT step depends only on this step's state and the next action, and there are four
 *                          actions: the casting workgroups of a launch commit the dynamics and also cast the four successor states
 *                          (a blocked / goal / raising move keeps the current frame; an agent that is done under cfg.auto_reset gets
 *                          the re-sampled world's, drawn ahead without being committed) into slots in HBM (two buffers of 10 bytes a
 *                          view column), and the fill workgroups of the NEXT launch, in the same launch as that step's casting, write the
 *                          frames the actions select.  Nothing inside a launch waits for anything else in it; the cast kernel and a
 *                          launch boundary leave the step's critical path.  rcw_reset / rcw_set_state (and a first step) cast as a
 *                          launch of their own, which leaves the slots of the agents it touches ready.
 * The rule: one launch where the geometry allows — a camera view the moving-window fill kernels take (256 rows: every BASELINE configuration;
 * also 256 k, 128 and 64 rows, up to 8191) without a top view (cfg.render_top_view = 0), fewer than 2^29 view columns in the batch — AND the batch is large enough for it to pay: a casting
 * workgroup marches five fans one after the other, so the launch is no shorter than that, and below ~100-350 MiB of frames a step
 * (by map size and view columns: 512 agents at 8x8 / 256 columns, 400 at 32x32 / 1024 columns) the cast kernel followed by the fill
 * kernel is the faster step (rcw_set_step_form(RCW_STEP_ONE_LAUNCH) takes it at any batch).  A step captured into a HIP graph (hipStreamBeginCapture on
 * the handle's stream) takes the two-launch form, and so does every later step of that handle: the one-launch form alternates its
 * two buffers from launch to launch on the host, which a replayed graph cannot.  rcw_set_step_form: 0 = the rule,
 * RCW_STEP_ONE_LAUNCH fails with RCW_ERR_UNSUPPORTED where the geometry cannot take it. */
enum { RCW_STEP_TWO_LAUNCHES = 1, RCW_STEP_ONE_LAUNCH = 2 };
RCW_API int rcw_step_form(rcw_handle* h, int32_t* form);
RCW_API int rcw_set_step_form(rcw_handle* h, int32_t form);
/* The kernel update_camera_view! (SR:374-444) runs in INSIDE A STEP of this handle (what bench.py labels its roofline block
 * with): "rcw_fill256_kernel", "rcw_fill_window_kernel", "rcw_fill_flat_kernel", ... by camera height and batch — and
 * "rcw_fill256_draw_kernel" where the handle also renders the top view and the camera fill and the top view's drawing go in
 * one launch, and "rcw_fill256_cast_kernel" for the one-launch step (rcw_update_camera_view alone always takes the plain fill
 * kernel). */
RCW_API int rcw_fill_kernel_name(rcw_handle* h, char* buf, int32_t buflen);

/* Introspection */
RCW_API int rcw_batch(rcw_handle* h, int32_t* out);
RCW_API int rcw_get_config(rcw_handle* h, rcw_config* out);
RCW_API int rcw_device_name(rcw_handle* h, char* buf, int32_t buflen);
RCW_API const char* rcw_last_error(void);
RCW_API int rcw_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RCW_H */
