# BatchedSingleRoom.jl — the reference-side binding of librcw_hip (include/rcw.h, ABI version 4).
#
# This is what a RayCastWorlds.jl maintainer would add to keep the package's API
# (`RCW.reset!`, `RCW.act!`, `RCW.cast_rays!`, `RCW.update_camera_view!`, `RCW.update_top_view!`,
# `RCW.RLBaseEnv` with `state` / `reward` / `is_terminated`) while the SingleRoom step/render path runs on an
# MI355X for a whole batch of agents.  EVERY export of include/rcw.h is bound here; tests/test_julia_binding.py
# checks each `ccall` below against the prototypes in the header (name, arity, pointer/scalar kind, width).
#
# NOT EXECUTED IN THIS PIPELINE: neither the build container nor the GPU box has a Julia toolchain
# (SURVEY.md §0), so this file is written against the C ABI and checked mechanically; the same calls are
# exercised by the Python/ctypes host layer in raycastworlds.jl_amd/ and by tests/c_abi_harness.c.
#
# Usage (inside the RayCastWorlds module tree, next to single_room.jl):
#
#     include("BatchedSingleRoom.jl")
#     env = RCW.BatchedSingleRoomModule.BatchedSingleRoom(4096; height_tile_map_tu = 8,
#                                                         width_tile_map_tu = 8, num_rays = 256)
#     RCW.reset!(env)
#     RCW.act!(env, rand(UInt8(1):UInt8(4), 4096))
#     rl = RCW.RLBaseEnv(env)
#     obs = RLBase.state(rl)        # the SAME Array{UInt32,3}(H_cam, N, B) every call (SR:576), refreshed lazily
#     RLBase.reward(rl); RLBase.is_terminated(rl)
#
# Observations.  The reference returns `camera_view` itself from `RLBase.state` (single_room.jl:576): one array,
# mutated in place by the next `act!`.  Here the frames live in HBM.  `RLBase.state` returns one host mirror —
# the same `Array` object on every call — and copies the batch off the device only when a step / reset has made
# the mirror stale, so calling it repeatedly costs nothing.  A device-side consumer skips the copy altogether:
# `camera_view_device_ptr(env)` is stable for the handle's lifetime, e.g. with AMDGPU.jl
# `unsafe_wrap(ROCArray{UInt32,3}, Ptr{UInt32}(ptr), (H_cam, N, B))`.

module BatchedSingleRoomModule

import ..RayCastWorlds as RCW
import MiniFB as MFB
import ReinforcementLearningBase as RLBase

const librcw = get(ENV, "LIBRCW_HIP", "librcw_hip.so")

const RCW_ABI_VERSION = 4
const NUM_ACTIONS = 4   # src/single_room.jl:19
const RCW_UNIQUE_ID_BYTES = 128
const RCW_GATHER_COLUMNS = Int32(0)
const RCW_GATHER_FRAMES = Int32(1)
const RCW_VIEW_OFF = Int32(0)      # rcw_set_learner_view: format
const RCW_VIEW_RGB8 = Int32(1)
const RCW_VIEW_GRAY8 = Int32(2)
const RCW_VIEW_DEPTH8 = Int32(4)   # bit 2: a depth plane follows the colour planes
const RCW_VIEW_RGBD8 = Int32(5)
const RCW_VIEW_GRAYD8 = Int32(6)
const RCW_VIEW_CHW = Int32(0)      # ... layout (C order; Julia sees the axes reversed)
const RCW_VIEW_HWC = Int32(1)
const RCW_VIEW_ONLY = Int32(1)     # ... flag: steps skip the UInt32 camera view
# R of SingleRoom(; R = ...) single_room.jl:266  <->  rcw_config.reward_type
const REWARD_TYPES = (Float32, Float64, Int32, Int64)

# struct rcw_config (include/rcw.h) — field order and types must match exactly (160 bytes)
Base.@kwdef mutable struct RcwConfig
    abi_version::Int32 = RCW_ABI_VERSION
    height_tile_map_tu::Int32 = 8
    width_tile_map_tu::Int32 = 16
    num_directions::Int32 = 128
    num_rays::Int32 = 512
    height_camera_view_pu::Int32 = 256
    pu_per_tu::Int32 = 32
    player_radius_wu::Float32 = 1 / 8
    position_increment_wu::Float32 = 1 / 8
    semi_field_of_view_wu::Float32 = 2 / 3
    camera_height_tile_wu::Float32 = 1
    goal_reward::Float32 = 1
    floor_color::UInt32 = 0x00404040
    ceiling_color::UInt32 = 0x00FFFFFF
    wall_dim_1_color::UInt32 = 0x00808080
    wall_dim_2_color::UInt32 = 0x00c0c0c0
    goal_dim_1_color::UInt32 = 0x00800000
    goal_dim_2_color::UInt32 = 0x00c00000
    dda_tie_break::Int32 = 0
    dda_distance::Int32 = 0
    normalize_mode::Int32 = 0
    auto_reset::Int32 = 0
    agent_id_offset::Int64 = 0
    reward_type::Int32 = 0
    out_of_bounds::Int32 = 0
    render_top_view::Int32 = 0
    world_unit_bits::Int32 = 32
    player_radius_wu_f64::Float64 = 1 / 8
    position_increment_wu_f64::Float64 = 1 / 8
    semi_field_of_view_wu_f64::Float64 = 2 / 3
    camera_height_tile_wu_f64::Float64 = 1
    goal_reward_f64::Float64 = 1
    reserved::NTuple{2, Int32} = (0, 0)
end

struct RcwError <: Exception
    code::Cint
    msg::String
end

last_error() = unsafe_string(ccall((:rcw_last_error, librcw), Cstring, ()))
abi_version() = ccall((:rcw_abi_version, librcw), Cint, ())

function check(rc::Cint)
    rc == 0 && return nothing
    msg = last_error()
    rc == -2 && throw(AssertionError(msg))            # @assert action in 1:4, single_room.jl:140
    rc == -5 && throw(BoundsError())                   # collision_detection.jl:35
    rc == -1 && throw(ArgumentError(msg))
    rc == -4 && throw(OutOfMemoryError())
    throw(RcwError(rc, msg))
end

# The library's own defaults (the reference's kwargs, single_room.jl:258-272, 288-296): equals RcwConfig()
function config_default()
    cfg = RcwConfig()
    check(ccall((:rcw_config_default, librcw), Cint, (Ref{RcwConfig},), cfg))
    return cfg
end

mutable struct BatchedSingleRoom{T, R} <: RCW.AbstractGame
    handle::Ptr{Cvoid}
    batch::Int
    config::RcwConfig
    camera_view::Array{UInt32, 3}     # (H_cam, N, B) host mirror: THE array RLBase.state returns, every call
    stale::Bool                       # the mirror is older than the device frames
    seed::UInt64
    rng::Any                          # the reference's `rng` keyword (single_room.jl:49,265): nothing (resets are sampled on the
                                      # device, keyed by `seed`), an AbstractRNG, or a vector of them, one per agent
    gather_buffer::Ptr{Cvoid}         # device memory for gather_observations (allocated on first use)
    gather_frames::Int                # agents the gather buffer holds

    # SingleRoom(; T, R, kwargs...) single_room.jl:258-272 for `batch` agents on HIP device `device`
    function BatchedSingleRoom(batch::Integer; T::Type = Float32, R::Type = Float32, device::Integer = 0,
                               seed::Integer = 0, rng = nothing, kwargs...)
        T in (Float32, Float64) || throw(ArgumentError("T must be Float32 or Float64"))
        R in REWARD_TYPES || throw(ArgumentError("R must be one of $(REWARD_TYPES)"))
        cfg = RcwConfig(; kwargs...)
        # convert(T, .) of the caller's world-unit parameters (single_room.jl:263-270): for T = Float64 the library
        # reads the *_f64 fields — the Float64 value itself, not the Float32 one widened
        for name in (:player_radius_wu, :position_increment_wu, :semi_field_of_view_wu, :camera_height_tile_wu)
            haskey(kwargs, name) && setfield!(cfg, Symbol(name, :_f64), Float64(kwargs[name]))
        end
        cfg.world_unit_bits = T === Float64 ? 64 : 32
        cfg.reward_type = Int32(findfirst(==(R), REWARD_TYPES) - 1)
        cfg.goal_reward = one(Float32); cfg.goal_reward_f64 = 1.0      # one(R) single_room.jl:82
        handle = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:rcw_create, librcw), Cint, (Ref{RcwConfig}, Int32, Int32, UInt64, Ref{Ptr{Cvoid}}),
                    cfg, batch, device, seed, handle))
        view = Array{UInt32, 3}(undef, cfg.height_camera_view_pu, cfg.num_rays, batch)
        env = new{T, R}(handle[], batch, cfg, view, true, seed, rng, C_NULL, 0)
        finalizer(destroy!, env)
        # the reference's constructor consumes its rng twice: the draws of single_room.jl:62-74, then reset!(world) :105
        rng === nothing || reset_from_rng!(env, rng; construction = true)
        return env
    end
end

function destroy!(env::BatchedSingleRoom)
    env.handle == C_NULL && return nothing
    env.gather_buffer != C_NULL && ccall((:rcw_device_free, librcw), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), env.handle, env.gather_buffer)
    ccall((:rcw_destroy, librcw), Cint, (Ptr{Cvoid},), env.handle)
    env.handle = C_NULL
    env.gather_buffer = C_NULL
    return nothing
end

#####
##### the generic functions of RayCastWorlds.jl:7-14 on the path
#####

# reset!(world) single_room.jl:110-137 with the CALLER's generator — the reference's `rng` keyword (single_room.jl:49,265).
# The draws are made on the host by the reference's own statements, in its order: `rand(rng, 2:H-1)`, `rand(rng, 2:W-1)`
# (:120), `RCW.sample_empty_position(rng, tile_map)` (:124 — the package's own function on a host tile map with the wall ring
# and the new goal, utils.jl:23-58), `rand(rng, 0:nd-1)` (:128) — agent after agent from one generator (B reference worlds
# sharing it, reset in order), or agent a from `rng[a]` (each agent IS the reference world built with that generator: its
# stream is the reference's, draw for draw).  The state goes to the engine with one rcw_set_state.
function reset_from_rng!(env::BatchedSingleRoom{T}, rng; mask::Union{Nothing, Vector{UInt8}} = nothing,
                         construction::Bool = false) where {T}
    H, W, nd, B = Int(env.config.height_tile_map_tu), Int(env.config.width_tile_map_tu), Int(env.config.num_directions), env.batch
    rng isa AbstractVector && length(rng) != B && throw(DimensionMismatch("expected one generator or $(B) of them"))
    goal = fill(Int32(2), 2, B); position = fill(T(1.5), 2, B); direction = zeros(Int32, B)
    tile_map = falses(2, H, W)                                                   # NUM_OBJECTS = 2, WALL = 1, GOAL = 2 (:16-18)
    tile_map[1, :, 1] .= true; tile_map[1, :, W] .= true; tile_map[1, 1, :] .= true; tile_map[1, H, :] .= true   # :57-60
    for a in 1:B
        (mask !== nothing && mask[a] == 0) && continue
        g = rng isa AbstractVector ? rng[a] : rng
        for pass in (construction ? (1, 2) : (2,))                              # (the constructor's own draws :62-74 come first)
            goal_position = CartesianIndex(rand(g, 2 : H - 1), rand(g, 2 : W - 1))                    # :62 / :120
            tile_map[2, goal_position] = true                                                         # :63 / :122
            player_position_tu = RCW.sample_empty_position(g, tile_map)                               # :71 / :124
            player_direction_au = rand(g, 0 : nd - 1)                                                 # :74 / :128
            tile_map[2, goal_position] = false                                                        # (:118 of the next reset!)
            goal[1, a] = goal_position[1]; goal[2, a] = goal_position[2]
            position[1, a] = convert(T, player_position_tu[1] - 0.5); position[2, a] = convert(T, player_position_tu[2] - 0.5)   # :125
            direction[a] = player_direction_au
        end
    end
    set_state!(env, goal, position, direction; mask = mask)
    return nothing
end

# RCW.reset!(env)  — single_room.jl:326-331 (all agents, or those whose mask byte is non-zero).  With `rng` (or an
# environment built with one): the caller's generator, as the reference; else sampled on the device, keyed by `seed`.
function RCW.reset!(env::BatchedSingleRoom; mask::Union{Nothing, Vector{UInt8}} = nothing, rng = env.rng,
                    seed::Union{Nothing, Integer} = nothing)
    if rng !== nothing && seed === nothing
        return reset_from_rng!(env, rng; mask = mask)
    end
    env.seed = seed === nothing ? env.seed : seed
    GC.@preserve mask check(ccall((:rcw_reset, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, UInt64),
                                  env.handle, mask === nothing ? Ptr{UInt8}(C_NULL) : pointer(mask), env.seed))
    env.stale = true
    return nothing
end

# ---- wall layouts (this build's addition; include/rcw.h, rcw_set_walls) ------------------------------------------------------
"""
    set_walls!(env, walls; index = nothing, mask = nothing)

Interior walls.  `walls` is `Bool` / `UInt8` `(H, W)` — one layout for every agent — or `(H, W, M)`, `walls[i, j, m]` = tile `(i, j)`
of layout `m` is a wall, the index order of `world.tile_map[WALL, i, j]`.  `index` (`Vector{<:Integer}`, 1-based, one entry an agent)
names each agent's layout; `nothing` needs `M == 1` or `M == batch` (agent `a` takes layout `a`).  `mask`: the agents the call touches.
The wall ring must be there and two interior tiles free.  The touched agents are reset against the new walls with the environment's
seed (an environment built with `rng` follows with `reset!(env; mask)` itself, whose host draws do not know the walls), and the walls
stay through every later `reset!`, `set_state!` and `auto_reset` restart until the next call.
"""
function set_walls!(env::BatchedSingleRoom, walls::AbstractArray; index::Union{Nothing, AbstractVector{<:Integer}} = nothing,
                    mask::Union{Nothing, Vector{UInt8}} = nothing)
    H, W = Int(env.config.height_tile_map_tu), Int(env.config.width_tile_map_tu)
    (ndims(walls) in (2, 3) && size(walls, 1) == H && size(walls, 2) == W) || throw(DimensionMismatch("walls must be ($H, $W) or ($H, $W, M)"))
    flat = Vector{UInt8}(vec(walls .!= 0))                                       # column-major: m H W + (i - 1) + H (j - 1)
    layouts = ndims(walls) == 2 ? 1 : size(walls, 3)
    index0 = index === nothing ? nothing : Vector{Int32}(index .- 1)
    index0 === nothing || length(index0) == env.batch || throw(DimensionMismatch("expected $(env.batch) layout indices"))
    mask === nothing || length(mask) == env.batch || throw(DimensionMismatch("expected $(env.batch) mask bytes"))
    GC.@preserve flat index0 mask check(ccall((:rcw_set_walls, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Ptr{Int32}, Ptr{UInt8}),
                                              env.handle, pointer(flat), layouts,
                                              index0 === nothing ? Ptr{Int32}(C_NULL) : pointer(index0),
                                              mask === nothing ? Ptr{UInt8}(C_NULL) : pointer(mask)))
    env.stale = true
    return nothing
end

# RCW.act!(env, action)  — single_room.jl:333-340; one action per agent (or one for all)
function RCW.act!(env::BatchedSingleRoom, actions::Vector{UInt8})
    length(actions) == env.batch || throw(DimensionMismatch("expected $(env.batch) actions"))
    check(ccall((:rcw_step, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}), env.handle, actions))
    env.stale = true
    return nothing
end
RCW.act!(env::BatchedSingleRoom, action::Integer) = RCW.act!(env, fill(UInt8(action), env.batch))

# The same with actions already in device memory (a policy that runs on the GPU): stream-ordered, no host round trip
function act_device!(env::BatchedSingleRoom, actions_device::Ptr{UInt8})
    check(ccall((:rcw_step_device, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}), env.handle, actions_device))
    env.stale = true
    return nothing
end

RCW.get_action_keys(env::BatchedSingleRoom) = (MFB.KB_KEY_W, MFB.KB_KEY_S, MFB.KB_KEY_A, MFB.KB_KEY_D)   # single_room.jl:485
RCW.get_action_names(env::BatchedSingleRoom) = (:MOVE_FORWARD, :MOVE_BACKWARD, :TURN_LEFT, :TURN_RIGHT)   # single_room.jl:486

# RCW.cast_rays!(world) single_room.jl:195-231, RCW.update_camera_view!(env) :374-444, RCW.update_top_view!(env) :446-483
function RCW.cast_rays!(env::BatchedSingleRoom)
    check(ccall((:rcw_cast_rays, librcw), Cint, (Ptr{Cvoid},), env.handle))
    return nothing
end
function RCW.update_camera_view!(env::BatchedSingleRoom)
    check(ccall((:rcw_update_camera_view, librcw), Cint, (Ptr{Cvoid},), env.handle))
    env.stale = true
    return nothing
end
function RCW.update_top_view!(env::BatchedSingleRoom)
    check(ccall((:rcw_update_top_view, librcw), Cint, (Ptr{Cvoid},), env.handle))
    return nothing
end

sync(env::BatchedSingleRoom) = check(ccall((:rcw_sync, librcw), Cint, (Ptr{Cvoid},), env.handle))
clear_error!(env::BatchedSingleRoom) = check(ccall((:rcw_clear_error, librcw), Cint, (Ptr{Cvoid},), env.handle))

# Inject the state reset!(world) would have produced (single_room.jl:118-132) — how "identical
# seeds" is realised against the CPU reference (SURVEY.md §8c).
function set_state!(env::BatchedSingleRoom{Float32}, goal_ij::Matrix{Int32}, position_wu::Matrix{Float32},
                    direction_au::Vector{Int32}; mask::Union{Nothing, Vector{UInt8}} = nothing)
    GC.@preserve mask check(ccall((:rcw_set_state, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Ptr{UInt8}),
                                  env.handle, goal_ij, position_wu, direction_au,
                                  mask === nothing ? Ptr{UInt8}(C_NULL) : pointer(mask)))
    env.stale = true
    return nothing
end
function set_state!(env::BatchedSingleRoom{Float64}, goal_ij::Matrix{Int32}, position_wu::Matrix{Float64},
                    direction_au::Vector{Int32}; mask::Union{Nothing, Vector{UInt8}} = nothing)
    GC.@preserve mask check(ccall((:rcw_set_state64, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{UInt8}),
                                  env.handle, goal_ij, position_wu, direction_au,
                                  mask === nothing ? Ptr{UInt8}(C_NULL) : pointer(mask)))
    env.stale = true
    return nothing
end

# Julia's own directions_wu (single_room.jl:65-69: Julia's cos / sin) instead of the C library's
function set_direction_table!(env::BatchedSingleRoom{Float32}, directions_wu::Matrix{Float32})
    check(ccall((:rcw_set_direction_table, librcw), Cint, (Ptr{Cvoid}, Ptr{Float32}), env.handle, directions_wu))
    env.stale = true
end
function set_direction_table!(env::BatchedSingleRoom{Float64}, directions_wu::Matrix{Float64})
    check(ccall((:rcw_set_direction_table64, librcw), Cint, (Ptr{Cvoid}, Ptr{Float64}), env.handle, directions_wu))
    env.stale = true
end
function julia_direction_table(::Type{T}, num_directions) where {T}
    out = Matrix{T}(undef, 2, num_directions)
    for i in 1:num_directions
        theta_wu = (i - 1) * 2 * pi / num_directions                     # single_room.jl:66
        out[1, i] = convert(T, cos(theta_wu)); out[2, i] = convert(T, sin(theta_wu))
    end
    return out
end

#####
##### world fields (single_room.jl:21-40)
#####

function reward(env::BatchedSingleRoom{T, R}) where {T, R}
    out = Vector{R}(undef, env.batch)
    check(ccall((:rcw_reward_typed, librcw), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), env.handle, out)); out
end
function reward_float32(env::BatchedSingleRoom{T, Float32}) where {T}
    out = Vector{Float32}(undef, env.batch)
    check(ccall((:rcw_reward, librcw), Cint, (Ptr{Cvoid}, Ptr{Float32}), env.handle, out)); out
end
function done(env::BatchedSingleRoom)
    out = Vector{UInt8}(undef, env.batch)
    check(ccall((:rcw_done, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}), env.handle, out)); out .!= 0
end
function player_position_wu(env::BatchedSingleRoom{Float32})
    out = Matrix{Float32}(undef, 2, env.batch)
    check(ccall((:rcw_position, librcw), Cint, (Ptr{Cvoid}, Ptr{Float32}), env.handle, out)); out
end
function player_position_wu(env::BatchedSingleRoom{Float64})
    out = Matrix{Float64}(undef, 2, env.batch)
    check(ccall((:rcw_position64, librcw), Cint, (Ptr{Cvoid}, Ptr{Float64}), env.handle, out)); out
end
function player_direction_au(env::BatchedSingleRoom)
    out = Vector{Int32}(undef, env.batch)
    check(ccall((:rcw_direction, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}), env.handle, out)); out
end
function goal_position(env::BatchedSingleRoom)
    out = Matrix{Int32}(undef, 2, env.batch)
    check(ccall((:rcw_goal, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}), env.handle, out))
    return [CartesianIndex(Int(out[1, b]), Int(out[2, b])) for b in 1:env.batch]
end
function episode(env::BatchedSingleRoom)
    out = Vector{UInt32}(undef, env.batch)
    check(ccall((:rcw_episode, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt32}), env.handle, out)); out
end
# ---- the episode time limit (this build's addition; include/rcw.h, rcw_set_time_limit) ----------------------------------------
"""
    set_time_limit!(env, max_episode_steps)

An episode ends after `max_episode_steps` calls of `act!` without the goal: that step sets `truncated`, and with `auto_reset`
the next action restarts the agent as it restarts a done one.  `0` switches the limit off (the default, the reference's
behaviour).  Decided on the device; every call zeroes `episode_steps` and `truncated` of every agent.
"""
function set_time_limit!(env::BatchedSingleRoom, max_episode_steps::Integer)
    check(ccall((:rcw_set_time_limit, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, max_episode_steps))
    return nothing
end
function time_limit(env::BatchedSingleRoom)
    n = Ref{Int32}(0)
    check(ccall((:rcw_time_limit, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, n)); Int(n[])
end
function episode_steps(env::BatchedSingleRoom)
    out = Vector{UInt32}(undef, env.batch)
    check(ccall((:rcw_episode_steps, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt32}), env.handle, out)); out
end
function truncated(env::BatchedSingleRoom)
    out = Vector{UInt8}(undef, env.batch)
    check(ccall((:rcw_truncated, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}), env.handle, out)); out .!= 0
end
function episode_steps_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_episode_steps_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function truncated_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_truncated_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
# (no RLBase verb in the reference; the device form mirrors is_terminated_device)
is_truncated(env::RCW.RLBaseEnv{E}) where {E <: BatchedSingleRoom} = truncated(env.env)
is_truncated_device(env::BatchedSingleRoom) = (ptr = truncated_device_ptr(env), eltype = UInt8, dims = (env.batch,))
# ---- the goal distance (this build's addition; include/rcw.h, rcw_set_goal_distance) -------------------------------------------
"""
    set_goal_distance!(env, on = true)

Keep every agent's shortest-path distance to its goal (breadth-first through its walls, in tiles) on the device, behind every
`act!`, `reset!`, `set_state!` and `set_walls!`: `goal_distance(env)` returns `(distance, start_distance, progress)`, each
`Vector{Int32}` of `batch` (`-1`: no path); `goal_distance_field(env)` the `UInt16` fields as `(H, W, batch)`, `0xFFFF` for
walls and tiles without a path.  Shaping is `reward .+ c .* progress`.
"""
function set_goal_distance!(env::BatchedSingleRoom, on::Bool = true)
    check(ccall((:rcw_set_goal_distance, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, on ? 1 : 0))
    return nothing
end
function goal_distance_enabled(env::BatchedSingleRoom)
    n = Ref{Int32}(0)
    check(ccall((:rcw_goal_distance_enabled, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, n)); n[] != 0
end
function goal_distance(env::BatchedSingleRoom)
    d, s, p = (Vector{Int32}(undef, env.batch) for _ in 1:3)
    check(ccall((:rcw_goal_distance, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}), env.handle, d, s, p))
    return (distance = d, start_distance = s, progress = p)
end
function goal_distance_device_ptr(env::BatchedSingleRoom)
    d, s, p = (Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:3)
    check(ccall((:rcw_goal_distance_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                env.handle, d, s, p))
    return (distance = d[], start_distance = s[], progress = p[])
end
function goal_distance_field(env::BatchedSingleRoom, first::Integer = 0, count::Integer = env.batch - first)
    out = Array{UInt16, 3}(undef, env.config.height_tile_map_tu, env.config.width_tile_map_tu, count)
    check(ccall((:rcw_goal_distance_field, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}), env.handle, first, count, out)); out
end
function goal_distance_field_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_goal_distance_field_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end

# ---- the start rule (this build's addition; include/rcw.h, rcw_set_start_distance) -----------------------------------------------
const START_DISTANCE_MAX = Int32(65534)
"""
    set_start_distance!(env, lo = 1, hi = nothing)
    set_start_distance!(env, nothing)

Place the player of every episode that starts from now on — `reset!`, a done or truncated restart under `auto_reset`, a layout source's
restart, `set_walls!` — on a tile whose shortest-path distance to the goal lies in `lo:hi` (`hi = nothing`: no upper bound), on the device.
Where the band lies beyond what the goal's region holds the farthest tiles are taken.  No agent moves when it is switched on; calling it
again only changes the band, without a wait.  `start_placed(env)` is a `Vector{UInt8}` of `batch`: 0 no start yet, 1 in the band, 2 clamped,
3 the drawn pose kept.  `start_rule` is the rule for one agent on the host, without a device.
"""
function set_start_distance!(env::BatchedSingleRoom, lo::Integer = 1, hi::Union{Integer, Nothing} = nothing)
    check(ccall((:rcw_set_start_distance, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Int32), env.handle, 1, lo, hi === nothing ? START_DISTANCE_MAX : hi))
    return nothing
end
function set_start_distance!(env::BatchedSingleRoom, ::Nothing)
    check(ccall((:rcw_set_start_distance, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Int32), env.handle, 0, 0, 0))
    return nothing
end
function start_distance_info(env::BatchedSingleRoom)
    e = Ref{Int32}(0); lo = Ref{Int32}(0); hi = Ref{Int32}(0)
    check(ccall((:rcw_start_distance_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), env.handle, e, lo, hi))
    return (enabled = e[] != 0, lo = lo[], hi = hi[])
end
function start_placed(env::BatchedSingleRoom)
    p = Vector{UInt8}(undef, env.batch)
    check(ccall((:rcw_start_distance, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}), env.handle, p))
    return p
end
function start_placed_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_start_distance_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p))
    return p[]
end
"""
    start_rule(walls, goal, key, lo = 1, hi = nothing) -> (tile, outcome)

The start rule for one agent: `walls` a `Matrix{UInt8}` `(H, W)`, non-zero = wall; `goal` its 1-based `(i, j)`; `key` the episode key.
`tile` is the 1-based `(i, j)` the player is placed on, `nothing` where the drawn pose is kept (`outcome == 3`).
"""
function start_rule(walls::Matrix{UInt8}, goal, key::Integer, lo::Integer = 1, hi::Union{Integer, Nothing} = nothing)
    t = Ref{Int32}(0); o = Ref{Int32}(0)
    H = size(walls, 1)
    check(ccall((:rcw_start_rule, librcw), Cint, (Ptr{UInt8}, Int32, Int32, Int32, Int32, UInt64, Int32, Int32, Ref{Int32}, Ref{Int32}),
                walls, H, size(walls, 2), goal[1], goal[2], key % UInt64, lo, hi === nothing ? START_DISTANCE_MAX : hi, t, o))
    return (tile = t[] < 0 ? nothing : (t[] % H + 1, t[] ÷ H + 1), outcome = o[])
end

# ---- the guide (this build's addition; include/rcw.h, rcw_set_guide) -------------------------------------------------------------
"""
    set_guide!(env, on = true)

Keep, on the device, the action that follows every agent's shortest path to its goal, behind every call that moves an agent, a goal or
a wall, a new direction table and a `snapshot_restore!`: `guide(env)` returns `(action, heading)` — `action` a `Vector{UInt8}` of
`batch`, always in 1..4 (what `act!` takes), `heading` a `Vector{Int32}`, the 0-based direction index the guide wants the agent to face,
`-1` where it has no advice.  Needs the goal distance (`set_goal_distance!` first; switching that off switches the guide off too).
`guide_info(env)` says whether it is on and whether `position_increment + player_radius <= 0.5`, for which following it is promised to
arrive.  `guide_rule` is the rule for one agent on the host, without a device.
"""
function set_guide!(env::BatchedSingleRoom, on::Bool = true)
    check(ccall((:rcw_set_guide, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, on ? 1 : 0))
    return nothing
end
function guide_info(env::BatchedSingleRoom)
    e = Ref{Int32}(0); p = Ref{Int32}(0)
    check(ccall((:rcw_guide_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), env.handle, e, p))
    return (enabled = e[] != 0, promised = p[] != 0)
end
function guide(env::BatchedSingleRoom)
    a = Vector{UInt8}(undef, env.batch); h = Vector{Int32}(undef, env.batch)
    check(ccall((:rcw_guide, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int32}), env.handle, a, h))
    return (action = a, heading = h)
end
function guide_device_ptr(env::BatchedSingleRoom)
    a = Ref{Ptr{Cvoid}}(C_NULL); h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_guide_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}), env.handle, a, h))
    return (action = a[], heading = h[])
end
"""
    guide_rule(field, position, direction, directions_wu, position_increment) -> (action, heading)

The guide's rule for one agent: `field` a `Matrix{UInt16}` `(H, W)` (one agent's `goal_distance_field`), `position` `(x, y)`,
`direction` the 0-based heading, `directions_wu` a `(2, nd)` matrix of `Float32` or `Float64` — the type the rule computes in.
"""
function guide_rule(field::Matrix{UInt16}, position, direction::Integer, directions_wu::Matrix{T}, position_increment::Real) where {T <: Union{Float32, Float64}}
    a = Ref{UInt8}(0); h = Ref{Int32}(0)
    check(ccall((:rcw_guide_rule, librcw), Cint,
                (Int32, Int32, Ptr{Cvoid}, Float64, Float64, Int32, Int32, Int32, Ptr{Cvoid}, Float64, Ref{UInt8}, Ref{Int32}),
                size(field, 1), size(field, 2), field, position[1], position[2], 8 * sizeof(T), direction, size(directions_wu, 2),
                directions_wu, position_increment, a, h))
    return (action = a[], heading = h[])
end

# ---- the seen map (this build's addition; include/rcw.h, rcw_set_seen_map) ------------------------------------------------------
"""
    set_seen_map!(env, on = true)

Keep, on the device, the tiles each agent's view rays have crossed since its episode began, behind every `act!`, `reset!`,
`set_state!` and `set_walls!`: `seen_words(env)` returns `(seen_count, newly_seen, goal_seen)`, each `Vector{Int32}` of `batch`;
`seen_map(env)` the `UInt8` maps as `(H, W, batch)`: `0` not seen, else `1` free, `2` wall, `3` goal.  A coverage bonus is
`c .* newly_seen`.
"""
function set_seen_map!(env::BatchedSingleRoom, on::Bool = true)
    check(ccall((:rcw_set_seen_map, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, on ? 1 : 0))
    return nothing
end
function seen_map_enabled(env::BatchedSingleRoom)
    n = Ref{Int32}(0)
    check(ccall((:rcw_seen_map_enabled, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, n)); n[] != 0
end
function seen_words(env::BatchedSingleRoom)
    c, n, g = (Vector{Int32}(undef, env.batch) for _ in 1:3)
    check(ccall((:rcw_seen_words, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}), env.handle, c, n, g))
    return (seen_count = c, newly_seen = n, goal_seen = g)
end
function seen_words_device_ptr(env::BatchedSingleRoom)
    c, n, g = (Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:3)
    check(ccall((:rcw_seen_words_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                env.handle, c, n, g))
    return (seen_count = c[], newly_seen = n[], goal_seen = g[])
end
function seen_map(env::BatchedSingleRoom, first::Integer = 0, count::Integer = env.batch - first)
    out = Array{UInt8, 3}(undef, env.config.height_tile_map_tu, env.config.width_tile_map_tu, count)
    check(ccall((:rcw_seen_map, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}), env.handle, first, count, out)); out
end
function seen_map_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_seen_map_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end

# ---- the frontier (this build's addition; include/rcw.h, rcw_set_frontier) ------------------------------------------------------
"""
    set_frontier!(env, on = true)

Keep, on the device, each agent's way to the nearest unseen tile, directly behind the seen map (`set_seen_map!` first; `set_seen_map!(env,
false)` is refused while the frontier is on): `frontier(env)` returns `(distance, tiles, action, heading)` — `distance` a `Vector{Int32}`
of `batch`, the moves to the nearest frontier tile, `-1` where nothing is left to explore from the agent's tile; `tiles` how many frontier
tiles its last flood found; `action` a `Vector{UInt8}`, always in 1..4 (what `act!` takes); `heading` the 0-based direction index to
face, `-1` where there is no advice.  `frontier_field(env)` is the `UInt16` field as `(H, W, batch)`: `0` on the unseen tiles next to a
seen free one, on a seen free tile the moves to the nearest of them, `0xFFFF` elsewhere.  `frontier_rule` is the flood for one agent on
the host, without a device.
"""
function set_frontier!(env::BatchedSingleRoom, on::Bool = true)
    check(ccall((:rcw_set_frontier, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, on ? 1 : 0))
    return nothing
end
function frontier_info(env::BatchedSingleRoom)
    e = Ref{Int32}(0)
    check(ccall((:rcw_frontier_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, e))
    return (enabled = e[] != 0,)
end
function frontier(env::BatchedSingleRoom)
    d = Vector{Int32}(undef, env.batch); t = Vector{Int32}(undef, env.batch)
    a = Vector{UInt8}(undef, env.batch); h = Vector{Int32}(undef, env.batch)
    check(ccall((:rcw_frontier, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}), env.handle, d, t, a, h))
    return (distance = d, tiles = t, action = a, heading = h)
end
function frontier_device_ptr(env::BatchedSingleRoom)
    d, t, a, h = (Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:4)
    check(ccall((:rcw_frontier_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                env.handle, d, t, a, h))
    return (distance = d[], tiles = t[], action = a[], heading = h[])
end
function frontier_field(env::BatchedSingleRoom, first::Integer = 0, count::Integer = env.batch - first)
    out = Array{UInt16, 3}(undef, env.config.height_tile_map_tu, env.config.width_tile_map_tu, count)
    check(ccall((:rcw_frontier_field, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}), env.handle, first, count, out)); out
end
function frontier_field_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_frontier_field_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
"""
    frontier_rule(seen_map) -> (field, tiles)

The frontier's flood for one agent: `seen_map` a `Matrix{UInt8}` `(H, W)` (one agent's `seen_map`), `field` a `Matrix{UInt16}` `(H, W)`.
"""
function frontier_rule(seen_map::Matrix{UInt8})
    field = Matrix{UInt16}(undef, size(seen_map)...); n = Ref{Int32}(0)
    check(ccall((:rcw_frontier_rule, librcw), Cint, (Int32, Int32, Ptr{UInt8}, Ptr{Cvoid}, Ref{Int32}),
                size(seen_map, 1), size(seen_map, 2), seen_map, field, n))
    return (field = field, tiles = n[])
end

# ---- the local map (this build's addition; include/rcw.h, rcw_set_local_map) ----------------------------------------------------
const LOCAL_MAP_SOURCES = (off = Int32(0), world = Int32(1), seen = Int32(2))
"""
    set_local_map!(env, size; cells_per_tile = 1, source = :world)

Keep, on the device, an agent-centred, heading-up crop of each agent's map, behind every `act!`, `reset!`, `set_state!`, `set_walls!`
and `set_direction_table!`: `local_map(env)` is `UInt8`, C row-major `(batch, size, size)` — in Julia's order `(size, size, batch)` with
the image's COLUMN first —, row 1 the farthest ahead, `cells_per_tile` cells to a tile; `0` outside the map (`:seen`: or not seen), else
`1` free, `2` wall, `3` goal.  `source = :seen` crops the seen map (`set_seen_map!` first).  `size = 0` switches it off.
"""
function set_local_map!(env::BatchedSingleRoom, size::Integer; cells_per_tile::Integer = 1, source::Symbol = :world)
    src = size == 0 ? LOCAL_MAP_SOURCES.off : getfield(LOCAL_MAP_SOURCES, source)
    check(ccall((:rcw_set_local_map, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Int32), env.handle, src, size, size == 0 ? 0 : cells_per_tile))
    return nothing
end
function local_map_info(env::BatchedSingleRoom)
    s = Ref{Int32}(0); n = Ref{Int32}(0); r = Ref{Int32}(0)
    check(ccall((:rcw_local_map_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), env.handle, s, n, r))
    return (source = s[], size = n[], cells_per_tile = r[])
end
function local_map_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_local_map_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function local_map(env::BatchedSingleRoom; first::Integer = 0, count::Integer = env.batch - first)
    n = Int(local_map_info(env).size)
    out = Array{UInt8, 3}(undef, n, n, count)
    check(ccall((:rcw_local_map_copy, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32), env.handle, out, first, count)); out
end

# ---- episode statistics (this build's addition; include/rcw.h, rcw_set_episode_stats) -------------------------------------------
const EPISODE_OPEN, EPISODE_SUCCESS, EPISODE_TRUNCATED = UInt8(0), UInt8(1), UInt8(2)
const EPISODE_STATS_COLUMNS = (:episodes, :successes, :truncations, :sum_length, :sum_moves, :spl_episodes, :sum_spl_q16)
"""
    set_episode_stats!(env, on = true)

Keep, on the device, how each agent's episodes end and their sums over the batch and per level of the layout source that is live NOW
(enable `set_wall_bank!` or a generator family — and `set_goal_distance!`, for SPL — first: while the statistics are on the layout source
cannot be changed).  `episode_stats(env)` returns `(finished, outcome, length, moves, level, spl_q16, episodes)`, each a vector of
`batch`; `episode_stats_table(env)` the `UInt64` table `(8, 1 + rows)`, column 1 the totals and column `1 + k` level `first + k - 1`,
its rows `EPISODE_STATS_COLUMNS` and a reserved zero; `episode_stats_clear!(env)` zeroes the table without waiting for the stream.
"""
function set_episode_stats!(env::BatchedSingleRoom, on::Bool = true)
    check(ccall((:rcw_set_episode_stats, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, on ? 1 : 0))
    return nothing
end
function episode_stats_info(env::BatchedSingleRoom)
    e = Ref{Int32}(0); r = Ref{Int32}(0); f = Ref{Int32}(0)
    check(ccall((:rcw_episode_stats_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), env.handle, e, r, f))
    return (enabled = e[] != 0, rows = r[], first = f[])
end
function episode_stats(env::BatchedSingleRoom)
    B = env.batch
    fin = Vector{UInt8}(undef, B); out = Vector{UInt8}(undef, B); len = Vector{UInt32}(undef, B); mov = Vector{UInt32}(undef, B)
    lev = Vector{Int32}(undef, B); spl = Vector{Int32}(undef, B); eps = Vector{UInt32}(undef, B)
    check(ccall((:rcw_episode_stats, librcw), Cint,
                (Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt8}, Ptr{UInt32}, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt32}),
                env.handle, fin, out, len, mov, lev, spl, eps))
    return (finished = fin, outcome = out, length = len, moves = mov, level = lev, spl_q16 = spl, episodes = eps)
end
function episode_stats_device_ptr(env::BatchedSingleRoom)
    p = [Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:7]
    check(ccall((:rcw_episode_stats_device_ptr, librcw), Cint,
                (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                env.handle, p[1], p[2], p[3], p[4], p[5], p[6], p[7]))
    return (finished = p[1][], outcome = p[2][], length = p[3][], moves = p[4][], level = p[5][], spl_q16 = p[6][], episodes = p[7][])
end
function episode_stats_table(env::BatchedSingleRoom)
    out = Matrix{UInt64}(undef, 8, 1 + Int(episode_stats_info(env).rows))
    check(ccall((:rcw_episode_stats_table, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt64}), env.handle, out)); out
end
function episode_stats_table_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_episode_stats_table_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function episode_stats_clear!(env::BatchedSingleRoom)
    check(ccall((:rcw_episode_stats_clear, librcw), Cint, (Ptr{Cvoid},), env.handle))
    return nothing
end

# ---- the visit map (this build's addition; include/rcw.h, rcw_set_visit_map) ------------------------------------------------------
const VISIT_TABLE = Int32(1)
"""
    set_visit_map!(env, on = true; sectors = 1, table = false)

Keep, on the device, how often each agent has stood in each cell — tile × heading sector — this episode: `visit_map(env)` is the `UInt16`
map as `(H, W, sectors, batch)`; `visit_words(env)` returns `(here, visited, first, level_here)` — `here` the count of the cell the agent
is on (the `N` of `beta / sqrt(N)`), `visited` the cells it has stood in, `first` 1 where the last call entered a cell for the first time
this episode, `level_here` the table's count of the cell on the agent's level.  With `table = true` a `UInt32` table
`(H, W, sectors, 1 + rows)` sums the counts over the batch (slice 1) and per level of the layout source that is live now;
`visit_table_clear!(env)` zeroes it without waiting for the stream.  `visit_cell` is the cell rule for one agent on the host.
"""
function set_visit_map!(env::BatchedSingleRoom, on::Bool = true; sectors::Integer = 1, table::Bool = false)
    check(ccall((:rcw_set_visit_map, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Int32), env.handle, on ? 1 : 0, sectors, table ? VISIT_TABLE : Int32(0)))
    return nothing
end
function visit_map_info(env::BatchedSingleRoom)
    e, s, f, r, l = (Ref{Int32}(0) for _ in 1:5)
    check(ccall((:rcw_visit_map_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}), env.handle, e, s, f, r, l))
    return (enabled = e[] != 0, sectors = s[], table = (f[] & VISIT_TABLE) != 0, rows = r[], first_level = l[])
end
function visit_words(env::BatchedSingleRoom)
    h = Vector{Int32}(undef, env.batch); v = Vector{Int32}(undef, env.batch)
    f = Vector{Int32}(undef, env.batch); l = Vector{UInt32}(undef, env.batch)
    check(ccall((:rcw_visit_words, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt32}), env.handle, h, v, f, l))
    return (here = h, visited = v, first = f, level_here = l)
end
function visit_words_device_ptr(env::BatchedSingleRoom)
    h, v, f, l = (Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:4)
    check(ccall((:rcw_visit_words_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                env.handle, h, v, f, l))
    return (here = h[], visited = v[], first = f[], level_here = l[])
end
function visit_map(env::BatchedSingleRoom, first::Integer = 0, count::Integer = env.batch - first)
    out = Array{UInt16, 4}(undef, env.config.height_tile_map_tu, env.config.width_tile_map_tu, Int(visit_map_info(env).sectors), count)
    check(ccall((:rcw_visit_map, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}), env.handle, first, count, out)); out
end
function visit_map_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_visit_map_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function visit_table(env::BatchedSingleRoom)
    info = visit_map_info(env)
    out = Array{UInt32, 4}(undef, env.config.height_tile_map_tu, env.config.width_tile_map_tu, Int(info.sectors), 1 + Int(info.rows))
    check(ccall((:rcw_visit_table, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt32}), env.handle, out)); out
end
function visit_table_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_visit_table_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function visit_table_clear!(env::BatchedSingleRoom)
    check(ccall((:rcw_visit_table_clear, librcw), Cint, (Ptr{Cvoid},), env.handle))
    return nothing
end
"""
    visit_cell(H, W, nd, sectors, x, y, direction; bits = 32) -> cell

The 0-based cell of an agent at `(x, y)` with the 0-based direction index `direction`: `s*H*W + i + H*j`; `-1`: no cell.
"""
function visit_cell(H::Integer, W::Integer, nd::Integer, sectors::Integer, x::Real, y::Real, direction::Integer; bits::Integer = 32)
    c = Ref{Int32}(0)
    check(ccall((:rcw_visit_cell, librcw), Cint, (Int32, Int32, Int32, Int32, Float64, Float64, Int32, Int32, Ref{Int32}),
                H, W, nd, sectors, x, y, bits, direction, c))
    return c[]
end

# ---- the state archive (this build's addition; include/rcw.h, rcw_set_snapshots) ------------------------------------------------
"""
    set_snapshots!(env, rows)

Bind the state archive: `rows` agent records kept on the device, none filled, laid out for the features that are on NOW (0 frees it).
`save_state!(env; rows = nothing, mask = nothing)` saves the records of the agents of `mask` into the 0-based rows `rows` (`nothing`:
agent `a` into row `a - 1`); `restore_state!(env; rows, mask)` puts them back — several agents may take one row — and renders them again.
Host vectors are checked on the host (a bad index, an unfilled row, two agents into one row: an error, nothing changes); the `_device`
variants take device pointers, wait for nothing and leave a bad agent as it was with its status word set.  `snapshot_filled(env)` says
which rows are filled; `snapshot_export(env)` / `snapshot_import!(env, d)` carry rows between environments of the same shape key.
"""
function set_snapshots!(env::BatchedSingleRoom, rows::Integer)
    check(ccall((:rcw_set_snapshots, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, rows))
    return nothing
end
function snapshot_info(env::BatchedSingleRoom)
    r = Ref{Int32}(0); b = Ref{UInt64}(0); k = Ref{UInt64}(0)
    check(ccall((:rcw_snapshot_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{UInt64}, Ref{UInt64}), env.handle, r, b, k))
    return (rows = r[], row_bytes = b[], shape_key = k[])
end
function snapshot_arguments(env::BatchedSingleRoom, rows, mask)
    r = rows === nothing ? nothing : Vector{Int32}(rows)
    m = mask === nothing ? nothing : Vector{UInt8}(mask .!= 0)
    (r === nothing || length(r) == env.batch) && (m === nothing || length(m) == env.batch) || throw(DimensionMismatch("rows and mask have one entry per agent"))
    return r, m
end
function save_state!(env::BatchedSingleRoom; rows = nothing, mask = nothing)
    r, m = snapshot_arguments(env, rows, mask)
    check(ccall((:rcw_snapshot_save, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{UInt8}), env.handle,
                r === nothing ? C_NULL : r, m === nothing ? C_NULL : m))
    return nothing
end
function restore_state!(env::BatchedSingleRoom; rows = nothing, mask = nothing)
    r, m = snapshot_arguments(env, rows, mask)
    check(ccall((:rcw_snapshot_restore, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{UInt8}), env.handle,
                r === nothing ? C_NULL : r, m === nothing ? C_NULL : m))
    return nothing
end
function save_state_device!(env::BatchedSingleRoom, rows::Ptr{Int32}, mask::Ptr{UInt8})
    check(ccall((:rcw_snapshot_save_device, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{UInt8}), env.handle, rows, mask))
    return nothing
end
function restore_state_device!(env::BatchedSingleRoom, rows::Ptr{Int32}, mask::Ptr{UInt8})
    check(ccall((:rcw_snapshot_restore_device, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{UInt8}), env.handle, rows, mask))
    return nothing
end
function snapshot_filled(env::BatchedSingleRoom)
    out = Vector{UInt8}(undef, Int(snapshot_info(env).rows))
    check(ccall((:rcw_snapshot_filled, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}), env.handle, out))
    return out .!= 0
end
function snapshot_export(env::BatchedSingleRoom; first::Integer = 0, count::Union{Nothing, Integer} = nothing)
    info = snapshot_info(env)
    n = count === nothing ? Int(info.rows) - Int(first) : Int(count)
    out = Matrix{UInt8}(undef, Int(info.row_bytes), max(n, 0))
    check(ccall((:rcw_snapshot_rows_copy, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}), env.handle, first, n, out))
    return (shape_key = info.shape_key, row_bytes = info.row_bytes, rows = out)
end
function snapshot_import!(env::BatchedSingleRoom, d; first::Integer = 0)
    rows = Matrix{UInt8}(d.rows)
    size(rows, 1) == Int(snapshot_info(env).row_bytes) || throw(DimensionMismatch("rows must be (row_bytes, count)"))
    check(ccall((:rcw_snapshot_rows_load, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, UInt64), env.handle, first, size(rows, 2), rows, d.shape_key))
    return nothing
end

# ---- the wall bank (this build's addition; include/rcw.h, rcw_set_wall_bank) ----------------------------------------------------
"""
    set_wall_bank!(env, walls; weights = nothing)

A bank of wall layouts on the device, one drawn for an agent at every start of an episode: `reset!`, a done or truncated restart under
`auto_reset`, and this call, which restarts every agent with the environment's seed (episode counters + 1).  `walls` is `Bool` / `UInt8`
`(H, W, M)` (or `(H, W)`: a bank of one), each layout checked as `set_walls!` checks one; `weights` is `M` integers in `0 : 2^32 - 1`
whose sum lies in `1 : 2^32 - 1` (`nothing`: uniform).  Layout `k` (0-based in `wall_layout(env)`) is drawn with probability
`weights[k + 1] / sum`, a pure function of (seed, global agent id, episode, bank).  `set_walls!` is refused while the bank is on;
`set_wall_bank!(env, nothing)` switches it off, the agents keep the walls they have.  An environment built with `rng` draws its resets
on the host and takes no bank.
"""
function set_wall_bank!(env::BatchedSingleRoom, walls::Union{Nothing, AbstractArray}; weights::Union{Nothing, AbstractVector{<:Integer}} = nothing)
    if walls === nothing
        check(ccall((:rcw_set_wall_bank, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Ptr{UInt32}), env.handle, C_NULL, 0, C_NULL))
        return nothing
    end
    env.rng === nothing || throw(ArgumentError("an environment built with rng draws its resets on the host: it takes no wall bank"))
    H, W = Int(env.config.height_tile_map_tu), Int(env.config.width_tile_map_tu)
    (ndims(walls) in (2, 3) && size(walls, 1) == H && size(walls, 2) == W) || throw(DimensionMismatch("walls must be ($H, $W) or ($H, $W, M)"))
    flat = Vector{UInt8}(vec(walls .!= 0))                                       # column-major: m H W + (i - 1) + H (j - 1)
    layouts = ndims(walls) == 2 ? 1 : size(walls, 3)
    w = weights === nothing ? nothing : Vector{UInt32}(weights)
    w === nothing || length(w) == layouts || throw(DimensionMismatch("expected $(layouts) weights"))
    GC.@preserve flat w check(ccall((:rcw_set_wall_bank, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Ptr{UInt32}),
                                    env.handle, pointer(flat), layouts, w === nothing ? Ptr{UInt32}(C_NULL) : pointer(w)))
    env.stale = true
    return nothing
end
"""
    set_wall_bank_weights!(env, weights)

New weights for the installed bank (`nothing`: uniform), in stream order and without waiting for the device: they hold from each agent's
next episode start, no agent is touched.
"""
function set_wall_bank_weights!(env::BatchedSingleRoom, weights::Union{Nothing, AbstractVector{<:Integer}})
    w = weights === nothing ? nothing : Vector{UInt32}(weights)
    w === nothing || length(w) == wall_bank_info(env).layouts || throw(DimensionMismatch("expected $(wall_bank_info(env).layouts) weights"))
    GC.@preserve w check(ccall((:rcw_set_wall_bank_weights, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt32}), env.handle,
                               w === nothing ? Ptr{UInt32}(C_NULL) : pointer(w)))
    return nothing
end
function wall_bank_info(env::BatchedSingleRoom)
    n = Ref{Int32}(0); t = Ref{UInt64}(0)
    check(ccall((:rcw_wall_bank_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{UInt64}), env.handle, n, t))
    return (layouts = n[], total_weight = t[])
end
function wall_layout(env::BatchedSingleRoom)
    out = Vector{Int32}(undef, env.batch)
    check(ccall((:rcw_wall_layout, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}), env.handle, out)); out
end
function wall_layout_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_wall_layout_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end

# ---- the wall generator (this build's addition; include/rcw.h, rcw_set_wall_generator) --------------------------------------------
"""
    set_wall_generator!(env; loops = 0.0, levels = 0, first_level = 0, level_seed = 0)
    set_wall_generator!(env, nothing)

A new maze made on the device at every start of an episode: `reset!`, a done or truncated restart under `auto_reset`, and this call,
which restarts every agent with the environment's seed (episode counters + 1).  The maze is the minimum spanning tree of the odd
sub-grid of tiles under an order drawn from one 64-bit key, plus the non-tree edges `loops` opens — a probability in `[0, 1]`, scaled
to `UInt32` with `min(floor(p * 2^32), 2^32 - 1)`.  `levels == 0`: every episode a maze of its own, `wall_layout(env)` reads `-1`.
`levels >= 1`: the episode picks level `first_level + (0 : levels - 1)` and the maze is a function of (level_seed, level, H, W, loops)
alone; `wall_layout(env)` says which.  Maps of 5 x 5 to 129 x 129.  `set_walls!` and `set_wall_bank!` are refused while the generator
is on; `set_wall_generator!(env, nothing)` switches it off, the agents keep their walls.  An environment built with `rng` draws its
resets on the host and takes no generator.
"""
function set_wall_generator!(env::BatchedSingleRoom; loops::Real = 0.0, levels::Integer = 0, first_level::Integer = 0, level_seed::Integer = 0)
    env.rng === nothing || throw(ArgumentError("an environment built with rng draws its resets on the host: it takes no wall generator"))
    0 <= loops <= 1 || throw(ArgumentError("loops is a probability in [0, 1]"))
    word = UInt32(min(floor(UInt64, Float64(loops) * 2.0^32), UInt64(0xFFFFFFFF)))
    check(ccall((:rcw_set_wall_generator, librcw), Cint, (Ptr{Cvoid}, Int32, UInt32, Int32, Int32, UInt64),
                env.handle, 1, word, levels, first_level, level_seed))
    env.stale = true
    return nothing
end
function set_wall_generator!(env::BatchedSingleRoom, ::Nothing)
    check(ccall((:rcw_set_wall_generator, librcw), Cint, (Ptr{Cvoid}, Int32, UInt32, Int32, Int32, UInt64), env.handle, 0, 0, 0, 0, 0))
    return nothing
end
function wall_generator_info(env::BatchedSingleRoom)
    on = Ref{Int32}(0); loops = Ref{UInt32}(0); levels = Ref{Int32}(0); first = Ref{Int32}(0); seed = Ref{UInt64}(0)
    check(ccall((:rcw_wall_generator_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{UInt32}, Ref{Int32}, Ref{Int32}, Ref{UInt64}),
                env.handle, on, loops, levels, first, seed))
    return (enabled = on[] != 0, loops = loops[], levels = levels[], first_level = first[], level_seed = seed[])
end
"""
    generated_maze_key(seed, global_agent, episode; levels = 0, first_level = 0, level_seed = 0) -> (maze_key, level)

The wall generator's maze key and level (`-1` with `levels == 0`) of episode `episode` (the counter before the increment) of a global
agent: host arithmetic, no device.
"""
function generated_maze_key(seed::Integer, global_agent::Integer, episode::Integer; levels::Integer = 0, first_level::Integer = 0, level_seed::Integer = 0)
    key = Ref{UInt64}(0); level = Ref{Int32}(0)
    check(ccall((:rcw_wall_generator_key, librcw), Cint, (UInt64, Int32, UInt32, Int32, Int32, UInt64, Ref{UInt64}, Ref{Int32}),
                seed, global_agent, episode, levels, first_level, level_seed, key, level))
    return (key[], level[])
end
"""
    generated_maze(maze_key, H, W; loops = 0.0) -> BitMatrix (H, W)

The wall generator's maze of one key (`true` = wall), as an agent's WALL layer holds it: host arithmetic (Kruskal), no device.
"""
function generated_maze(maze_key::Integer, H::Integer, W::Integer; loops::Real = 0.0)
    0 <= loops <= 1 || throw(ArgumentError("loops is a probability in [0, 1]"))
    word = UInt32(min(floor(UInt64, Float64(loops) * 2.0^32), UInt64(0xFFFFFFFF)))
    out = Matrix{UInt8}(undef, max(H, 0), max(W, 0))                             # column-major: tile (i, j) at (i - 1) + H (j - 1)
    check(ccall((:rcw_wall_generator_layout, librcw), Cint, (Int32, Int32, UInt64, UInt32, Ptr{UInt8}), H, W, maze_key, word, out))
    return out .!= 0
end

# ---- the wall generator: caves (this build's addition; include/rcw.h, rcw_set_wall_caves) -----------------------------------------
"""
    set_wall_caves!(env; fill = 0.40, smooth = 2, levels = 0, first_level = 0, level_seed = 0)
    set_wall_caves!(env, nothing)

A new cave made on the device at every start of an episode, where `set_wall_generator!` makes a maze: the interior filled with
probability `fill` (scaled to `UInt32` as `loops` is), smoothed `smooth` times (0 to 8) by the 5-of-9 automaton and pruned to its
largest 4-connected region; a cave whose region has fewer than `max(7, (H-2)(W-2) ÷ 4)` tiles is replaced by the perfect maze of the
same key (on small maps that is most of them).  The level parameters and `wall_layout(env)` are the generator's.  Maps of 5 x 5 up to
4096 interior tiles (66 x 66).  `set_walls!`, `set_wall_bank!` and `set_wall_generator!` are refused while caves are on;
`set_wall_caves!(env, nothing)` switches them off, the agents keep their walls.  An environment built with `rng` takes no caves.
"""
function set_wall_caves!(env::BatchedSingleRoom; fill::Real = 0.40, smooth::Integer = 2, levels::Integer = 0, first_level::Integer = 0, level_seed::Integer = 0)
    env.rng === nothing || throw(ArgumentError("an environment built with rng draws its resets on the host: it takes no wall caves"))
    0 <= fill <= 1 || throw(ArgumentError("fill is a probability in [0, 1]"))
    word = UInt32(min(floor(UInt64, Float64(fill) * 2.0^32), UInt64(0xFFFFFFFF)))
    check(ccall((:rcw_set_wall_caves, librcw), Cint, (Ptr{Cvoid}, Int32, UInt32, Int32, Int32, Int32, UInt64),
                env.handle, 1, word, smooth, levels, first_level, level_seed))
    env.stale = true
    return nothing
end
function set_wall_caves!(env::BatchedSingleRoom, ::Nothing)
    check(ccall((:rcw_set_wall_caves, librcw), Cint, (Ptr{Cvoid}, Int32, UInt32, Int32, Int32, Int32, UInt64), env.handle, 0, 0, 0, 0, 0, 0))
    return nothing
end
function wall_caves_info(env::BatchedSingleRoom)
    on = Ref{Int32}(0); fill = Ref{UInt32}(0); smooth = Ref{Int32}(0)
    check(ccall((:rcw_wall_caves_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{UInt32}, Ref{Int32}), env.handle, on, fill, smooth))
    return (enabled = on[] != 0, fill = fill[], smooth = smooth[])
end
"""
    generated_cave(key, H, W; fill = 0.40, smooth = 2) -> (BitMatrix (H, W), fell_back)

The wall generator's cave of one key (`generated_maze_key` serves both families; `true` = wall), as an agent's WALL layer holds it, and
whether it is the fallback maze: host arithmetic (a queue flood fill), no device.
"""
function generated_cave(key::Integer, H::Integer, W::Integer; fill::Real = 0.40, smooth::Integer = 2)
    0 <= fill <= 1 || throw(ArgumentError("fill is a probability in [0, 1]"))
    word = UInt32(min(floor(UInt64, Float64(fill) * 2.0^32), UInt64(0xFFFFFFFF)))
    out = Matrix{UInt8}(undef, max(H, 0), max(W, 0))                             # column-major: tile (i, j) at (i - 1) + H (j - 1)
    fell = Ref{Int32}(0)
    check(ccall((:rcw_wall_caves_layout, librcw), Cint, (Int32, Int32, UInt64, UInt32, Int32, Ptr{UInt8}, Ref{Int32}), H, W, key, word, smooth, out, fell))
    return (out .!= 0, fell[] != 0)
end

# ---- the wall generator: rooms (this build's addition; include/rcw.h, rcw_set_wall_rooms) -----------------------------------------
"""
    set_wall_rooms!(env; room = 2, stop = 0.25, doors = 0.25, levels = 0, first_level = 0, level_seed = 0)
    set_wall_rooms!(env, nothing)

New rooms made on the device at every start of an episode, where `set_wall_generator!` makes a maze: the interior is split
recursively by walls on even lines, each with a door and, with probability `doors`, a second one; a chamber other than the whole
interior is left a room with probability `stop` (both scaled to `UInt32` as `loops` is); no room side falls below `room`.  Connected by
construction from 5 x 5: no fallback.  The level parameters and `wall_layout(env)` are the generator's.  Maps up to
`cld(H-2, 2) * cld(W-2, 2) == 4096` (130 x 130, 5 x 4097).  `set_walls!`, `set_wall_bank!`, `set_wall_generator!` and `set_wall_caves!`
are refused while rooms are on; `set_wall_rooms!(env, nothing)` switches them off, the agents keep their walls.  An environment built
with `rng` takes no rooms.
"""
function set_wall_rooms!(env::BatchedSingleRoom; room::Integer = 2, stop::Real = 0.25, doors::Real = 0.25, levels::Integer = 0, first_level::Integer = 0,
                         level_seed::Integer = 0)
    env.rng === nothing || throw(ArgumentError("an environment built with rng draws its resets on the host: it takes no wall rooms"))
    (0 <= stop <= 1 && 0 <= doors <= 1) || throw(ArgumentError("stop and doors are probabilities in [0, 1]"))
    word(p) = UInt32(min(floor(UInt64, Float64(p) * 2.0^32), UInt64(0xFFFFFFFF)))
    check(ccall((:rcw_set_wall_rooms, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, UInt32, UInt32, Int32, Int32, UInt64),
                env.handle, 1, room, word(stop), word(doors), levels, first_level, level_seed))
    env.stale = true
    return nothing
end
function set_wall_rooms!(env::BatchedSingleRoom, ::Nothing)
    check(ccall((:rcw_set_wall_rooms, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, UInt32, UInt32, Int32, Int32, UInt64), env.handle, 0, 0, 0, 0, 0, 0, 0))
    return nothing
end
function wall_rooms_info(env::BatchedSingleRoom)
    on = Ref{Int32}(0); room = Ref{Int32}(0); stop = Ref{UInt32}(0); doors = Ref{UInt32}(0)
    check(ccall((:rcw_wall_rooms_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{UInt32}, Ref{UInt32}), env.handle, on, room, stop, doors))
    return (enabled = on[] != 0, room = room[], stop = stop[], doors = doors[])
end
"""
    generated_rooms(key, H, W; room = 2, stop = 0.25, doors = 0.25) -> (BitMatrix (H, W), rooms)

The wall generator's rooms of one key (`generated_maze_key` serves every family; `true` = wall), as an agent's WALL layer holds them,
and how many rooms there are: host arithmetic (depth first off a stack), no device.
"""
function generated_rooms(key::Integer, H::Integer, W::Integer; room::Integer = 2, stop::Real = 0.25, doors::Real = 0.25)
    (0 <= stop <= 1 && 0 <= doors <= 1) || throw(ArgumentError("stop and doors are probabilities in [0, 1]"))
    word(p) = UInt32(min(floor(UInt64, Float64(p) * 2.0^32), UInt64(0xFFFFFFFF)))
    out = Matrix{UInt8}(undef, max(H, 0), max(W, 0))                             # column-major: tile (i, j) at (i - 1) + H (j - 1)
    rooms = Ref{Int32}(0)
    check(ccall((:rcw_wall_rooms_layout, librcw), Cint, (Int32, Int32, UInt64, Int32, UInt32, UInt32, Ptr{UInt8}, Ref{Int32}),
                H, W, key, room, word(stop), word(doors), out, rooms))
    return (out .!= 0, Int(rooms[]))
end

# per-agent sticky status: 0, -5 where the reference would have raised BoundsError, -2 for an invalid device action,
# 1 (a warning) where sample_empty_position gave up after max_tries and returned an occupied tile (utils.jl:34 @warns there)
function status(env::BatchedSingleRoom)
    out = Vector{Int32}(undef, env.batch)
    check(ccall((:rcw_status, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}), env.handle, out)); out
end
# tile_map as B BitArray{3}(2, H, W): the library hands back `.chunks` verbatim
function tile_maps(env::BatchedSingleRoom)
    n = Ref{Int32}(0)
    check(ccall((:rcw_tile_map_num_chunks, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, n))
    chunks = Matrix{UInt64}(undef, n[], env.batch)
    check(ccall((:rcw_tile_map_chunks, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt64}), env.handle, chunks))
    H, W = env.config.height_tile_map_tu, env.config.width_tile_map_tu
    return map(1:env.batch) do b
        tm = falses(2, H, W)
        copyto!(tm.chunks, view(chunks, :, b))
        tm
    end
end

# world.ray_stop_position_tu / ray_hit_dimension / ray_distance_wu / ray_directions_wu (single_room.jl:29-31,39)
# of agents first+1 : first+count (0-based `first`, as in the C ABI)
function rays(env::BatchedSingleRoom{Float32}; first::Integer = 0, count::Integer = env.batch - first)
    N = Int(env.config.num_rays)
    stop = Array{Int64, 3}(undef, 2, N, count); dim = Matrix{Int64}(undef, N, count)
    dist = Matrix{Float32}(undef, N, count); dirs = Array{Float32, 3}(undef, 2, N, count)
    check(ccall((:rcw_rays, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float32}, Ptr{Float32}),
                env.handle, first, count, stop, dim, dist, dirs))
    return (ray_stop_position_tu = stop, ray_hit_dimension = dim, ray_distance_wu = dist, ray_directions_wu = dirs)
end
function rays(env::BatchedSingleRoom{Float64}; first::Integer = 0, count::Integer = env.batch - first)
    N = Int(env.config.num_rays)
    stop = Array{Int64, 3}(undef, 2, N, count); dim = Matrix{Int64}(undef, N, count)
    dist = Matrix{Float64}(undef, N, count); dirs = Array{Float64, 3}(undef, 2, N, count)
    check(ccall((:rcw_rays64, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                env.handle, first, count, stop, dim, dist, dirs))
    return (ray_stop_position_tu = stop, ray_hit_dimension = dim, ray_distance_wu = dist, ray_directions_wu = dirs)
end

# directions_wu (single_room.jl:28) and the (direction, ray) table the kernels use: (N, 5, nd)
function directions_wu(env::BatchedSingleRoom{Float32})
    out = Matrix{Float32}(undef, 2, env.config.num_directions)
    check(ccall((:rcw_direction_table, librcw), Cint, (Ptr{Cvoid}, Ptr{Float32}), env.handle, out)); out
end
function directions_wu(env::BatchedSingleRoom{Float64})
    out = Matrix{Float64}(undef, 2, env.config.num_directions)
    check(ccall((:rcw_direction_table64, librcw), Cint, (Ptr{Cvoid}, Ptr{Float64}), env.handle, out)); out
end
function ray_table(env::BatchedSingleRoom{Float32})
    out = Array{Float32, 3}(undef, env.config.num_rays, 5, env.config.num_directions)
    check(ccall((:rcw_ray_table, librcw), Cint, (Ptr{Cvoid}, Ptr{Float32}), env.handle, out)); out
end
function ray_table(env::BatchedSingleRoom{Float64})
    out = Array{Float64, 3}(undef, env.config.num_rays, 5, env.config.num_directions)
    check(ccall((:rcw_ray_table64, librcw), Cint, (Ptr{Cvoid}, Ptr{Float64}), env.handle, out)); out
end

#####
##### images
#####

# Device pointer of the observation batch (aliased, stable): for AMDGPU.jl users
#   unsafe_wrap(ROCArray{UInt32,3}, Ptr{UInt32}(ptr), (H_cam, N, B))
# The buffer is the library's between calls.  After every step it equals the reference's `camera_view` for every agent.
# A step may leave untouched the frames of agents whose view it did not change.  A caller that writes into the buffer
# calls `RCW.update_camera_view!(env)` or `bind_obs!` before the next step.
function camera_view_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_obs_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
# The host mirror, refreshed only if a step / reset happened since the last refresh (the SAME array every call)
function camera_view(env::BatchedSingleRoom)
    if env.stale
        check(ccall((:rcw_obs_copy, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt32}, Int32, Int32),
                    env.handle, env.camera_view, 0, env.batch))
        env.stale = false
    end
    return env.camera_view
end
# Render into caller-owned device memory instead (double-buffered observations); C_NULL restores the library's buffer.
# The step after a `bind_obs!` — also with the pointer the handle already has — stores every frame: callers that alternate
# two buffers get every step written in full.
bind_obs!(env::BatchedSingleRoom, device_ptr::Ptr{Cvoid}) =
    check(ccall((:rcw_bind_obs, librcw), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), env.handle, device_ptr))

# env.top_view (single_room.jl:302; build with render_top_view = 1): (H*pu, W*pu, count) copied to host
function top_view(env::BatchedSingleRoom; first::Integer = 0, count::Integer = env.batch - first)
    c = env.config
    out = Array{UInt32, 3}(undef, c.height_tile_map_tu * c.pu_per_tu, c.width_tile_map_tu * c.pu_per_tu, count)
    check(ccall((:rcw_top_view_copy, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt32}, Int32, Int32), env.handle, out, first, count)); out
end
function top_view_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_top_view_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function reward_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_reward_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function done_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_done_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end

# The RLBase verbs for a GPU-RESIDENT agent: where `RLBase.state / reward / is_terminated` below hand out host arrays
# (one device-to-host copy and a wait for the engine's stream per call), these hand out what the engine itself writes —
# (device pointer, element type, dims), stable for the handle's lifetime and refreshed by every step in stream order, to
# be wrapped once, e.g. with AMDGPU.jl `unsafe_wrap(ROCArray{R,1}, Ptr{R}(ptr), dims)`.  A loop
# `act!(env, actions_device_ptr) -> policy kernels on stream(env)` then never synchronises the host (the Python mirror's
# RLBase.reward / is_terminated return exactly these aliases by default; bench.py --api rlbase measures the loop).
state_device(env::BatchedSingleRoom) =
    (ptr = camera_view_device_ptr(env), eltype = UInt32,
     dims = (Int(env.config.height_camera_view_pu), Int(env.config.num_rays), env.batch))
reward_device(env::BatchedSingleRoom{T, R}) where {T, R} = (ptr = reward_device_ptr(env), eltype = R, dims = (env.batch,))
is_terminated_device(env::BatchedSingleRoom) = (ptr = done_device_ptr(env), eltype = UInt8, dims = (env.batch,))

# The compact per-column descriptor of the frames: height_line_pu (single_room.jl:408-411) and colour id by image column
function columns(env::BatchedSingleRoom; first::Integer = 0, count::Integer = env.batch - first)
    N = Int(env.config.num_rays)
    h = Matrix{Int32}(undef, N, count); c = Matrix{UInt8}(undef, N, count)
    check(ccall((:rcw_columns, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{UInt8}), env.handle, first, count, h, c))
    return (height_line_pu = h, colour_id = c)
end
function columns_device_ptr(env::BatchedSingleRoom)
    h = Ref{Ptr{Cvoid}}(C_NULL); c = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_columns_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}), env.handle, h, c))
    return (h[], c[])
end
# descriptors (device pointers) -> frames (device pointer), with this handle's colours: the receiving side of a gather
expand_columns!(env::BatchedSingleRoom, height_line_pu_device::Ptr{Int32}, colour_id_device::Ptr{UInt8}, count::Integer,
                frames_device::Ptr{Cvoid}) =
    check(ccall((:rcw_expand_columns, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
                env.handle, height_line_pu_device, colour_id_device, count, frames_device))

#####
##### the learner view: UInt8 RGB / gray / inverse depth, area-averaged to (h, w), rendered by every reset / step (include/rcw.h)
#####

# format = :gray | :rgb | :depth (inverse depth, one plane) | :rgbd (R, G, B, D) | :grayd (Y, D) | :off; size = (h, w) with h <= height_camera_view_pu, w <= num_rays; layout = :chw | :hwc;
# camera_view = false: steps skip the UInt32 camera view (RCW_VIEW_ONLY).  Renders the current state at once.
# stack = k (1 .. 16, :chw only): the view holds each agent's last k frames, slot 1 the oldest (Julia sees (w, h, k C, B)); the engine
# shifts it at every step and fills all k slots with the new frame at reset!, set_state! and when auto_reset restarts the agent.
function set_learner_view!(env::BatchedSingleRoom; format::Symbol = :gray,
                           size::Tuple{Integer, Integer} = (env.config.height_camera_view_pu, env.config.num_rays),
                           layout::Symbol = :chw, camera_view::Bool = true, stack::Integer = 1)
    fmt = format === :gray ? RCW_VIEW_GRAY8 : format === :rgb ? RCW_VIEW_RGB8 : format === :depth ? RCW_VIEW_DEPTH8 :
          format === :rgbd ? RCW_VIEW_RGBD8 : format === :grayd ? RCW_VIEW_GRAYD8 : format === :off ? RCW_VIEW_OFF :
          throw(ArgumentError("format must be :gray, :rgb, :depth, :rgbd, :grayd or :off"))
    lay = layout === :chw ? RCW_VIEW_CHW : layout === :hwc ? RCW_VIEW_HWC : throw(ArgumentError("layout must be :chw or :hwc"))
    flags = camera_view ? Int32(0) : RCW_VIEW_ONLY
    stack == 1 && return check(ccall((:rcw_set_learner_view, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32),
                                     env.handle, fmt, lay, size[1], size[2], flags))
    check(ccall((:rcw_set_learner_view_stack, librcw), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32, Int32),
                env.handle, fmt, lay, size[1], size[2], flags, stack))
end
# the number of frame slots of the learner view (0: no view)
function learner_view_stack(env::BatchedSingleRoom)
    k = Ref{Int32}(0)
    check(ccall((:rcw_learner_view_stack, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, k))
    return Int(k[])
end
function learner_view_info(env::BatchedSingleRoom)
    f = Ref{Int32}(0); l = Ref{Int32}(0); h = Ref{Int32}(0); w = Ref{Int32}(0); fl = Ref{Int32}(0)
    check(ccall((:rcw_learner_view_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}),
                env.handle, f, l, h, w, fl))
    return (format = f[], layout = l[], height = h[], width = w[], flags = fl[])
end
# The column-major shape Julia sees of the C-order (B, k C, h, w) / (B, h, w, C) batch: (w, h, k C, B) for :chw, (C, w, h, B) for :hwc
function learner_view_dims(env::BatchedSingleRoom)
    v = learner_view_info(env)
    v.format == RCW_VIEW_OFF && error("no learner view: call set_learner_view! first")
    C = ((v.format & Int32(3)) == RCW_VIEW_RGB8 ? 3 : (v.format & Int32(3)) == RCW_VIEW_GRAY8 ? 1 : 0) + ((v.format & RCW_VIEW_DEPTH8) != 0 ? 1 : 0)
    return v.layout == RCW_VIEW_CHW ? (Int(v.width), Int(v.height), learner_view_stack(env) * C, env.batch) : (C, Int(v.width), Int(v.height), env.batch)
end
function learner_view_device_ptr(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_learner_view_device_ptr, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p))
    return p[]
end
# agents [first, first + count) of the learner view on the host, in learner_view_dims' shape
function learner_view(env::BatchedSingleRoom; first::Integer = 0, count::Integer = env.batch - first)
    dims = learner_view_dims(env)
    out = Array{UInt8, 4}(undef, dims[1], dims[2], dims[3], count)
    check(ccall((:rcw_learner_view_copy, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32), env.handle, out, first, count))
    return out
end
# descriptors (device pointers) -> this handle's learner view of them (device pointer, count * C * h * w bytes)
expand_columns_view!(env::BatchedSingleRoom, height_line_pu_device::Ptr{Int32}, colour_id_device::Ptr{UInt8}, count::Integer,
                     view_device::Ptr{Cvoid}) =
    check(ccall((:rcw_expand_columns_view, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
                env.handle, height_line_pu_device, colour_id_device, count, view_device))

#####
##### streams, device memory, timing, introspection
#####

set_stream!(env::BatchedSingleRoom, hip_stream::Ptr{Cvoid}) =
    check(ccall((:rcw_set_stream, librcw), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), env.handle, hip_stream))
function get_stream(env::BatchedSingleRoom)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_get_stream, librcw), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), env.handle, p)); p[]
end
function device_malloc(env::BatchedSingleRoom, bytes::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rcw_device_malloc, librcw), Cint, (Ptr{Cvoid}, UInt64, Ref{Ptr{Cvoid}}), env.handle, bytes, p)); p[]
end
device_free(env::BatchedSingleRoom, p::Ptr{Cvoid}) =
    check(ccall((:rcw_device_free, librcw), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), env.handle, p))
memcpy_to_host!(env::BatchedSingleRoom, dst::Array, src_device::Ptr{Cvoid}) =
    check(ccall((:rcw_memcpy_to_host, librcw), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, UInt64),
                env.handle, dst, src_device, sizeof(dst)))

timer_start(env::BatchedSingleRoom) = check(ccall((:rcw_timer_start, librcw), Cint, (Ptr{Cvoid},), env.handle))
function timer_stop(env::BatchedSingleRoom)
    ms = Ref{Float32}(0)
    check(ccall((:rcw_timer_stop, librcw), Cint, (Ptr{Cvoid}, Ref{Float32}), env.handle, ms)); ms[]
end
profile!(env::BatchedSingleRoom, enable::Bool) =
    check(ccall((:rcw_profile, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, enable ? 1 : 0))
function profile_read(env::BatchedSingleRoom)
    c = Ref{Float32}(0); t = Ref{Float32}(0); f = Ref{Float32}(0); n = Ref{Int32}(0)
    check(ccall((:rcw_profile_read, librcw), Cint, (Ptr{Cvoid}, Ref{Float32}, Ref{Float32}, Ref{Float32}, Ref{Int32}),
                env.handle, c, t, f, n))
    return (cast_ms = c[], top_view_ms = t[], fill_ms = f[], steps = n[])
end
"Which kernel form `update_top_view!` takes: `:none`, `:in_place`, `:one_kernel` or `:two_kernels` (rcw.h)."
function top_view_form(env::BatchedSingleRoom)
    f = Ref{Int32}(0)
    check(ccall((:rcw_top_view_form, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, f))
    return (:none, :in_place, :one_kernel, :two_kernels)[f[] + 1]
end
"The form `update_top_view!(env)` takes when it is called alone, outside a step (`rcw_update_top_view_form`)."
function update_top_view_form(env::BatchedSingleRoom)
    f = Ref{Int32}(0)
    check(ccall((:rcw_update_top_view_form, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, f))
    return (:none, :in_place, :one_kernel, :two_kernels)[f[] + 1]
end
"""
    set_top_view_form!(env, form = :auto; runs = 0)

Choose the kernel form of `update_top_view!` instead of the library's rule (`rcw_set_top_view_form`): `:auto`,
`:in_place`, `:one_kernel` or `:two_kernels`; `runs` = 0 (automatic) or 1..8 runs of agents for the two-kernel form.
All forms write the same pixels.  Throws when the geometry cannot take the form (the handle keeps the automatic one).
"""
function set_top_view_form!(env::BatchedSingleRoom, form::Symbol = :auto; runs::Integer = 0)
    code = Dict(:auto => 0, :in_place => 1, :one_kernel => 2, :two_kernels => 3)[form]
    check(ccall((:rcw_set_top_view_form, librcw), Cint, (Ptr{Cvoid}, Int32, Int32), env.handle, code, runs))
    return nothing
end
"How many launches a step takes (`rcw_step_form`): `:two_launches` (cast kernel, then fill kernel) or `:one_launch`."
function step_form(env::BatchedSingleRoom)
    f = Ref{Int32}(0)
    check(ccall((:rcw_step_form, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, f))
    return (:two_launches, :one_launch)[f[]]
end
"""
    set_step_form!(env, form = :auto)

Choose the step's form instead of the library's rule (`rcw_set_step_form`): `:auto`, `:two_launches` or `:one_launch`
(the fill workgroups of a launch write the frames the actions select among the successor states the previous launch cast).
Both leave the same state and the same pixels.  Throws where the geometry cannot take the one-launch form.
"""
function set_step_form!(env::BatchedSingleRoom, form::Symbol = :auto)
    code = Dict(:auto => 0, :two_launches => 1, :one_launch => 2)[form]
    check(ccall((:rcw_set_step_form, librcw), Cint, (Ptr{Cvoid}, Int32), env.handle, code))
    return nothing
end
"The kernel `update_camera_view!` takes for this camera height and batch (`rcw_fill_kernel_name`)."
function fill_kernel_name(env::BatchedSingleRoom)
    buf = Vector{UInt8}(undef, 64)
    check(ccall((:rcw_fill_kernel_name, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32), env.handle, buf, length(buf)))
    return unsafe_string(pointer(buf))
end
function batch(env::BatchedSingleRoom)
    n = Ref{Int32}(0)
    check(ccall((:rcw_batch, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}), env.handle, n)); Int(n[])
end
function get_config(env::BatchedSingleRoom)
    cfg = RcwConfig()
    check(ccall((:rcw_get_config, librcw), Cint, (Ptr{Cvoid}, Ref{RcwConfig}), env.handle, cfg)); cfg
end
function device_name(env::BatchedSingleRoom)
    buf = Vector{UInt8}(undef, 256)
    check(ccall((:rcw_device_name, librcw), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32), env.handle, buf, length(buf)))
    return unsafe_string(pointer(buf))
end

#####
##### multi-GPU: one process (or task) per GPU, agents sharded by rank; the observation gather over RCCL
#####
# rank 0 makes the id and ships its 128 bytes to the other ranks (Distributed.jl, MPI.jl, a file — caller's choice)
function comm_unique_id()
    id = Vector{UInt8}(undef, RCW_UNIQUE_ID_BYTES)
    check(ccall((:rcw_comm_unique_id, librcw), Cint, (Ptr{Cvoid},), id)); id
end
comm_init!(env::BatchedSingleRoom, unique_id::Vector{UInt8}, rank::Integer, world::Integer) =
    check(ccall((:rcw_comm_init, librcw), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32), env.handle, unique_id, rank, world))
comm_destroy!(env::BatchedSingleRoom) = check(ccall((:rcw_comm_destroy, librcw), Cint, (Ptr{Cvoid},), env.handle))
function comm_info(env::BatchedSingleRoom)
    r = Ref{Int32}(0); w = Ref{Int32}(0)
    check(ccall((:rcw_comm_info, librcw), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), env.handle, r, w))
    return (rank = Int(r[]), world = Int(w[]))
end
# all-gather of the compact descriptors into caller-owned device memory (B*world columns each)
gather_columns!(env::BatchedSingleRoom, height_line_pu_all_device::Ptr{Int32}, colour_id_all_device::Ptr{UInt8}) =
    check(ccall((:rcw_gather_columns, librcw), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{UInt8}),
                env.handle, height_line_pu_all_device, colour_id_all_device))
# the GLOBAL observation batch (H_cam, N, B*world) into caller-owned device memory
gather_observations!(env::BatchedSingleRoom, frames_all_device::Ptr{Cvoid}; mode::Int32 = RCW_GATHER_COLUMNS) =
    check(ccall((:rcw_gather_observations, librcw), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}), env.handle, mode, frames_all_device))
# ... and as a host Array, through a device buffer the binding keeps (what a learner on rank 0 would read)
function gather_observations(env::BatchedSingleRoom; mode::Int32 = RCW_GATHER_COLUMNS)
    world = comm_info(env).world
    world >= 1 || throw(ArgumentError("comm_init! first"))
    c = env.config
    out = Array{UInt32, 3}(undef, c.height_camera_view_pu, c.num_rays, env.batch * world)
    if env.gather_frames != env.batch * world
        env.gather_buffer != C_NULL && device_free(env, env.gather_buffer)
        env.gather_buffer = device_malloc(env, sizeof(out))
        env.gather_frames = env.batch * world
    end
    gather_observations!(env, env.gather_buffer; mode = mode)
    memcpy_to_host!(env, out, env.gather_buffer)
    return out
end

#####
##### RLBase API  — single_room.jl:574-584
#####

RLBase.StateStyle(env::RCW.RLBaseEnv{E}) where {E <: BatchedSingleRoom} = RLBase.Observation{Any}()
RLBase.state_space(env::RCW.RLBaseEnv{E}, ::RLBase.Observation) where {E <: BatchedSingleRoom} = nothing
RLBase.state(env::RCW.RLBaseEnv{E}, ::RLBase.Observation) where {E <: BatchedSingleRoom} = camera_view(env.env)
RLBase.reset!(env::RCW.RLBaseEnv{E}) where {E <: BatchedSingleRoom} = RCW.reset!(env.env)
RLBase.action_space(env::RCW.RLBaseEnv{E}) where {E <: BatchedSingleRoom} = Base.OneTo(NUM_ACTIONS)
(env::RCW.RLBaseEnv{E})(action) where {E <: BatchedSingleRoom} = RCW.act!(env.env, action)
RLBase.reward(env::RCW.RLBaseEnv{E}) where {E <: BatchedSingleRoom} = reward(env.env)
RLBase.is_terminated(env::RCW.RLBaseEnv{E}) where {E <: BatchedSingleRoom} = done(env.env)

end # module
