// The goal distance (include/rcw.h, rcw_set_goal_distance): per agent the breadth-first distance field from its goal through its walls,
// UInt16 (H*W) in the tile map's linear order, and three Int32 words — distance at the player's tile, distance at the episode's start,
// progress of the last call.  One kernel behind every step / reset / set_state / set_walls of a handle that enabled it; nothing else
// of the library knows about it.
//
// rcw_goal_distance_kernel: ONE WAVEFRONT PER AGENT (a 64-thread workgroup: every __syncthreads below orders the wave's own LDS traffic and
// costs no barrier instruction).  An agent whose field is current — the usual case of a step — reads its two counters, its position, one field
// entry and its distance, and writes two words.  An agent whose field is stale (in the mask of a refill launch, or its episode counter is not the recorded one: auto_reset
// re-sampled it in the step in front) floods first:
//   LDS   `blocked`, a bit per tile (walls, then also what the flood has reached), and `queue`, the tile indices in the order reached
//         (UInt16: H*W <= 65280; every tile enters at most once, so H*W entries always suffice).  H*W / 8 + 2 H*W bytes: 2.2 KiB at 32 x 32,
//         135.5 KiB at the largest map rcw_create accepts — one path for every size.
//   HBM   the field is only ever WRITTEN: a tile's distance is the level the wave is at when the tile leaves the queue, so the flood never
//         reads a distance back and no global latency sits in the loop.  Behind the flood one coalesced pass writes 0xFFFF to the walls and
//         to what was not reached; the two sets of stores are disjoint.
// A level is the queue segment [head, level_end): a lane a tile, the four neighbours claimed with an LDS atomic OR on `blocked` (the lane that
// flips the bit owns the tile), appended behind a ballot prefix — the tail stays in a scalar register.  Work is proportional to the free
// tiles (each is popped once and looks at four neighbours), not to levels x tiles: a serpentine 254 x 254 has 31,877 levels of one tile.
// The player's distance is picked up in passing (the lane that pops the player's tile leaves the level in LDS): the field is not read back.
#include "rcw_device.h"

namespace {

constexpr int kGoalBlock = 64;            // one wavefront
constexpr uint32_t kUnreached = 0xFFFFu;

// bit t of the result = bit 2 t of x (the WALL layer of 16 tiles of a tile-map word)
__device__ __forceinline__ uint32_t even_bits(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

struct GoalDistanceArgs {
    int32_t B, H, W, nwords, real64, refill;
    const float2* pos;
    const double2* pos64;
    const int2* goal;
    const uint32_t* episode;
    const uint32_t* tile_map;
    const uint8_t* mask;
    uint16_t* field;             // [B][H*W]
    RcwGoalWords words;
    uint32_t* last_episode;      // [B] the episode counter the agent's field was flooded in
};

__global__ __launch_bounds__(kGoalBlock) void rcw_goal_distance_kernel(const GoalDistanceArgs g)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_g[];
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= g.B) return;
    if (g.refill && g.mask != nullptr && g.mask[a] == 0) return;          // an agent outside the call's mask keeps every byte
    const uint32_t ep = g.episode[a];
    const bool stale = g.refill || g.last_episode[a] != ep;
    const int H = g.H, W = g.W, HW = H * W;
    // the player's tile, 0-based (wu_to_tu UT:5 minus one); -1: off the map (also a NaN)
    double x, y;
    if (g.real64) { const double2 q = g.pos64[a]; x = q.x; y = q.y; }
    else          { const float2 q = g.pos[a]; x = (double)q.x; y = (double)q.y; }
    const double fx = floor(x), fy = floor(y);                            // (floor of a Float32 is the same number in Float64)
    const bool on_map = fx >= 0.0 && fx < (double)H && fy >= 0.0 && fy < (double)W;
    const int tp = on_map ? (int)fx + H * (int)fy : -1;
    uint16_t* const field = g.field + (size_t)a * HW;

    if (!stale) {
        if (lane == 0) {
            const uint32_t f = tp >= 0 ? (uint32_t)field[tp] : kUnreached;
            const int32_t now = f == kUnreached ? -1 : (int32_t)f, old = g.words.distance[a];
            g.words.progress[a] = old >= 0 && now >= 0 ? old - now : 0;
            g.words.distance[a] = now;
        }
        return;
    }

    // ---- the flood -------------------------------------------------------------------------------------------------------------
    const int bwords = (HW + 31) >> 5;
    uint32_t* const blocked = lds_g;                                       // [bwords]
    uint32_t* const found = lds_g + bwords;                                // the player's distance, once its tile is popped
    uint16_t* const queue = reinterpret_cast<uint16_t*>(lds_g + bwords + 1);   // [HW]
    const uint32_t* const tm = g.tile_map + (size_t)a * g.nwords;
    for (int w = lane; w < bwords; w += kGoalBlock) {                      // (nwords is even and >= HW / 16: 2 w + 1 is inside)
        uint32_t b = even_bits(tm[2 * w]) | (even_bits(tm[2 * w + 1]) << 16);
        if (w == bwords - 1 && (HW & 31) != 0) b |= ~0u << (HW & 31);      // past the map: blocked
        blocked[w] = b;
    }
    if (lane == 0) *found = kUnreached;
    __syncthreads();
    const int2 gij = g.goal[a];
    const bool goal_on_map = gij.x >= 1 && gij.x <= H && gij.y >= 1 && gij.y <= W;
    const int tg = goal_on_map ? (gij.x - 1) + H * (gij.y - 1) : 0;
    int tail = 0;
    if (goal_on_map && ((blocked[tg >> 5] >> (tg & 31)) & 1u) == 0u) {     // (a goal inside a wall: nothing is reached)
        __syncthreads();                                                   // every lane has read the bit
        if (lane == 0) { blocked[tg >> 5] |= 1u << (tg & 31); queue[0] = (uint16_t)tg; }
        tail = 1;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    int head = 0;
    for (uint32_t level = 0; head < tail; ++level) {                       // (head, tail, level: the same in every lane)
        const int level_end = tail;
        for (int base = head; base < level_end; base += kGoalBlock) {
            const int q = base + lane;
            const bool live = q < level_end;
            const int t = live ? (int)queue[q] : 0;
            if (live) {
                field[t] = (uint16_t)level;
                if (t == tp) *found = level;
            }
            const int step[4] = {-1, 1, -H, H};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int n = t + step[k];
                bool won = false;
                if (live && n >= 0 && n < HW) {                            // (a free tile is interior in every map the library accepts: the range is the guard, not the rule)
                    const uint32_t bit = 1u << (n & 31);
                    won = (atomicOr(&blocked[n >> 5], bit) & bit) == 0u;
                }
                const unsigned long long m = __ballot(won);
                if (won) queue[tail + __popcll(m & below)] = (uint16_t)n;  // (tail + count <= free tiles <= HW: each bit flips once)
                tail += __popcll(m);
            }
        }
        head = level_end;
        __syncthreads();                                                   // the level's appends, before the next level reads them
    }
    // walls and what the flood did not reach.  (`blocked` = walls | reached: a reached tile is blocked and no wall)
    for (int t = lane; t < HW; t += kGoalBlock) {
        const uint32_t wall = (tm[t >> 4] >> ((t & 15) * 2)) & 1u;
        const uint32_t reached_or_wall = (blocked[t >> 5] >> (t & 31)) & 1u;
        if (wall != 0u || reached_or_wall == 0u) field[t] = (uint16_t)kUnreached;
    }
    if (lane == 0) {
        const uint32_t f = *found;
        const int32_t now = f == kUnreached ? -1 : (int32_t)f;
        g.words.distance[a] = now;
        g.words.start_distance[a] = now;
        g.words.progress[a] = 0;
        g.last_episode[a] = ep;
    }
}

}  // namespace

size_t rcw_goal_distance_lds_bytes(const RcwDev& p)
{
    const size_t HW = (size_t)p.H * p.W;
    return (((HW + 31) >> 5) + 1) * sizeof(uint32_t) + ((HW + 1) & ~(size_t)1) * sizeof(uint16_t);
}

hipError_t rcw_launch_goal_distance(const RcwDev& p, int32_t B, const uint8_t* mask_dev, bool refill, uint16_t* field, const RcwGoalWords& words,
                                    uint32_t* last_episode, hipStream_t s)
{
    if (B < 1) return hipSuccess;
    const size_t lds = rcw_goal_distance_lds_bytes(p);
    if (lds > 64 * 1024) {                                                  // (maps from 181 x 181 up: a workgroup a CU)
        static std::mutex mu;
        static bool raised[64];
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (device < 0 || device >= 64 || !raised[device]) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rcw_goal_distance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            if (device >= 0 && device < 64) raised[device] = true;
        }
    }
    const GoalDistanceArgs g{B, p.H, p.W, p.nwords, p.real64, refill ? 1 : 0, p.pos, p.pos64, p.goal, p.episode, p.tile_map, mask_dev,
                             field, words, last_episode};
    hipLaunchKernelGGL(rcw_goal_distance_kernel, dim3(B), dim3(kGoalBlock), lds, s, g);
    return hipGetLastError();
}
