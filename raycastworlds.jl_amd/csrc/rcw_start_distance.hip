// The start rule (include/rcw.h, rcw_set_start_distance): an agent that began an episode is placed on a tile whose shortest-path distance to
// its goal lies in the handle's band [lo, hi] — or, where the band lies beyond what can be reached, on one of the farthest tiles.  One kernel
// directly behind the layout source's launch point, at every call that can move an episode counter; nothing else of the library knows about it.
//
// rcw_start_distance_kernel: ONE WAVEFRONT PER AGENT (a 64-thread workgroup: every __syncthreads below orders the wave's own LDS traffic and
// costs no barrier instruction).  The usual case — the agent has begun no episode — reads two words (its counter and the recorded one),
// writes mask[a] = 0 and leaves.  An agent whose counter moved (force: every agent) floods from its goal, in LDS only:
//   LDS   `blocked`, a bit per tile (walls, then also what the flood has reached), and `queue`, the tile indices in the order reached
//         (UInt16: H*W <= 65280; every tile enters at most once).  H*W / 8 + 2 H*W bytes, the goal distance's own request: 135.5 KiB at the
//         largest map rcw_create accepts — one path for every size.  No field is written and none is read: the handle needs no goal distance.
//   the band   The queue is sorted by distance, so the tiles of [lo, hi] are ONE segment of it: it opens where level lo begins and closes
//         where level hi ends — the flood stops there, level hi is never expanded — or where the flood ends.  A flood that ends below lo
//         leaves the segment of its last level, the clamp.
//   the draw   Where a tile lies INSIDE a level depends on which lane won an LDS atomic, so the queue's order must not reach the result: the
//         segment's tiles are marked in a bitmap (the words of `blocked`, free by then), and the r-th set bit in ascending tile order is
//         found with per-lane popcounts over a contiguous run of words, a wave prefix, and a walk of the one lane that holds it.
// ONE lane — the lane whose run of words holds the r-th set bit; lane 0 where the drawn pose is kept — writes the pose (plain vector
// stores), placed[a], the recorded counter and mask[a] = 1: the host re-casts and repaints the masked agents through the existing masked path.
#include "rcw_device.h"

namespace {

constexpr int kStartBlock = 64;            // one wavefront
constexpr uint64_t kStartDraw = 0xC000000000000000ull;   // (reset_agent's indices count from 0, the layout sources take 2^63)

// bit t of the result = bit 2 t of x (the WALL layer of 16 tiles of a tile-map word)
__device__ __forceinline__ uint32_t wall_bits(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

struct StartArgs {
    int32_t B, H, W, nwords, real64, force;
    uint32_t lo, hi;
    uint64_t seed;
    int64_t agent_id_offset;
    float2* pos;
    double2* pos64;
    const int2* goal;
    const uint32_t* episode;
    const uint32_t* tile_map;
    RcwStartRule rule;
};

__global__ __launch_bounds__(kStartBlock) void rcw_start_distance_kernel(const StartArgs g)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_s[];
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= g.B) return;
    const uint32_t ep = g.episode[a];
    if (!g.force && g.rule.last_episode[a] == ep) {
        if (lane == 0) g.rule.mask[a] = 0;
        return;
    }
    const int H = g.H, W = g.W, HW = H * W;

    // ---- the flood (rcw_goal_distance_kernel's, without the field) ------------------------------------------------------------------
    const int bwords = (HW + 31) >> 5;
    uint32_t* const blocked = lds_s;                                       // [bwords]
    uint16_t* const queue = reinterpret_cast<uint16_t*>(lds_s + bwords);   // [HW]
    const uint32_t* const tm = g.tile_map + (size_t)a * g.nwords;
    for (int w = lane; w < bwords; w += kStartBlock) {                     // (nwords is even and >= HW / 16: 2 w + 1 is inside)
        uint32_t b = wall_bits(tm[2 * w]) | (wall_bits(tm[2 * w + 1]) << 16);
        if (w == bwords - 1 && (HW & 31) != 0) b |= ~0u << (HW & 31);      // past the map: blocked
        blocked[w] = b;
    }
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
    int seg_first = -1, seg_end = 0;                                       // the band's segment of the queue; -1: level lo was not reached
    int last_first = 0;                                                    // where the last level that had tiles begins
    uint32_t levels = 0;                                                   // levels that had tiles: the largest distance is levels - 1
    for (uint32_t level = 0; head < tail; ++level) {                       // (head, tail, level: the same in every lane)
        const int level_end = tail;
        last_first = head;
        levels = level + 1u;
        if (level == g.lo) seg_first = head;
        if (level == g.hi) break;                                          // level hi is complete: nothing beyond it is wanted
        for (int base = head; base < level_end; base += kStartBlock) {
            const int q = base + lane;
            const bool live = q < level_end;
            const int t = live ? (int)queue[q] : 0;
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
    // the band's segment ends where level hi ends (the break: tail is that level's end) or where the flood ended
    seg_end = tail;
    uint32_t outcome = 1u;
    if (seg_first < 0) {                                                   // the band is empty: the farthest tiles, if any lie beyond the goal
        outcome = levels >= 2u ? 2u : 3u;
        seg_first = last_first;
    }
    if (outcome == 3u) {                                                   // the pose reset_agent drew stays
        if (lane == 0) { g.rule.placed[a] = 3; g.rule.last_episode[a] = ep; g.rule.mask[a] = 1; }
        return;
    }

    // ---- the segment's tiles as a bitmap, in the words of `blocked` -------------------------------------------------------------------
    __syncthreads();
    for (int w = lane; w < bwords; w += kStartBlock) blocked[w] = 0u;
    __syncthreads();
    for (int q = seg_first + lane; q < seg_end; q += kStartBlock) {
        const int t = (int)queue[q];
        atomicOr(&blocked[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    const uint32_t n = (uint32_t)(seg_end - seg_first);                    // >= 1
    const uint64_t key = rcw_episode_key(g.seed, (uint64_t)(g.agent_id_offset + a), (uint64_t)(ep - 1u));   // (the episode the agent began: the counter before its increment)
    const uint32_t r = (uint32_t)rcw_below(rcw_draw(key, kStartDraw), (uint64_t)n);
    // the r-th set bit in ascending tile order: lane l counts words [l * run, (l + 1) * run)
    const int run = (bwords + kStartBlock - 1) / kStartBlock;
    const int w0 = lane * run, w1 = min(w0 + run, bwords);
    uint32_t mine = 0u;
    for (int w = w0; w < w1; ++w) mine += (uint32_t)__popc(blocked[w]);
    uint32_t incl = mine;                                                  // inclusive prefix over the wave
#pragma unroll
    for (int d = 1; d < kStartBlock; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, kStartBlock);
        if (lane >= d) incl += up;
    }
    const uint32_t excl = incl - mine;
    if (r >= excl && r < incl) {                                           // exactly one lane (the counts sum to n > r)
        uint32_t left = r - excl;
        int t = -1;
        for (int w = w0; w < w1; ++w) {
            uint32_t bits = blocked[w];
            const uint32_t c = (uint32_t)__popc(bits);
            if (left >= c) { left -= c; continue; }
            for (; left > 0u; --left) bits &= bits - 1u;                   // drop the `left` lowest set bits
            t = 32 * w + (int)__builtin_ctz(bits);
            break;
        }
        if (t >= 0 && t < HW) {
            const int j = t / H, i = t - j * H;                            // 0-based; the tile's centre as reset_agent writes one
            const double cx = (double)(i + 1) - 0.5, cy = (double)(j + 1) - 0.5;
            if (g.real64) g.pos64[a] = make_double2(cx, cy);
            else          g.pos[a] = make_float2((float)cx, (float)cy);
        }
        g.rule.placed[a] = (uint8_t)outcome;
        g.rule.last_episode[a] = ep;
        g.rule.mask[a] = 1;
    }
}

}  // namespace

size_t rcw_start_distance_lds_bytes(const RcwDev& p)
{
    const size_t HW = (size_t)p.H * p.W;
    return ((HW + 31) >> 5) * sizeof(uint32_t) + ((HW + 1) & ~(size_t)1) * sizeof(uint16_t);
}

hipError_t rcw_launch_start_distance(const RcwDev& p, const RcwStartRule& rule, uint32_t lo, uint32_t hi, bool force, hipStream_t s)
{
    if (p.B < 1) return hipSuccess;
    const size_t lds = rcw_start_distance_lds_bytes(p);
    if (lds > 64 * 1024) {                                                  // (maps from 181 x 181 up: a workgroup a CU)
        static std::mutex mu;
        static bool raised[64];
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (device < 0 || device >= 64 || !raised[device]) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rcw_start_distance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            if (device >= 0 && device < 64) raised[device] = true;
        }
    }
    const StartArgs g{p.B, p.H, p.W, p.nwords, p.real64, force ? 1 : 0, lo, hi, p.seed, p.agent_id_offset, p.pos, p.pos64, p.goal, p.episode,
                      p.tile_map, rule};
    hipLaunchKernelGGL(rcw_start_distance_kernel, dim3(p.B), dim3(kStartBlock), lds, s, g);
    return hipGetLastError();
}
