// The frontier (include/rcw.h, rcw_set_frontier): per agent the breadth-first distance field to the nearest unseen tile that borders a seen
// passable one — UInt16 (H*W) in the seen map's order — and two Int32 words: the field at the player's tile, and the number of such tiles
// as of the agent's last flood.  One kernel directly behind the seen map's on a handle that enabled it; the action words follow from one
// launch of the guide's kernel on this field (rcw_launch_guide).  Nothing else of the library knows about it.
//
// rcw_frontier_kernel: ONE WAVEFRONT PER AGENT, the goal distance's decomposition (rcw_goal_distance.hip: a 64-thread workgroup, every
// __syncthreads orders the wave's own LDS traffic).  An agent whose field is current — its episode counter is the recorded one and the seen
// map's launch in front added nothing to its map — reads its position and one field entry and writes one word.  Every other agent floods:
//   bits    the agent's map bytes are read ONCE, coalesced: sixteen at a time (a 128-bit load a lane, 1 KiB a wavefront) where the agent's
//           map begins on a multiple of 16 bytes, else a byte a lane.  They become three bitmaps in LDS: `pass` (bytes 1 and 3), `unseen`
//           (byte 0) — both constant from here on — and `blocked` = ~pass, to which the flood adds what it reaches.
//   seeds   a lane a tile: a source is an unseen tile with a passable edge neighbour ON THE MAP — tile (H-1, j) and tile (0, j+1) are one
//           apart in linear order and no neighbours; the row comes from a multiply-high by ceil(2^32 / H), exact below 2^16.  ALL sources
//           enter the queue behind a ballot prefix, as level 0; their number is `tiles`.  The same pass writes 0xFFFF to every tile that is
//           neither passable nor a source: the flood never touches those.
//   flood   the goal distance's: a level is the queue segment [head, level_end), a lane a tile, the neighbours claimed with an LDS atomic OR
//           on `blocked` and appended behind a ballot prefix; the field is only ever WRITTEN (a tile's value is the level at which it leaves
//           the queue), so the values do not depend on the order within a level.  A source is blocked from the start and is never claimed;
//           a neighbour is looked at only where it lies on the map, by the same row test.
//   rest    0xFFFF to the passable tiles the flood did not reach.  The three sets of stores are disjoint.
// LDS: 3 (H*W / 8) + 2 H*W bytes: 2.4 KiB at 32 x 32, 151.4 KiB at the largest map rcw_create accepts — one path for every size.
#include "rcw_device.h"

namespace {

constexpr int kFrontierBlock = 64;        // one wavefront
constexpr uint32_t kFrontierUnreached = 0xFFFFu;

struct FrontierArgs {
    int32_t B, H, W, real64, refill;
    uint32_t row_magic;          // ceil(2^32 / H): t / H == mulhi(t, row_magic) for t < 2^16
    const float2* pos;
    const double2* pos64;
    const uint32_t* episode;
    const uint8_t* mask;
    const uint8_t* map;          // [B][H*W] the seen map
    const int32_t* newly_seen;   // [B] what the seen map's launch in front added
    uint16_t* field;             // [B][H*W]
    int32_t* distance;           // [B]
    int32_t* tiles;              // [B]
    uint32_t* last_episode;      // [B] the episode counter the agent's field was flooded in
};

// bit k of the result = byte k of x is zero (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x)
{
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in every zero byte
    return (((z >> 7) * 0x01020408u) >> 24) & 0xFu;
}
// of four map bytes: bits 0..3 the passable ones (1 or 3: everything but bit 1 equals 1), bits 16..19 the unseen ones (0)
__device__ __forceinline__ uint32_t classify4(uint32_t x)
{
    return zero_bytes((x ^ 0x01010101u) & 0xFDFDFDFDu) | (zero_bytes(x) << 16);
}

__global__ __launch_bounds__(kFrontierBlock) void rcw_frontier_kernel(const FrontierArgs g)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_f[];
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= g.B) return;
    if (g.refill && g.mask != nullptr && g.mask[a] == 0) return;          // an agent outside the call's mask keeps every byte
    const uint32_t ep = g.episode[a];
    const bool stale = g.refill || g.last_episode[a] != ep || g.newly_seen[a] != 0;
    const int H = g.H, W = g.W, HW = H * W;
    // the player's tile, 0-based; -1: off the map (also a NaN)
    double x, y;
    if (g.real64) { const double2 q = g.pos64[a]; x = q.x; y = q.y; }
    else          { const float2 q = g.pos[a]; x = (double)q.x; y = (double)q.y; }
    const double fx = floor(x), fy = floor(y);
    const bool on_map = fx >= 0.0 && fx < (double)H && fy >= 0.0 && fy < (double)W;
    const int tp = on_map ? (int)fx + H * (int)fy : -1;
    uint16_t* const field = g.field + (size_t)a * HW;

    if (!stale) {
        if (lane == 0) {
            const uint32_t f = tp >= 0 ? (uint32_t)field[tp] : kFrontierUnreached;
            g.distance[a] = f == kFrontierUnreached ? -1 : (int32_t)f;
        }
        return;
    }

    // ---- the bitmaps ---------------------------------------------------------------------------------------------------------------
    const int bwords = (HW + 31) >> 5;
    uint32_t* const pass = lds_f;                                          // [bwords]
    uint32_t* const unseen = lds_f + bwords;                               // [bwords]
    uint32_t* const blocked = lds_f + 2 * bwords;                          // [bwords]
    uint32_t* const found = lds_f + 3 * bwords;                            // the player's distance, once its tile is popped
    uint16_t* const queue = reinterpret_cast<uint16_t*>(lds_f + 3 * bwords + 1);   // [HW]
    const uint8_t* const map = g.map + (size_t)a * HW;
    if ((reinterpret_cast<uintptr_t>(map) & 15u) == 0u) {
        // sixteen tiles a lane: half a bitmap word (little-endian: half h of the bitmap holds tiles 16 h .. 16 h + 15)
        uint16_t* const pass16 = reinterpret_cast<uint16_t*>(pass);
        uint16_t* const unseen16 = reinterpret_cast<uint16_t*>(unseen);
        uint16_t* const blocked16 = reinterpret_cast<uint16_t*>(blocked);
        const int whole = HW >> 4;
        for (int c = lane; c < 2 * bwords; c += kFrontierBlock) {
            uint32_t p = 0u, u = 0u;
            if (c < whole) {
                const uint4 v = reinterpret_cast<const uint4*>(map)[c];
                const uint32_t k0 = classify4(v.x), k1 = classify4(v.y), k2 = classify4(v.z), k3 = classify4(v.w);
                p = (k0 & 0xFu) | ((k1 & 0xFu) << 4) | ((k2 & 0xFu) << 8) | ((k3 & 0xFu) << 12);
                u = (k0 >> 16) | ((k1 >> 16) << 4) | ((k2 >> 16) << 8) | ((k3 >> 16) << 12);
            } else {
                for (int t = c << 4; t < HW; ++t) {                        // (the map's last H*W % 16 bytes; nothing past the map)
                    const uint32_t v = map[t];
                    p |= (uint32_t)((v & 0xFDu) == 1u) << (t & 15);
                    u |= (uint32_t)(v == 0u) << (t & 15);
                }
            }
            pass16[c] = (uint16_t)p;
            unseen16[c] = (uint16_t)u;
            blocked16[c] = (uint16_t)~p;                                   // (past the map: blocked)
        }
    } else {
        for (int base = 0; base < HW; base += kFrontierBlock) {           // a byte a lane, two bitmap words a pass
            const int t = base + lane;
            const uint32_t v = t < HW ? (uint32_t)map[t] : 0xFFu;
            const unsigned long long p = __ballot((v & 0xFDu) == 1u), u = __ballot(v == 0u);
            if (lane < 2 && (base >> 5) + lane < bwords) {
                const uint32_t pw = (uint32_t)(p >> (32 * lane));
                pass[(base >> 5) + lane] = pw;
                unseen[(base >> 5) + lane] = (uint32_t)(u >> (32 * lane));
                blocked[(base >> 5) + lane] = ~pw;
            }
        }
    }
    if (lane == 0) *found = kFrontierUnreached;
    __syncthreads();

    // ---- the seeds -----------------------------------------------------------------------------------------------------------------
    const unsigned long long below = (1ull << lane) - 1ull;
    const auto bit = [](const uint32_t* m, int t) { return (m[t >> 5] >> (t & 31)) & 1u; };
    int tail = 0;
    for (int base = 0; base < HW; base += kFrontierBlock) {
        const int t = base + lane;
        bool src = false;
        if (t < HW) {
            const bool p = bit(pass, t) != 0u;
            if (!p && bit(unseen, t) != 0u) {
                const int j = (int)__umulhi((uint32_t)t, g.row_magic), i = t - j * H;
                src = (i > 0 && bit(pass, t - 1) != 0u) || (i < H - 1 && bit(pass, t + 1) != 0u) ||
                      (j > 0 && bit(pass, t - H) != 0u) || (j < W - 1 && bit(pass, t + H) != 0u);
            }
            if (!p && !src) field[t] = (uint16_t)kFrontierUnreached;
        }
        const unsigned long long m = __ballot(src);
        if (src) queue[tail + __popcll(m & below)] = (uint16_t)t;         // (sources + passable tiles <= HW: the queue holds them all)
        tail += __popcll(m);
    }
    const int sources = tail;
    __syncthreads();

    // ---- the flood -----------------------------------------------------------------------------------------------------------------
    int head = 0;
    for (uint32_t level = 0; head < tail; ++level) {                       // (head, tail, level: the same in every lane)
        const int level_end = tail;
        for (int base = head; base < level_end; base += kFrontierBlock) {
            const int q = base + lane;
            const bool live = q < level_end;
            const int t = live ? (int)queue[q] : 0;
            if (live) {
                field[t] = (uint16_t)level;
                if (t == tp) *found = level;
            }
            const int j = (int)__umulhi((uint32_t)t, g.row_magic), i = t - j * H;
            const int step[4] = {-1, 1, -H, H};
            const bool there[4] = {i > 0, i < H - 1, j > 0, j < W - 1};    // the neighbour lies on the map: 0 <= n < HW
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int n = t + step[k];
                bool won = false;
                if (live && there[k]) {
                    const uint32_t b = 1u << (n & 31);
                    won = (atomicOr(&blocked[n >> 5], b) & b) == 0u;
                }
                const unsigned long long m = __ballot(won);
                if (won) queue[tail + __popcll(m & below)] = (uint16_t)n;  // (each bit flips once)
                tail += __popcll(m);
            }
        }
        head = level_end;
        __syncthreads();                                                   // the level's appends, before the next level reads them
    }
    // the passable tiles no source can be reached from
    for (int t = lane; t < HW; t += kFrontierBlock)
        if (bit(pass, t) != 0u && bit(blocked, t) == 0u) field[t] = (uint16_t)kFrontierUnreached;
    if (lane == 0) {
        const uint32_t f = *found;
        g.distance[a] = f == kFrontierUnreached ? -1 : (int32_t)f;
        g.tiles[a] = sources;
        g.last_episode[a] = ep;
    }
}

}  // namespace

size_t rcw_frontier_lds_bytes(const RcwDev& p)
{
    const size_t HW = (size_t)p.H * p.W;
    return (3 * ((HW + 31) >> 5) + 1) * sizeof(uint32_t) + ((HW + 1) & ~(size_t)1) * sizeof(uint16_t);
}

hipError_t rcw_launch_frontier(const RcwDev& p, int32_t B, const uint8_t* mask_dev, bool refill, const uint8_t* seen_map, const int32_t* newly_seen,
                               uint16_t* field, const RcwFrontierWords& words, uint32_t* last_episode, hipStream_t s)
{
    if (B < 1) return hipSuccess;
    if (p.H < 2 || p.W < 1 || (int64_t)p.H * p.W > 65535) return hipErrorInvalidValue;   // (UInt16 tile indices, row_magic; rcw_create accepts less)
    const size_t lds = rcw_frontier_lds_bytes(p);
    if (lds > 64 * 1024) {                                                  // (a workgroup a CU)
        static std::mutex mu;
        static bool raised[64];
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (device < 0 || device >= 64 || !raised[device]) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rcw_frontier_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            if (device >= 0 && device < 64) raised[device] = true;
        }
    }
    const uint32_t row_magic = (uint32_t)(((1ull << 32) + (uint64_t)p.H - 1) / (uint64_t)p.H);   // (H >= 2: it fits)
    const FrontierArgs g{B, p.H, p.W, p.real64, refill ? 1 : 0, row_magic, p.pos, p.pos64, p.episode, mask_dev, seen_map, newly_seen,
                         field, words.distance, words.tiles, last_episode};
    hipLaunchKernelGGL(rcw_frontier_kernel, dim3(B), dim3(kFrontierBlock), lds, s, g);
    return hipGetLastError();
}
