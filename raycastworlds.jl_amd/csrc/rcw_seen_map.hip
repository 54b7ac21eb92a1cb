// The seen map (include/rcw.h, rcw_set_seen_map): per agent the tiles its view rays have crossed since its episode began — UInt8 (H*W) in the
// tile map's linear order, 0 = not seen, else 1 + the tile's bits — and three Int32 words: how many are seen, how many the last call added,
// whether the goal tile is among them.  One kernel behind every step / reset / set_state / set_walls of a handle that enabled it; nothing
// else of the library knows about it.
//
// rcw_seen_map_kernel<T, TIE_LE>: ONE WORKGROUP PER AGENT, a lane a ray (rays tid, tid + block, ...).
//   LDS   the agent's tiles, a byte each (stage_tile_bytes: what the ray kernels march on), and `marked`, a bit per tile, zeroed.
//         H*W + H*W / 8 bytes: 1.1 KiB at 32 x 32, 71.7 KiB at the largest map rcw_create accepts (from 58,240 tiles the launch needs the
//         raised dynamic-LDS limit) — one path for every size.
//   march visit_ray below: cast_ray's march (rcw_device.h) select for select, without the distance, with one LDS atomic OR per tile the ray
//         is on — the player's tile through the stop tile.  The result of the OR is not used: no lane waits for it.
//   fold  behind a barrier, a lane a bitmap word: fresh = marked & ~seen against the agent's packed `seen` bits in HBM (taken as zero for an
//         agent that is being cleared), a map byte written for every fresh bit, the word's popcount.  A cleared agent's whole map is
//         rewritten instead, a lane a byte.  The lane that holds the goal tile's word writes goal_seen.
//   sum   the popcounts: across the wavefront with shuffles, across wavefronts through LDS; lane 0 writes the words and the counter.
// An agent is cleared when it is in the mask of a refill launch, or its episode counter is not the one recorded at its last clear
// (auto_reset re-sampled it in the step in front).
#include "rcw_device.h"

namespace {

constexpr int kSeenBlock = 256;

struct SeenMapArgs {
    int32_t B, H, W, N, nwords, refill;
    const void* pos;             // float2 / double2 [B]
    const int32_t* dir;
    const int2* goal;
    const uint32_t* episode;
    const uint32_t* tile_map;
    const void* ray_table;       // [nd][RCW_TABLE_ROWS][N] in T
    const uint8_t* mask;
    uint8_t* map;                // [B][H*W]
    uint32_t* seen;              // [B][(H*W + 31) / 32]
    RcwSeenWords words;
    uint32_t* last_episode;      // [B] the episode counter the agent's map was last cleared in
};

// RayCaster.cast_ray's march (cast_ray, rcw_device.h: the same selects in the same order, so the same tiles) with a visitor: the bit of
// every tile the ray is on — the start tile, every tile stepped to, the stop tile — is set in `marked`.  An index outside [0, H*W) reads
// and marks the LAST tile, which stage_tile_bytes made an obstacle: such a ray ends there, and nothing outside the agent's arrays is touched.
template <typename T, bool TIE_LE>
__device__ __forceinline__ void visit_ray(const uint8_t* tb, uint32_t* marked, int H, int W, T x, T y, T dx, T dy, T ddx, T ddy)
{
    const int i0 = (int)rfloor(x) + 1;    // wu_to_tu UT:5
    const int j0 = (int)rfloor(y) + 1;
    const bool neg_x = dx < (T)0, neg_y = dy < (T)0;
    const int si = neg_x ? -1 : 1;
    const int tj = neg_y ? -H : H;
    const T fx = neg_x ? x - (T)(i0 - 1) : (T)i0 - x;
    const T fy = neg_y ? y - (T)(j0 - 1) : (T)j0 - y;
    T sx = fx * ddx, sy = fy * ddy;
    int t = (i0 - 1) + H * (j0 - 1);
    const unsigned last = (unsigned)(H * W - 1);
    unsigned u = (unsigned)t < last ? (unsigned)t : last;                     // never outside the map
    uint32_t bits = tb[u];
    atomicOr(&marked[u >> 5], 1u << (u & 31u));
    while (bits == 0u) {
        const bool xf = TIE_LE ? (sx <= sy) : (sx < sy);
        const T nx = sx + ddx, ny = sy + ddy;
        sx = xf ? nx : sx;
        sy = xf ? sy : ny;
        t += xf ? si : tj;
        u = (unsigned)t < last ? (unsigned)t : last;
        bits = tb[u];
        atomicOr(&marked[u >> 5], 1u << (u & 31u));
    }
}

template <typename T, bool TIE_LE>
__global__ __launch_bounds__(kSeenBlock) void rcw_seen_map_kernel(const SeenMapArgs g)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_s[];
    const int a = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    if (a >= g.B) return;
    if (g.refill && g.mask != nullptr && g.mask[a] == 0) return;          // an agent outside the call's mask keeps every byte
    const uint32_t ep = g.episode[a];
    const bool clear = g.refill || g.last_episode[a] != ep;
    const int H = g.H, W = g.W, HW = H * W;
    const int bwords = (HW + 31) >> 5, tile_words = (HW + 3) >> 2;
    uint8_t* const tb = reinterpret_cast<uint8_t*>(lds_s);                 // [HW]
    uint32_t* const marked = lds_s + tile_words;                           // [bwords]
    uint32_t* const partial = marked + bwords;                             // [kSeenBlock / 64]
    const uint32_t* const tm = g.tile_map + (size_t)a * g.nwords;
    stage_tile_bytes(tb, tm, HW, tid, nthreads);
    for (int w = tid; w < bwords; w += nthreads) marked[w] = 0u;
    __syncthreads();

    // the player's tile: off the map (also a NaN) marks nothing
    const typename Real<T>::vec2 pos = static_cast<const typename Real<T>::vec2*>(g.pos)[a];
    const T fx = rfloor(pos.x), fy = rfloor(pos.y);
    if (fx >= (T)0 && fx < (T)H && fy >= (T)0 && fy < (T)W) {
        const T* const tab = static_cast<const T*>(g.ray_table) + (size_t)g.dir[a] * RCW_TABLE_ROWS * g.N;
        for (int i = tid; i < g.N; i += nthreads)
            visit_ray<T, TIE_LE>(tb, marked, H, W, pos.x, pos.y, tab[i], tab[g.N + i], tab[2 * g.N + i], tab[3 * g.N + i]);
    }
    __syncthreads();

    // ---- the fold ----------------------------------------------------------------------------------------------------------------
    uint8_t* const map = g.map + (size_t)a * HW;
    uint32_t* const seen = g.seen + (size_t)a * bwords;
    const int2 gij = g.goal[a];
    const bool goal_on_map = gij.x >= 1 && gij.x <= H && gij.y >= 1 && gij.y <= W;
    const int tg = goal_on_map ? (gij.x - 1) + H * (gij.y - 1) : -1;
    int count = 0;
    for (int w = tid; w < bwords; w += nthreads) {
        const uint32_t m = marked[w];
        const uint32_t old = clear ? 0u : seen[w];
        uint32_t fresh = m & ~old;
        count += __popc(fresh);
        if (clear || fresh != 0u) seen[w] = old | m;
        if (tg >= 0 && (tg >> 5) == w) g.words.goal_seen[a] = (int32_t)(((old | m) >> (tg & 31)) & 1u);
        if (!clear) {
            while (fresh != 0u) {                                          // (bits past the map are never marked)
                const int t = (w << 5) + (__ffs(fresh) - 1);
                map[t] = (uint8_t)(1u + ((tm[t >> 4] >> ((t & 15) * 2)) & 3u));
                fresh &= fresh - 1u;
            }
        }
    }
    if (clear) {
        for (int t = tid; t < HW; t += nthreads) {                         // the whole map, coalesced
            const uint32_t on = (marked[t >> 5] >> (t & 31)) & 1u;
            map[t] = (uint8_t)(on ? 1u + ((tm[t >> 4] >> ((t & 15) * 2)) & 3u) : 0u);
        }
    }

    // ---- the sum -----------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
    if ((tid & 63) == 0) partial[tid >> 6] = (uint32_t)count;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < (nthreads + 63) >> 6; ++k) total += (int)partial[k];
        g.words.seen_count[a] = clear ? total : g.words.seen_count[a] + total;
        g.words.newly_seen[a] = clear ? 0 : total;
        if (tg < 0) g.words.goal_seen[a] = 0;
        if (clear) g.last_episode[a] = ep;
    }
}

template <typename T, bool TIE_LE>
hipError_t launch(const SeenMapArgs& g, int block, size_t lds, int which, hipStream_t s)
{
    if (lds > 64 * 1024) {                                                  // (maps from 58,240 tiles up)
        static std::mutex mu;
        static bool raised[4][64];
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (device < 0 || device >= 64 || !raised[which][device]) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rcw_seen_map_kernel<T, TIE_LE>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
            if (e != hipSuccess) return e;
            if (device >= 0 && device < 64) raised[which][device] = true;
        }
    }
    hipLaunchKernelGGL((rcw_seen_map_kernel<T, TIE_LE>), dim3(g.B), dim3(block), lds, s, g);
    return hipGetLastError();
}

}  // namespace

size_t rcw_seen_map_lds_bytes(const RcwDev& p)
{
    const size_t HW = (size_t)p.H * p.W;
    return (((HW + 3) >> 2) + ((HW + 31) >> 5) + kSeenBlock / 64) * sizeof(uint32_t);
}

hipError_t rcw_launch_seen_map(const RcwDev& p, int32_t B, const uint8_t* mask_dev, bool refill, uint8_t* map, uint32_t* seen_bits,
                               const RcwSeenWords& words, uint32_t* last_episode, hipStream_t s)
{
    if (B < 1) return hipSuccess;
    const size_t lds = rcw_seen_map_lds_bytes(p);
    const int block = p.N >= kSeenBlock ? kSeenBlock : ((p.N + 63) & ~63);   // a lane a ray, whole wavefronts
    const SeenMapArgs g{B, p.H, p.W, p.N, p.nwords, refill ? 1 : 0, p.real64 ? (const void*)p.pos64 : (const void*)p.pos, p.dir, p.goal, p.episode,
                        p.tile_map, p.real64 ? (const void*)p.ray_table64 : (const void*)p.ray_table, mask_dev, map, seen_bits, words, last_episode};
    if (p.real64) return p.tie_le ? launch<double, true>(g, block, lds, 3, s) : launch<double, false>(g, block, lds, 2, s);
    return p.tie_le ? launch<float, true>(g, block, lds, 1, s) : launch<float, false>(g, block, lds, 0, s);
}
