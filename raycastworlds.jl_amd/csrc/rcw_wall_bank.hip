// The layout sources (rcw_kernels.h, "THE LAYOUT SOURCES"): ONE launch point, rcw_launch_layout_source — behind the core launches of every
// call that can move an episode counter — and behind it one of four restart kernels, by the kind of the handle's live source:
//   rcw_wall_bank_kernel<T>        the wall bank: layout k of L resident on the device, k drawn by the weights
//   rcw_wall_generator_kernel<T>   mazes: a spanning tree of the odd sub-grid, made in LDS (maze_in_lds)
//   rcw_wall_caves_kernel<T>       caves: a smoothed random fill pruned to its largest region, made in LDS; the maze where that is too small
//   rcw_wall_rooms_kernel<T>       rooms: the interior split recursively by walls with doors, made in LDS
// Nothing else of the library knows where a layout comes from.  What the four share:
//   the shape   ONE WAVEFRONT PER AGENT (a 64-thread workgroup: every __syncthreads below orders the wave's own LDS traffic and costs no
//               barrier instruction), the episode's layout in LDS in the tile map's own word format — nwords uint32 an agent, 16 tiles a
//               word, bit 0 of each 2-bit field = WALL, the GOAL bits and the padding past H*W clear (what rcw_set_walls_kernel writes);
//   no_restart  the opening.  The usual case — the agent has not begun an episode — reads two words (its counter and the recorded one),
//               writes mask[a] = 0 and leaves.  An agent whose counter moved (by one: the kernel runs behind every such call) began episode
//               e = counter - 1 in the launch in front, against the walls it had; that reset is discarded;
//   the key     draw 2^63 of the episode's key — reset_agent's own indices count from 0 and stay far below —: the bank scales it to the
//               weights' sum and looks it up in the cumulative weights by binary search (uniform: scalar registers, log2 L loads), a family
//               takes it as the layout's key, or picks a level with it and takes the level's key (layout_key);
//   restart_on_lds_words   the tail.  Lane 0 puts the counter back to e and runs reset_agent against the LDS words: the SAME key, draw
//               indices from 0 — the rejection loops are sequential per agent, so one lane runs them, as in rcw_reset_kernel —, which writes
//               goal, pose, heading, reward, done and the counter e + 1; then the time limit's two words, wall_layout[a], the recorded
//               counter.  The wave copies the LDS words (walls + the new goal bit) over the agent's tile map, coalesced: the tile map in HBM
//               is only ever written whole, no read-modify-write meets the copy;
//   mask[a] = 1 the host re-casts the masked agents through the existing masked path and repaints their camera view with
//               rcw_wall_bank_paint_kernel below (a handle with a top view: through the existing masked fill, which may carry the drawing).
// The discarded reset leaves one possible trace, the sticky status word (RCW_WARN_SAMPLER_GAVE_UP is set only over 0).  `status_seen` holds
// each agent's status word as of its last start here (rcw_clear_error zeroes it with the words): a warning that is there now and was not
// then can only be the discarded reset's — the restarted agent's action was ignored, no other writer ran — and is taken back before the
// real reset may set its own.
// Beside them, the bank's two other kernels:
//   rcw_wall_bank_pack_kernel   once per rcw_set_wall_bank: the layouts, UInt8 (H*W, L) as rcw_set_walls takes them, into the word format.  A
//               thread a word, 16 byte loads each: paid once, not per episode;
//   rcw_wall_bank_paint_kernel  the camera view of the agents a launch restarted.
#include "rcw_device.h"

namespace {

constexpr int kBankBlock = 64;            // one wavefront
constexpr uint64_t kLayoutDraw = 0x8000000000000000ull;

__global__ void rcw_wall_bank_pack_kernel(const uint8_t* __restrict__ walls, uint32_t* __restrict__ words, int HW, int nwords, long long total)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long long m = g / nwords;
    const int w = (int)(g - m * nwords);
    const uint8_t* const layout = walls + (size_t)m * (size_t)HW;
    uint32_t word = 0u;
    for (int k = 0; k < 16; ++k) {
        const int t = 16 * w + k;
        if (t < HW && layout[t] != 0) word |= 1u << (2 * k);
    }
    words[g] = word;
}

// The opening of the four restart kernels, behind the loads of the agent's counter ep: has the agent begun no episode since its last start
// here (and is not every agent restarted: force)?  Then mask[a] = 0 and the wave leaves.
__device__ __forceinline__ bool no_restart(const RcwWallBank& b, int force, int a, int lane, uint32_t ep)
{
    if (!force && b.last_episode[a] == ep) {
        if (lane == 0) b.mask[a] = 0;
        return true;
    }
    return false;
}

// Word w of a layout whose every tile is WALL: the tiles of the word inside the map set, the padding clear (nwords is even: a whole word may
// be padding).
__device__ __forceinline__ uint32_t all_wall_word(int HW, int w)
{
    const int left = HW - 16 * w;
    return left >= 16 ? 0x55555555u : left <= 0 ? 0u : (0x55555555u & ((1u << (2 * left)) - 1u));
}

// The tail the four restart kernels share, behind a barrier: the episode's layout (WALL bits, nothing else) lies in lds_w.
// Lane 0 takes back the discarded reset's status, puts the counter back to e = ep - 1 and runs reset_agent against the LDS words; then the
// wave copies them over the agent's tile map.  k: what wall_layout[a] says.
template <typename T>
__device__ __forceinline__ void restart_on_lds_words(const RcwDev& p, const RcwLimit& lim, const RcwWallBank& b, int a, int lane, uint32_t* lds_w,
                                                     uint32_t ep, int k)
{
    if (lane == 0) {
        if (p.status[a] == RCW_WARN_SAMPLER_GAVE_UP && b.status_seen[a] != RCW_WARN_SAMPLER_GAVE_UP) p.status[a] = 0;
        p.episode[a] = ep - 1u;
        reset_agent<T>(p, a, lds_w, nullptr);                              // (reads the counter back: e; leaves e + 1)
        lim.episode_steps[a] = 0u;
        lim.truncated[a] = 0;
        b.status_seen[a] = p.status[a];
        b.layout[a] = k;
        b.last_episode[a] = ep;
        b.mask[a] = 1;
    }
    __syncthreads();
    uint32_t* const tm = p.tile_map + (size_t)a * (size_t)p.nwords;
    for (int w = lane; w < p.nwords; w += kBankBlock) tm[w] = lds_w[w];
}

template <typename T>
__global__ __launch_bounds__(kBankBlock) void rcw_wall_bank_kernel(const RcwDev p, const RcwLimit lim, const RcwWallBank b, const int force)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_b[];
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= p.B) return;
    const uint32_t ep = p.episode[a];
    if (no_restart(b, force, a, lane, ep)) return;
    // the layout of episode e = ep - 1 (the counter before the increment the launch in front made)
    const uint32_t e = ep - 1u;
    const uint64_t key = rcw_episode_key(p.seed, (uint64_t)(p.agent_id_offset + a), (uint64_t)e);
    const uint32_t total = b.cum[b.layouts - 1];
    const uint32_t r = (uint32_t)rcw_below(rcw_draw(key, kLayoutDraw), (uint64_t)total);
    int lo = 0, hi = b.layouts - 1;                                        // the smallest k with cum[k] > r (r < total = cum[L - 1])
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (b.cum[mid] > r) hi = mid; else lo = mid + 1;
    }
    const int k = lo;
    const uint32_t* const src = b.words + (size_t)k * (size_t)p.nwords;
    for (int w = lane; w < p.nwords; w += kBankBlock) lds_b[w] = src[w];
    __syncthreads();
    restart_on_lds_words<T>(p, lim, b, a, lane, lds_b, ep, k);
}

// ---- mazes (include/rcw.h, "the wall generator") ------------------------------------------------------------------------------------------
// rcw_wall_generator_kernel<T>   An agent that began an episode gets the maze of one 64-bit key m, made by the whole wave in LDS:
//            words   [nwords]  the tile map's words: every tile WALL, then the cells' bits cleared (ds_and);
//            slot    [C]       per label the smallest order word of an edge leaving it this round (ds_min_u64), then its hook;
//            label   [C]       per cell the cell that names its component (label[root] == root);
//          C = ni * nj cells, cell c = ci * nj + cj on tile (2 ci + 1, 2 cj + 1) (0-based), lane takes cells lane + 64 i.
//          The tree is the minimum spanning tree under the order words w(id) = (draw(m, id) & ~0xFFFFF) | id — distinct, so the tree is
//          unique and Boruvka finds the one Kruskal finds.  A round:
//            offer   every cell offers the order words of its east (id 2c) and south (id 2c + 1) edge, where the edge joins two labels, to
//                    both labels' slots;
//            pick    every root with an offer opens the winning edge's passage tile and leaves in its slot the label across it;
//            hook    ... and hangs itself under that label — of two roots that picked each other (the same edge: the only cycle distinct
//                    words allow) the smaller stays a root;
//            jump    label[c] = label[label[c]] until nothing moves; one label left: done.  Every round at least halves the labels:
//                    at most ceil(log2 C) rounds.
//          Then one pass over the edges opens those whose loop draw (index 2C + id, high word) is below `loops` (tree edges are open
//          already: clearing a clear bit changes nothing).  Every barrier is the wave's own (a 64-thread workgroup), every condition around
//          one is uniform: the agent, the round's counts (__syncthreads_or / _count) and kernel arguments.
__device__ __forceinline__ void open_tile(uint32_t* words, int t) { atomicAnd(&words[t >> 4], ~(1u << ((t & 15) * 2))); }

// The maze of key m in LDS, by the whole wave: `words` (nwords) and, 8-byte aligned, `scratch` (12 bytes a cell: slots, then labels).  Ends
// on a barrier: the words are complete.  The generator's kernel and the caves' fallback call it.
__device__ __forceinline__ void maze_in_lds(uint32_t* const words, void* const scratch, const int H, const int HW, const int nwords, const int ni, const int nj,
                                            const uint64_t m, const uint32_t loops, const int lane)
{
    const int C = ni * nj;
    unsigned long long* const slot = reinterpret_cast<unsigned long long*>(scratch);
    uint32_t* const label = reinterpret_cast<uint32_t*>(slot + C);
    for (int w = lane; w < nwords; w += kBankBlock) words[w] = all_wall_word(HW, w);
    for (int c = lane; c < C; c += kBankBlock) label[c] = (uint32_t)c;
    __syncthreads();
    for (int c = lane; c < C; c += kBankBlock) {
        const int ci = c / nj, cj = c - ci * nj;
        open_tile(words, (2 * ci + 1) + H * (2 * cj + 1));
    }
    constexpr unsigned long long kNone = ~0ull;
    for (int round = 0; round < 13 && C > 1; ++round) {                    // (C <= 4096: 12 rounds at most; the count below ends it sooner)
        for (int c = lane; c < C; c += kBankBlock) slot[c] = kNone;
        __syncthreads();
        for (int c = lane; c < C; c += kBankBlock) {                       // offer
            const int ci = c / nj, cj = c - ci * nj;
            const uint32_t la = label[c];
            if (cj + 1 < nj) {
                const uint32_t lb = label[c + 1];
                if (la != lb) {
                    const unsigned long long id = 2ull * (unsigned)c;
                    const unsigned long long w = (rcw_draw(m, id) & 0xFFFFFFFFFFF00000ull) | id;
                    atomicMin(&slot[la], w); atomicMin(&slot[lb], w);
                }
            }
            if (ci + 1 < ni) {
                const uint32_t lb = label[c + nj];
                if (la != lb) {
                    const unsigned long long id = 2ull * (unsigned)c + 1ull;
                    const unsigned long long w = (rcw_draw(m, id) & 0xFFFFFFFFFFF00000ull) | id;
                    atomicMin(&slot[la], w); atomicMin(&slot[lb], w);
                }
            }
        }
        __syncthreads();
        for (int c = lane; c < C; c += kBankBlock) {                       // pick: the roots' winning edges are opened, the slot takes the label across
            if (label[c] != (uint32_t)c) continue;
            const unsigned long long w = slot[c];
            if (w == kNone) { slot[c] = (unsigned long long)c; continue; }
            const int id = (int)(w & 0xFFFFFull), ec = id >> 1, ed = ec + ((id & 1) ? nj : 1);
            const int ci = ec / nj, cj = ec - ci * nj;
            open_tile(words, (id & 1) ? (2 * ci + 2) + H * (2 * cj + 1) : (2 * ci + 1) + H * (2 * cj + 2));
            const uint32_t la = label[ec], lb = label[ed];
            slot[c] = (unsigned long long)(la == (uint32_t)c ? lb : la);
        }
        __syncthreads();
        for (int c = lane; c < C; c += kBankBlock) {                       // hook (only roots' labels are written, only slots are read)
            if (label[c] != (uint32_t)c) continue;
            const uint32_t o = (uint32_t)slot[c];
            if (o != (uint32_t)c && !((uint32_t)slot[o] == (uint32_t)c && (uint32_t)c < o)) label[c] = o;
        }
        __syncthreads();
        for (;;) {                                                         // jump: any value read is an ancestor, so the race within the wave is benign
            int moved = 0;
            for (int c = lane; c < C; c += kBankBlock) {
                const uint32_t q = label[c], qq = label[q];
                if (qq != q) { label[c] = qq; moved = 1; }
            }
            if (!__syncthreads_or(moved)) break;
        }
        int apart = 0;
        const uint32_t l0 = label[0];
        for (int c = lane; c < C; c += kBankBlock) apart |= (label[c] != l0) ? 1 : 0;
        if (!__syncthreads_or(apart)) break;
    }
    if (loops != 0u) {
        for (int c = lane; c < C; c += kBankBlock) {
            const int ci = c / nj, cj = c - ci * nj;
            const unsigned long long id = 2ull * (unsigned)c, base = 2ull * (unsigned)C;
            if (cj + 1 < nj && (uint32_t)(rcw_draw(m, base + id) >> 32) < loops) open_tile(words, (2 * ci + 1) + H * (2 * cj + 2));
            if (ci + 1 < ni && (uint32_t)(rcw_draw(m, base + id + 1ull) >> 32) < loops) open_tile(words, (2 * ci + 2) + H * (2 * cj + 1));
        }
    }
    __syncthreads();
}

// The key of the layout of the episode an agent began (counter ep): the episode's own draw 2^63 (the bank's index), or the key of the level it
// picks; *level: what wall_layout[a] says.
__device__ __forceinline__ uint64_t layout_key(const RcwDev& p, const RcwWallGen& g, int a, uint32_t ep, int* level)
{
    const uint64_t key = rcw_episode_key(p.seed, (uint64_t)(p.agent_id_offset + a), (uint64_t)(ep - 1u));
    const uint64_t u = rcw_draw(key, kLayoutDraw);
    *level = -1;
    if (g.levels <= 0) return u;
    *level = g.first_level + (int)rcw_below(u, (uint64_t)g.levels);
    return rcw_episode_key(g.level_seed, (uint64_t)*level, 0ull);
}

template <typename T>
__global__ __launch_bounds__(kBankBlock) void rcw_wall_generator_kernel(const RcwDev p, const RcwLimit lim, const RcwWallBank b, const RcwWallGen g, const int force)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_g[];
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= p.B) return;
    const uint32_t ep = p.episode[a];
    if (no_restart(b, force, a, lane, ep)) return;
    int level;
    const uint64_t m = layout_key(p, g, a, ep, &level);
    maze_in_lds(lds_g, lds_g + ((p.nwords + 1) & ~1), p.H, p.H * p.W, p.nwords, g.ni, g.nj, m, g.loops, lane);   // (the scratch: 8-byte aligned)
    restart_on_lds_words<T>(p, lim, b, a, lane, lds_g, ep, level);
}

// ---- caves (include/rcw.h, "the wall generator: caves") ------------------------------------------------------------------------------------
// rcw_wall_caves_kernel<T>   An agent that began an episode gets cave(m, H, W, fill, smooth), made by the whole wave in LDS over the n = (H - 2)(W - 2) INTERIOR tiles,
//          q = (i - 1) + (H - 2)(j - 1) — the tile map's own order, so the smallest q of a region is its smallest tile index:
//            words   [nwords]  the tile map's words, written last;
//            label   [n]       per free tile the tile that names its region (label[root] == root), kNoLabel on a wall;
//            count   [n]       per root its region's tiles (ds_add);
//            plane   [2][n]    generations g and g + 1, a byte a tile (1 = WALL); the ring is not stored: a neighbour outside the
//                              interior counts as WALL.
//          Lane takes tiles lane + 64 i.  Generation 0 is one draw a tile; a smoothing step reads one plane and writes the other.  Labels:
//            hook    every free tile takes the smallest label among itself and its free 4-neighbours, and hangs the tile its label named
//                    under that one too (ds_min): labels only fall, and a label always names a tile of the same region at or below its owner;
//            jump    label[q] = label[label[q]] until nothing moves;
//          until a hook moves nothing (__syncthreads_or): then neighbours agree, every label is a root, and the root of a region is its
//          smallest tile — no iteration cap.  One ds_max of (size << 16) | (0xFFFF - root) over the roots picks the largest region, of equals
//          the one with the smallest root (n <= 4096: the size fits 13 bits, the root 16).  Every lane reads that word back: a kept region of
//          `need` tiles opens its tiles in `words`; anything less is the fallback, maze(m, H, W, 0) by maze_in_lds, whose slots and labels
//          alias label / count / plane (12 bytes a cell, ni nj <= 4 n / 9).  Every barrier is the wave's own and under a uniform condition:
//          the agent, kernel arguments, __syncthreads_or's result, the word every lane read after a barrier.
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;
constexpr uint64_t kCaveDraw = 0x4000000000000000ull;

template <typename T>
__global__ __launch_bounds__(kBankBlock) void rcw_wall_caves_kernel(const RcwDev p, const RcwLimit lim, const RcwWallBank b, const RcwWallGen g, const RcwWallCaves cv,
                                                                    const int force)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_c[];
    __shared__ uint32_t best;
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= p.B) return;
    const uint32_t ep = p.episode[a];
    if (no_restart(b, force, a, lane, ep)) return;
    const int H = p.H, nwords = p.nwords, HW = p.H * p.W, h = p.H - 2, w = p.W - 2, n = h * w;
    uint32_t* const words = lds_c;
    uint32_t* const label = lds_c + ((nwords + 1) & ~1);                    // (8-byte aligned: the maze's slots alias it)
    uint32_t* const count = label + n;
    uint8_t* plane = reinterpret_cast<uint8_t*>(count + n);
    uint8_t* next = plane + n;
    int level;
    const uint64_t m = layout_key(p, g, a, ep, &level);
    // generation 0
    for (int q = lane; q < n; q += kBankBlock) {
        const int jj = q / h, ii = q - jj * h;
        const uint64_t t = (uint64_t)((ii + 1) + H * (jj + 1));
        plane[q] = (uint32_t)(rcw_draw(m, kCaveDraw + t) >> 32) < cv.fill ? 1 : 0;
    }
    if (lane == 0) best = 0u;
    __syncthreads();
    // smoothing: WALL in g + 1 where at least 5 of the 3 x 3 are WALL in g
    for (int s = 0; s < cv.smooth; ++s) {
        for (int q = lane; q < n; q += kBankBlock) {
            const int jj = q / h, ii = q - jj * h;
            int walls = 0;
            for (int dj = -1; dj <= 1; ++dj)
                for (int di = -1; di <= 1; ++di) {
                    const int i2 = ii + di, j2 = jj + dj;
                    walls += (i2 < 0 || i2 >= h || j2 < 0 || j2 >= w) ? 1 : (int)plane[i2 + h * j2];
                }
            next[q] = walls >= 5 ? 1 : 0;
        }
        __syncthreads();
        uint8_t* const swap = plane; plane = next; next = swap;
    }
    // regions
    for (int q = lane; q < n; q += kBankBlock) {
        label[q] = plane[q] ? kNoLabel : (uint32_t)q;
        count[q] = 0u;
    }
    __syncthreads();
    for (;;) {
        int hooked = 0;
        for (int q = lane; q < n; q += kBankBlock) {                       // hook
            const uint32_t mine = label[q];
            if (mine == kNoLabel) continue;
            const int jj = q / h, ii = q - jj * h;
            uint32_t least = mine;                                          // (a wall's kNoLabel never wins a min)
            if (ii > 0) least = min(least, label[q - 1]);
            if (ii + 1 < h) least = min(least, label[q + 1]);
            if (jj > 0) least = min(least, label[q - h]);
            if (jj + 1 < w) least = min(least, label[q + h]);
            if (least < mine) { atomicMin(&label[mine], least); atomicMin(&label[q], least); hooked = 1; }
        }
        if (!__syncthreads_or(hooked)) break;
        for (;;) {                                                         // jump: any value read names a tile of the region at or below: the race is benign
            int moved = 0;
            for (int q = lane; q < n; q += kBankBlock) {
                const uint32_t l = label[q];
                if (l == kNoLabel) continue;
                const uint32_t ll = label[l];
                if (ll != l) { label[q] = ll; moved = 1; }
            }
            if (!__syncthreads_or(moved)) break;
        }
    }
    for (int q = lane; q < n; q += kBankBlock) {
        const uint32_t l = label[q];
        if (l != kNoLabel) atomicAdd(&count[l], 1u);
    }
    __syncthreads();
    for (int q = lane; q < n; q += kBankBlock)
        if (label[q] == (uint32_t)q) atomicMax(&best, (count[q] << 16) | (0xFFFFu - (uint32_t)q));
    __syncthreads();
    const uint32_t kept = best;                                            // (the same word on every lane)
    const int size = (int)(kept >> 16), need = max(7, n / 4);
    if (size >= need) {
        const uint32_t root = 0xFFFFu - (kept & 0xFFFFu);
        for (int x = lane; x < nwords; x += kBankBlock) {                  // (all_wall_word's expression, written out: through the helper this kernel's code comes out different)
            const int left = HW - 16 * x;
            words[x] = left >= 16 ? 0x55555555u : left <= 0 ? 0u : (0x55555555u & ((1u << (2 * left)) - 1u));
        }
        __syncthreads();
        for (int q = lane; q < n; q += kBankBlock) {
            if (label[q] != root) continue;
            const int jj = q / h, ii = q - jj * h;
            open_tile(words, (ii + 1) + H * (jj + 1));
        }
        __syncthreads();
    } else {
        maze_in_lds(words, label, H, HW, nwords, g.ni, g.nj, m, 0u, lane);
    }
    restart_on_lds_words<T>(p, lim, b, a, lane, words, ep, level);
}

// ---- rooms (include/rcw.h, "the wall generator: rooms") ------------------------------------------------------------------------------------
// rcw_wall_rooms_kernel<T>   An agent that began an episode gets rooms(m, H, W, room, stop, doors), made by the whole wave in LDS:
//            words   [nwords]  the tile map's words: the ring WALL, the interior free, the padding clear; wall tiles are set with ds_or;
//            list    [Q]       the chambers, four uint16 each (i0, i1, j0, j1, inclusive); i0 == 0 flags a room (a live i0 is odd);
//            tail              the entries in use (static LDS, ds_add).
//          The root is entry 0.  A round: lane takes the entries lane + 64 i below the tail as the round found it.  A live chamber is
//          either left whole — flagged — or cut: its lane paints the wall on line s but for the doors, overwrites the entry with the
//          child in front of s and appends the child behind it at the old tail + 1 ...; appended entries wait for the next round, so
//          round r handles the chambers r cuts below the root.  Until a round cuts nothing (__syncthreads_or).  The chambers of the list
//          are disjoint and each holds an (odd, odd) tile: never more than Q entries.  The layout does not depend on the order the lanes
//          append in: a chamber's draws are indexed by its own corners.  A wall is as long as the side it runs along, the shorter one but
//          for chambers too narrow to cut the other way: its lane paints it alone (at 130 x 130 the root's 128 tiles are the longest).
//          Every barrier is the wave's own and under a uniform condition: the agent, __syncthreads_or's result.
constexpr uint64_t kRoomsDraw = 0x2000000000000000ull;

// The even numbers of lo .. hi: their count, the first in *first.
__device__ __forceinline__ int evens(int lo, int hi, int* first)
{
    *first = lo + (lo & 1);
    return *first > hi ? 0 : (hi - *first) / 2 + 1;
}

template <typename T>
__global__ __launch_bounds__(kBankBlock) void rcw_wall_rooms_kernel(const RcwDev p, const RcwLimit lim, const RcwWallBank b, const RcwWallGen g, const RcwWallRooms rm,
                                                                    const int force)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_r[];
    __shared__ int tail;
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= p.B) return;
    const uint32_t ep = p.episode[a];
    if (no_restart(b, force, a, lane, ep)) return;
    const int H = p.H, W = p.W, nwords = p.nwords, HW = p.H * p.W, room = min(rm.room, kWallRoomsMaxTiles);   // (no side reaches it: the sums below stay in range)
    uint32_t* const words = lds_r;
    ushort4* const list = reinterpret_cast<ushort4*>(lds_r + ((nwords + 1) & ~1));   // (8-byte aligned)
    int level;
    const uint64_t m = layout_key(p, g, a, ep, &level);
    for (int x = lane; x < nwords; x += kBankBlock) {
        int t = 16 * x, j = t / H, i = t - j * H;
        uint32_t word = 0u;
        for (int k = 0; k < 16 && t < HW; ++k, ++t) {                      // (the padding stays clear)
            if (i == 0 || i == H - 1 || j == 0 || j == W - 1) word |= 1u << (2 * k);
            if (++i == H) { i = 0; ++j; }
        }
        words[x] = word;
    }
    if (lane == 0) {
        list[0] = make_ushort4((unsigned short)1, (unsigned short)(H - 2), (unsigned short)1, (unsigned short)(W - 2));
        tail = 1;
    }
    __syncthreads();
    const uint32_t root0 = (uint32_t)(1 + H), root1 = (uint32_t)((H - 2) + H * (W - 2));
    for (;;) {
        const int n = tail;                                                // (the same on every lane: nobody appends before the barrier)
        __syncthreads();
        int cut = 0;
        for (int e = lane; e < n; e += kBankBlock) {
            const ushort4 c = list[e];
            if (c.x == 0) continue;                                        // a room
            const int i0 = c.x, i1 = c.y, j0 = c.z, j1 = c.w;
            int r0, c0;
            const int nr = j1 > j0 ? evens(i0 + room, i1 - room, &r0) : 0;
            const int nc = i1 > i0 ? evens(j0 + room, j1 - room, &c0) : 0;
            const uint32_t t0 = (uint32_t)(i0 + H * j0), t1 = (uint32_t)(i1 + H * j1);
            const uint64_t d = kRoomsDraw + 8ull * (uint64_t)((t0 << 16) | t1);
            const bool root = t0 == root0 && t1 == root1;
            if ((nr == 0 && nc == 0) || (!root && (uint32_t)(rcw_draw(m, d + 1ull) >> 32) < rm.stop)) {
                list[e].x = 0;
                continue;
            }
            bool row = nc == 0;
            if (nr != 0 && nc != 0) {
                const int di = i1 - i0, dj = j1 - j0;
                row = di > dj || (di == dj && (rcw_draw(m, d) >> 63) != 0ull);
            }
            const int s = (row ? r0 : c0) + 2 * (int)rcw_below(rcw_draw(m, d + 2ull), (uint64_t)(row ? nr : nc));
            const int lo = row ? j0 : i0, hi = row ? j1 : i1, cnt = (hi - lo) / 2 + 1;
            const int door1 = lo + 2 * (int)rcw_below(rcw_draw(m, d + 3ull), (uint64_t)cnt);
            int door2 = door1;
            if ((uint32_t)(rcw_draw(m, d + 4ull) >> 32) < rm.doors) door2 = lo + 2 * (int)rcw_below(rcw_draw(m, d + 5ull), (uint64_t)cnt);
            const int base = row ? s : H * s, stride = row ? H : 1;          // the span's tile at position x: base + stride x
            for (int x = lo; x <= hi; ++x) {
                if (x == door1 || x == door2) continue;
                const int t = base + stride * x;
                atomicOr(&words[t >> 4], 1u << ((t & 15) * 2));
            }
            const int fresh = atomicAdd(&tail, 1);
            if (row) {
                list[e] = make_ushort4((unsigned short)i0, (unsigned short)(s - 1), (unsigned short)j0, (unsigned short)j1);
                list[fresh] = make_ushort4((unsigned short)(s + 1), (unsigned short)i1, (unsigned short)j0, (unsigned short)j1);
            } else {
                list[e] = make_ushort4((unsigned short)i0, (unsigned short)i1, (unsigned short)j0, (unsigned short)(s - 1));
                list[fresh] = make_ushort4((unsigned short)i0, (unsigned short)i1, (unsigned short)(s + 1), (unsigned short)j1);
            }
            cut = 1;
        }
        if (!__syncthreads_or(cut)) break;
    }
    restart_on_lds_words<T>(p, lim, b, a, lane, words, ep, level);
}

// The camera view of the agents the bank restarted (mask[a] != 0), from their fresh column descriptors: update_camera_view!'s column fill
// (SR:431-440, rcw_fill.hip's pixel rule: column_padding, then ceiling | colour | floor by row) one workgroup per agent.  Restarts are sparse:
// nearly every workgroup reads its mask byte and leaves, where the camera fill's moving window would sweep every column of the batch to
// skip it (33-35 us at 4096 x 256 columns with nobody in the mask).  A wavefront takes every fourth column, its lanes the rows: the
// stores of a column (Hc contiguous words) coalesce.
constexpr int kPaintBlock = 256;
__global__ __launch_bounds__(kPaintBlock) void rcw_wall_bank_paint_kernel(const RcwDev p, const uint8_t* __restrict__ mask)
{
    const int a = blockIdx.x;
    if (a >= p.B || mask[a] == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = p.N, Hc = p.Hc;
    const int32_t* const col_h = p.col_h + (size_t)a * (size_t)N;
    const uint8_t* const col_c = p.col_c + (size_t)a * (size_t)N;
    uint32_t* const frame = p.obs + (size_t)a * (size_t)N * (size_t)Hc;
    const uint32_t ceil_c = p.ceiling_color, floor_c = p.floor_color;
    for (int c = wave; c < N; c += kPaintBlock / 64) {
        const int pad = column_padding(Hc, col_h[c]);
        const uint32_t colour = p.colour[col_c[c] & 3];
        uint32_t* const column = frame + (size_t)c * (size_t)Hc;
        for (int r = lane; r < Hc; r += 64) column[r] = pixel(r, pad, Hc, colour, ceil_c, floor_c);
    }
}

}  // namespace

hipError_t rcw_launch_wall_bank_paint(const RcwDev& p, const uint8_t* mask_dev, hipStream_t s)
{
    if (p.B < 1) return hipSuccess;
    hipLaunchKernelGGL(rcw_wall_bank_paint_kernel, dim3(p.B), dim3(kPaintBlock), 0, s, p, mask_dev);
    return hipGetLastError();
}

hipError_t rcw_launch_wall_bank_pack(const RcwDev& p, const uint8_t* walls_dev, uint32_t* words_dev, int32_t layouts, hipStream_t s)
{
    const long long total = (long long)layouts * p.nwords;
    if (total < 1) return hipSuccess;
    hipLaunchKernelGGL(rcw_wall_bank_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, walls_dev, words_dev, p.H * p.W, p.nwords, total);
    return hipGetLastError();
}

// THE launch point, and the only place that sizes the kernels' LDS.  Every request starts with the map's words, rounded to an even count
// where something 8-byte aligned follows, and stays under the 64 KiB default:
//   bank    the words alone: at most 16 KiB, the largest map rcw_create accepts has 4080 words.
//   mazes   8 bytes a slot and 4 a label: at the 4096-cell bound 48 KiB + the words.  A square map has the fewest (129 x 129: 1042, 4.1 KiB), a
//           thin one the most: 2 x 2048 cells lie on 5 x 4097 (1282 words) and, with the last interior row and column left wall, on
//           6 x 4098 — 1538 words, 6.0 KiB, the largest request: 55,304 bytes.
//   caves   per interior tile 4 bytes of label, 4 of counter and the two planes' bytes — or, where that is more, the fallback maze's 12 bytes
//           a cell (it never is: ni nj <= 4 n / 9).  At the 4096-tile bound: 66 x 66 has 274 words, 42,056 bytes; the largest request is
//           5 x 1367's (4095 tiles, 428 words): 42,664 bytes.
//   rooms   8 bytes a chamber for Q entries.  At the 4096-room bound the list is 32 KiB: 130 x 130 (1057 words) asks for 37,000 bytes,
//           5 x 4097 (1281 words) for 37,896, and the largest request is 6 x 4098's (1537 words): 38,920 bytes.
hipError_t rcw_launch_layout_source(const RcwPlan& p, const RcwLayoutSource& src, bool force, hipStream_t s)
{
    if (p.B < 1) return hipSuccess;
    const dim3 grid(p.B), block(kBankBlock);
    const int f = force ? 1 : 0;
    const size_t even_words = (size_t)((p.nwords + 1) & ~1) * sizeof(uint32_t);
    switch (src.kind) {
    case kLayoutNone:
        return hipSuccess;
    case kLayoutBank: {
        if (src.agents.layouts < 1) return hipSuccess;
        const size_t lds = (size_t)p.nwords * sizeof(uint32_t);
        if (p.real64) hipLaunchKernelGGL(rcw_wall_bank_kernel<double>, grid, block, lds, s, p, p.limit, src.agents, f);
        else          hipLaunchKernelGGL(rcw_wall_bank_kernel<float>, grid, block, lds, s, p, p.limit, src.agents, f);
        break;
    }
    case kLayoutMazes: {
        const int cells = src.gen.ni * src.gen.nj;
        if (cells < 1 || cells > kWallGenMaxCells) return cells > kWallGenMaxCells ? hipErrorInvalidValue : hipSuccess;
        const size_t lds = even_words + (size_t)cells * 12u;
        if (p.real64) hipLaunchKernelGGL(rcw_wall_generator_kernel<double>, grid, block, lds, s, p, p.limit, src.agents, src.gen, f);
        else          hipLaunchKernelGGL(rcw_wall_generator_kernel<float>, grid, block, lds, s, p, p.limit, src.agents, src.gen, f);
        break;
    }
    case kLayoutCaves: {
        const long long n = (long long)(p.H - 2) * (long long)(p.W - 2);
        if (p.H < 5 || p.W < 5 || n > kWallCavesMaxTiles) return hipErrorInvalidValue;
        const size_t cave = ((size_t)n * 10u + 3u) & ~(size_t)3u, maze = (size_t)((p.H - 1) / 2) * (size_t)((p.W - 1) / 2) * 12u;
        const size_t lds = even_words + (cave > maze ? cave : maze);
        if (p.real64) hipLaunchKernelGGL(rcw_wall_caves_kernel<double>, grid, block, lds, s, p, p.limit, src.agents, src.gen, src.caves, f);
        else          hipLaunchKernelGGL(rcw_wall_caves_kernel<float>, grid, block, lds, s, p, p.limit, src.agents, src.gen, src.caves, f);
        break;
    }
    case kLayoutRooms: {
        if (p.H < 5 || p.W < 5 || src.rooms.room < 1 || rcw_wall_rooms_bound(p.H, p.W) > kWallRoomsMaxRooms || (long long)p.H * (long long)p.W > kWallRoomsMaxTiles)
            return hipErrorInvalidValue;
        const size_t lds = even_words + (size_t)rcw_wall_rooms_bound(p.H, p.W) * sizeof(ushort4);
        if (p.real64) hipLaunchKernelGGL(rcw_wall_rooms_kernel<double>, grid, block, lds, s, p, p.limit, src.agents, src.gen, src.rooms, f);
        else          hipLaunchKernelGGL(rcw_wall_rooms_kernel<float>, grid, block, lds, s, p, p.limit, src.agents, src.gen, src.rooms, f);
        break;
    }
    }
    return hipGetLastError();
}
