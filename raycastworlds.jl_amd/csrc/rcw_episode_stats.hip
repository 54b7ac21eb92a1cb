// Episode statistics (include/rcw.h, rcw_set_episode_stats): per agent the record of its episode — length, moves, outcome, level, SPL — and a
// table of UInt64 sums over the records that closed, row 0 for the batch and a row per level.  One kernel behind every step / reset /
// set_state / set_walls of a handle that enabled it; nothing else of the library knows about it.
//
// rcw_episode_stats_kernel<T>: ONE LANE PER AGENT, workgroups of 256, every array structure-of-arrays: a wavefront's loads and stores are
// coalesced.  No lane leaves early — the tail of the last wavefront takes part in the ballots and the reductions with nothing to add.
//   refill  (reset / set_state / set_walls / enabling) the agents of the mask begin a record, every other agent's `finished` is cleared.
//   step    the first that applies: the episode counter moved -> begin; a closed record -> frozen; else the record lives through the call
//           and closes where done | truncated.
//   table   all integers, so the sums do not depend on the order of the adds.  A wavefront that closed nothing issues no atomic.  One that
//           did goes in ROUNDS, each a ballot of the lanes the round takes and the six sums reduced over them (popcounts of ballots; the
//           lengths, moves and SPL words in the vector unit's data-parallel primitives, no LDS round trip), then one relaxed agent-scope
//           64-bit add per non-zero column from one lane: round 0 is row 0 and takes every closing lane; each later round takes the level
//           row of the first lane still waiting and every lane that shares it — so a step that closes a whole batch into a few levels (a
//           bank of two under a time limit: every agent truncates on the same call) adds 7 words a level a wavefront, not 6 a lane onto the
//           same two cache lines (measured: profiles/episode_stats_bench.txt).  After kRowRounds level rows the lanes left add their own
//           record to their own row: many levels, little contention.
//   SPL     Float64, one rounding per operation (-ffp-contract=off): p = moves * inc; q = floor((65536 * l) / fmax(p, l)).
#include "rcw_kernels.h"
#include "../../include/rcw.h"

namespace {

constexpr int kStatsBlock = 256;

struct EpisodeStatsArgs {
    int32_t B, rows, first;
    int32_t refill;                  // 1: the mask rule, 0: the step rule
    double inc;                      // position_increment_wu, widened
    const void* pos;                 // float2 / double2 [B]
    const uint8_t* done;
    const uint8_t* truncated;        // zero on a limit-less handle
    const uint32_t* episode;
    const int32_t* layout;           // NULL: no layout source
    const int32_t* start_distance;   // NULL: no goal distance
    const uint8_t* mask;             // refill only; NULL: every agent
    RcwEpisodeWords w;
    uint32_t* last_episode;
    void* prev_x;                    // T [B]
    void* prev_y;
    unsigned long long* table;       // [1 + rows][RCW_EPISODE_STATS_ROW_WORDS]
};

constexpr int kRowRounds = 4;

// The sum of x >= 0 over the wavefront, below 2^31, as a wave-uniform value (DPP, the sequence of AMD's cross-lane guide: quad_perm
// [1,0,3,2], [2,3,0,1], row_ror:4, :8, row_bcast:15, :31 leave the total in lane 63).  Every lane of the wavefront must be active.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp0(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xF, true); }
__device__ __forceinline__ int wave_sum(int x)
{
    x += dpp0<0xB1>(x); x += dpp0<0x4E>(x); x += dpp0<0x124>(x); x += dpp0<0x128>(x);
    x += dpp0<0x142, 0xA>(x); x += dpp0<0x143, 0xC>(x);
    return __builtin_amdgcn_readlane(x, 63);
}
// ... of UInt32 values, in 64 bits: the two 16-bit halves apart (64 * 65535 < 2^31)
__device__ __forceinline__ unsigned long long wave_sum64(uint32_t v)
{
    const unsigned long long lo = (uint32_t)wave_sum((int)(v & 0xFFFFu)), hi = (uint32_t)wave_sum((int)(v >> 16));
    return lo + (hi << 16);
}

__device__ __forceinline__ void table_add(unsigned long long* row, int col, unsigned long long v)
{
    if (v) __hip_atomic_fetch_add(row + col, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T> struct Bits;
template <> struct Bits<float> { typedef uint32_t type; };
template <> struct Bits<double> { typedef unsigned long long type; };

template <typename T>
__global__ __launch_bounds__(kStatsBlock) void rcw_episode_stats_kernel(const EpisodeStatsArgs g)
{
    typedef typename Bits<T>::type U;                                        // positions are compared and kept as bit patterns
    const int a = blockIdx.x * kStatsBlock + threadIdx.x;
    const bool live = a < g.B;
    U* const prev_x = static_cast<U*>(g.prev_x);
    U* const prev_y = static_cast<U*>(g.prev_y);
    U px = 0, py = 0;
    uint32_t ep = 0;
    if (live) {
        const U* const q = static_cast<const U*>(g.pos) + 2 * (size_t)a;
        px = q[0]; py = q[1];
        ep = g.episode[a];
    }
    bool begin = false, closing = false;
    if (g.refill) {
        begin = live && (!g.mask || g.mask[a]);
        if (live && !begin) g.w.finished[a] = 0;
    } else if (live) {
        begin = ep != g.last_episode[a];
    }
    if (begin) {
        g.w.length[a] = 0; g.w.moves[a] = 0; g.w.outcome[a] = RCW_EPISODE_OPEN; g.w.finished[a] = 0;
        g.w.level[a] = -1; g.w.spl_q16[a] = -1;
        prev_x[a] = px; prev_y[a] = py;
        g.last_episode[a] = ep;
    }
    if (g.refill) return;                                                    // (wave-uniform: no lane of a refill goes on)

    uint32_t length = 0, moves = 0;
    int32_t level = -1, spl = -1;
    bool success = false;
    if (live && !begin) {
        if (g.w.outcome[a] != RCW_EPISODE_OPEN) {                            // frozen: the words keep the finished episode
            g.w.finished[a] = 0;
            prev_x[a] = px; prev_y[a] = py;
        } else {
            length = g.w.length[a] + 1u;
            moves = g.w.moves[a] + ((px != prev_x[a] || py != prev_y[a]) ? 1u : 0u);
            g.w.length[a] = length; g.w.moves[a] = moves;
            prev_x[a] = px; prev_y[a] = py;
            success = g.done[a] != 0;
            closing = success || g.truncated[a] != 0;
            if (!closing) g.w.finished[a] = 0;
        }
    }
    const unsigned long long closed = __ballot(closing);
    if (!closed) return;                                                     // (wave-uniform)

    if (closing) {
        level = g.layout ? g.layout[a] : -1;
        const int32_t l = g.start_distance ? g.start_distance[a] : -1;
        if (l >= 1) {
            spl = 0;
            if (success) {
                const double p = (double)moves * g.inc;
                const double num = 65536.0 * (double)l;
                spl = (int32_t)floor(num / fmax(p, (double)l));
            }
        }
        g.w.outcome[a] = success ? RCW_EPISODE_SUCCESS : RCW_EPISODE_TRUNCATED;
        g.w.level[a] = level;
        g.w.spl_q16[a] = spl;
        g.w.episodes[a] += 1u;
        g.w.finished[a] = 1;
    }
    // the level row of a close: 1 + (level - first) inside [1, rows], or 0: none
    const long long k = (long long)level - (long long)g.first;
    const int row = closing && k >= 0 && k < (long long)g.rows ? 1 + (int)k : 0;
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long todo = 0;                                             // lanes whose level row is still to be added
    int target = 0;                                                          // the round's row
    bool mine = closing;                                                     // ... and whether it takes this lane
    for (int round = 0;; ++round) {                                          // (every condition wave-uniform)
        const unsigned long long m = __ballot(mine);
        const unsigned long long n = (unsigned long long)__popcll(m);
        const unsigned long long n_success = (unsigned long long)__popcll(__ballot(mine && success));
        const unsigned long long n_spl = (unsigned long long)__popcll(__ballot(mine && spl >= 0));
        const unsigned long long s_length = wave_sum64(mine ? length : 0u);
        const unsigned long long s_moves = wave_sum64(mine ? moves : 0u);
        const unsigned long long s_spl = (uint32_t)wave_sum(mine && spl >= 0 ? spl : 0);      // (64 * 65536 < 2^31)
        if (lane == 0) {
            unsigned long long* const t = g.table + (size_t)target * RCW_EPISODE_STATS_ROW_WORDS;
            table_add(t, 0, n); table_add(t, 1, n_success); table_add(t, 2, n - n_success);
            table_add(t, 3, s_length); table_add(t, 4, s_moves); table_add(t, 5, n_spl); table_add(t, 6, s_spl);
        }
        todo = round == 0 ? __ballot(row != 0) : todo & ~m;
        if (!todo || round == kRowRounds) break;
        target = __shfl(row, __ffsll((long long)todo) - 1, 64);              // the first waiting lane's row: never 0
        mine = row == target;
    }
    if ((todo >> lane) & 1ull) {
        unsigned long long* const t = g.table + (size_t)row * RCW_EPISODE_STATS_ROW_WORDS;
        table_add(t, 0, 1ull); table_add(t, success ? 1 : 2, 1ull);
        table_add(t, 3, length); table_add(t, 4, moves);
        if (spl >= 0) { table_add(t, 5, 1ull); table_add(t, 6, (unsigned long long)spl); }
    }
}

}  // namespace

hipError_t rcw_launch_episode_stats(const RcwDev& p, const RcwLimit& limit, const RcwEpisodeStats& st, const int32_t* layout,
                                    const int32_t* start_distance, const uint8_t* mask_dev, bool refill, hipStream_t s)
{
    if (p.B < 1) return hipSuccess;
    const EpisodeStatsArgs g{p.B, st.rows, st.first, refill ? 1 : 0, p.real64 ? p.inc64 : (double)p.inc,
                             p.real64 ? (const void*)p.pos64 : (const void*)p.pos, p.done, limit.truncated, p.episode, layout,
                             start_distance, refill ? mask_dev : nullptr, st.words, st.last_episode, st.prev_x, st.prev_y,
                             reinterpret_cast<unsigned long long*>(st.table)};
    const dim3 grid((unsigned)((p.B + kStatsBlock - 1) / kStatsBlock)), block(kStatsBlock);
    if (p.real64) hipLaunchKernelGGL(rcw_episode_stats_kernel<double>, grid, block, 0, s, g);
    else hipLaunchKernelGGL(rcw_episode_stats_kernel<float>, grid, block, 0, s, g);
    return hipGetLastError();
}
