// The guide (include/rcw.h, rcw_set_guide): per agent the action that follows its shortest path to the goal — UInt8 `action`, always a
// valid one, and Int32 `heading`, the direction index the guide wants the agent to face (-1: no advice).  A pure function of the goal
// distance's field, the pose and the direction table as they are when the kernel runs: one launch behind the goal distance's wherever
// that runs, and behind a new direction table and a restore, of a handle that enabled it; nothing else of the library knows about it.
//
// rcw_guide_kernel<T>: ONE WAVEFRONT PER AGENT (a 64-thread workgroup, the goal distance's decomposition).
//   scalars  the pose, the agent's own field entry and its four neighbours' are the same in every lane; every lane takes the same branch up
//            to the target, so nothing is broadcast.  The loads go out in two batches: pose, heading and the lane's first table entry at
//            once, the five field entries together behind the pose (a neighbour's does not wait for the own entry's value).  No index
//            leaves the field: the own entry is read behind the bounds check, a neighbour only where it lies on the map.
//   table    the 64 lanes stride the direction table, lane l entries l, l + 64, ...: a wavefront load is 512 contiguous bytes (Float32)
//            or 1 KiB (Float64).  s[k] = fl(fl(D1[k] vx) + fl(D2[k] vy)), a rounding per operation (-ffp-contract=off).  A lane keeps the
//            first of its greatest s: k rises within a lane, so `>` keeps the smaller index; a NaN compares false and never enters.
//   argmax   over the wavefront on the pair (s, -k), six xor-shuffle rounds in registers, no LDS: the greater s wins, of equal s the
//            smaller k, and a lane that holds nothing (k = -1: nd < 64, or every entry it saw was NaN) loses to one that holds something.
//            Every lane ends with the same pair; nothing at all (an all-NaN table) is heading 0.
//   stores   lane 0, two plain vector stores.
#include "rcw_kernels.h"
#include "../../include/rcw.h"

namespace {

constexpr int kGuideBlock = 64;            // one wavefront
constexpr uint32_t kGuideUnreached = 0xFFFFu;

struct GuideArgs {
    int32_t B, H, W, nd;
    const void* pos;             // float2 / double2 [B]
    const int32_t* dir;          // [B] 0-based heading
    const void* table;           // float2 / double2 [nd]: (D1, D2)
    const uint16_t* field;       // [B][H*W] the goal distance's
    double inc;                  // position_increment_wu in T (exact as a double)
    uint8_t* action;             // [B]
    int32_t* heading;            // [B]
};

__device__ __forceinline__ float floor_t(float v) { return __builtin_floorf(v); }
__device__ __forceinline__ double floor_t(double v) { return __builtin_floor(v); }
__device__ __forceinline__ float abs_t(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double abs_t(double v) { return __builtin_fabs(v); }

template <typename T> struct Pair;
template <> struct Pair<float> { typedef float2 type; };
template <> struct Pair<double> { typedef double2 type; };

template <typename T>
__global__ __launch_bounds__(kGuideBlock) void rcw_guide_kernel(const GuideArgs g)
{
    typedef typename Pair<T>::type T2;
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= g.B) return;
    const int H = g.H, W = g.W;
    // what depends on nothing but the agent and the lane goes out first — the pose, the heading, the lane's first table entry —, then the
    // five field entries together behind the pose
    const T2* const table = static_cast<const T2*>(g.table);
    const T2 q = static_cast<const T2*>(g.pos)[a];
    const int32_t d0 = g.dir[a];
    T2 entry = table[lane < g.nd ? lane : 0];                                   // (nd >= 1: entry 0 is there; a lane past the table never uses it)
    const T x = q.x, y = q.y;
    // 1  the tile, and where there is no advice: the agent turns on the spot
    const T fx = floor_t(x), fy = floor_t(y);
    const bool on_map = fx >= (T)0 && fx < (T)H && fy >= (T)0 && fy < (T)W;     // (false for a NaN or an infinity)
    int i = 0, j = 0;
    uint32_t f = kGuideUnreached, up = kGuideUnreached, down = kGuideUnreached, left = kGuideUnreached, right = kGuideUnreached;
    const uint16_t* const field = g.field + (size_t)a * ((size_t)H * (size_t)W);
    if (on_map) {                                                               // (0 <= i < H, 0 <= j < W: every index below is inside the agent's field)
        i = (int)fx; j = (int)fy;
        const size_t t = (size_t)i + (size_t)H * (size_t)j;
        f = field[t];
        if (i > 0) up = field[t - 1];
        if (i < H - 1) down = field[t + 1];
        if (j > 0) left = field[t - (size_t)H];
        if (j < W - 1) right = field[t + (size_t)H];
    }
    // 2  the next tile: the first of (i-1, j), (i+1, j), (i, j-1), (i, j+1) on the map one step nearer
    int ni = -1, nj = -1;
    if (f != kGuideUnreached && f != 0u) {
        const uint32_t want = f - 1u;
        if (up == want) { ni = i - 1; nj = j; }
        else if (down == want) { ni = i + 1; nj = j; }
        else if (left == want) { ni = i; nj = j - 1; }
        else if (right == want) { ni = i; nj = j + 1; }
    }
    if (ni < 0) {                                                               // (also a field no flood wrote: no neighbour is nearer)
        if (lane == 0) { g.heading[a] = -1; g.action[a] = 3; }
        return;
    }
    // 3  the target: the next tile's centre once the agent is within inc of the corridor's axis, its own tile's centre before
    const T ctx = (T)i + (T)0.5, cty = (T)j + (T)0.5;
    const T e = ni != i ? y - cty : x - ctx;
    const bool go = abs_t(e) <= (T)g.inc;
    const T px = go ? (T)ni + (T)0.5 : ctx, py = go ? (T)nj + (T)0.5 : cty;
    const T vx = px - x, vy = py - y;
    // 4  the heading: the smallest k of the greatest s[k]
    T best = (T)0;
    int bk = -1;
    for (int k = lane; k < g.nd; k += kGuideBlock) {
        const T s = entry.x * vx + entry.y * vy;
        if (bk < 0 ? s == s : s > best) { best = s; bk = k; }
        if (k + kGuideBlock < g.nd) entry = table[k + kGuideBlock];
    }
#pragma unroll
    for (int m = 1; m < kGuideBlock; m <<= 1) {
        const T os = __shfl_xor(best, m, kGuideBlock);
        const int ok = __shfl_xor(bk, m, kGuideBlock);
        if (ok >= 0 && (bk < 0 || os > best || (os == best && ok < bk))) { best = os; bk = ok; }
    }
    if (lane != 0) return;
    const int heading = bk < 0 ? 0 : bk;
    // 5  the action: forward, or the shorter turn (left on a tie)
    const int64_t nd = g.nd;
    const int64_t delta = ((((int64_t)heading - (int64_t)d0) % nd) + nd) % nd;
    g.heading[a] = heading;
    g.action[a] = delta == 0 ? 1 : (delta <= nd / 2 ? 3 : 4);
}

}  // namespace

hipError_t rcw_launch_guide(const RcwDev& p, int32_t B, const uint16_t* field, const RcwGuideWords& words, hipStream_t s)
{
    if (B < 1) return hipSuccess;
    const GuideArgs g{B, p.H, p.W, p.nd, p.real64 ? (const void*)p.pos64 : (const void*)p.pos, p.dir,
                      p.real64 ? (const void*)p.dir_table64 : (const void*)p.dir_table, field, p.real64 ? p.inc64 : (double)p.inc,
                      words.action, words.heading};
    if (p.real64) hipLaunchKernelGGL(rcw_guide_kernel<double>, dim3(B), dim3(kGuideBlock), 0, s, g);
    else          hipLaunchKernelGGL(rcw_guide_kernel<float>, dim3(B), dim3(kGuideBlock), 0, s, g);
    return hipGetLastError();
}
