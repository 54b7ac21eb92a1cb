// The state archive (include/rcw.h, "the state archive"): `rows` agent records kept on the device.  A record is a list of SEGMENTS — one per
// per-agent array of the handle, every one stored [B][bytes] live and [rows][bytes] in the archive —, so save and restore are the same copy
// with the two sides exchanged.  Two launches a call, both on the handle's stream, neither touches anything a step's kernels run:
//
// rcw_snapshot_resolve_kernel, A LANE PER AGENT: which row the agent takes (rows[a], or a), or -1 — outside the mask, or an index outside
//   [0, nrows), or (restore) a row nobody has filled: those two leave the agent as it is and set its status word and the handle's error word
//   to RCW_ERR_INVALID_ARGUMENT, as an invalid action does.  A save also marks the row filled and enters owner[row] = max(agents that save
//   into it) with atomicMax (owner: -1 everywhere in front of the launch): the copy below writes a row for its owner alone, so a row two
//   agents save into holds the whole record of the higher one, never a mixture.
//
// rcw_snapshot_copy_kernel, ONE KERNEL FOR BOTH DIRECTIONS, memory-bound, driven by the segment table in its arguments (at most
//   kSnapshotKernelSegments a launch; the host launches again for the rest).  The work is cut into wavefront TASKS, numbered through the
//   table: a segment of more than kSmallBytes has a task an agent — the wavefront copies the record, 16 bytes a lane an access where the
//   record's bytes and both bases are 16-byte multiples (every record then begins on one), else a 4-byte body, unaligned where the
//   record begins on an odd address (189-byte stacks, 25-byte maps), and a byte tail —; a smaller segment has a task per
//   64 agents, a lane an agent (the 4-byte words: one coalesced load, one scattered store).  The grid is capped and the wavefronts stride
//   over the tasks.  Plain C++: no inline assembly, vector stores only.
#include "rcw_kernels.h"
#include "../../include/rcw.h"

namespace {

constexpr int kSnapBlock = 256;          // four wavefronts
constexpr uint32_t kSmallBytes = 16;     // up to here a lane copies an agent's whole record of the segment

struct ResolveArgs {
    int32_t B, nrows, restore;
    const int32_t* rows;         // [B] or NULL: agent a takes row a
    const uint8_t* mask;         // [B] or NULL: every agent
    uint8_t* filled;             // [nrows]
    int32_t* owner;              // [nrows], save only
    int32_t* sel;                // [B] out
    int32_t* status;             // [B] the agents' sticky status words
    int32_t* err;                // the handle's error word
};

__global__ __launch_bounds__(kSnapBlock) void rcw_snapshot_resolve_kernel(const ResolveArgs g)
{
    const int a = blockIdx.x * kSnapBlock + threadIdx.x;
    if (a >= g.B) return;
    int32_t r = -1;
    if (!g.mask || g.mask[a]) {
        r = g.rows ? g.rows[a] : a;
        bool ok = r >= 0 && r < g.nrows;
        if (ok && g.restore) ok = g.filled[r] != 0;
        if (!ok) {
            g.err[0] = RCW_ERR_INVALID_ARGUMENT;
            g.status[a] = RCW_ERR_INVALID_ARGUMENT;
            r = -1;
        } else if (!g.restore) {
            atomicMax(&g.owner[r], a);
            g.filled[r] = 1;
        }
    }
    g.sel[a] = r;
}

template <typename V>
__device__ __forceinline__ void copy_units(uint8_t* dst, const uint8_t* src, uint32_t n, int lane)
{
    for (uint32_t i = (uint32_t)lane; i < n; i += 64u) reinterpret_cast<V*>(dst)[i] = reinterpret_cast<const V*>(src)[i];
}

// A record whose bytes or bases are no 16-byte multiples: a 4-byte body — the record may begin on any address, and the two sides on different
// ones; global accesses of gfx950 need no alignment, and the compiler is told so (memcpy of 4 bytes: align 1) — and a byte tail of up to 3.
__device__ __forceinline__ void copy_dwords_and_tail(uint8_t* dst, const uint8_t* src, uint32_t bytes, int lane)
{
    const uint32_t n4 = bytes >> 2, tail = bytes & 3u;
    for (uint32_t i = (uint32_t)lane; i < n4; i += 64u) {
        uint32_t v;
        __builtin_memcpy(&v, src + 4u * i, 4);
        __builtin_memcpy(dst + 4u * i, &v, 4);
    }
    if ((uint32_t)lane < tail) dst[4u * n4 + lane] = src[4u * n4 + lane];
}

__global__ __launch_bounds__(kSnapBlock) void rcw_snapshot_copy_kernel(const RcwSnapshotTable t, const int32_t B, const int32_t* __restrict__ sel,
                                                                      const int32_t* __restrict__ owner, const int32_t restore)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kSnapBlock + threadIdx.x) >> 6));
    const uint32_t nwaves = gridDim.x * (kSnapBlock / 64);
    for (uint32_t task = wave0; task < t.tasks; task += nwaves) {
        int s = 0;                                                           // the task's segment: wave-uniform, at most 31 steps
        while (s + 1 < t.n && task >= t.seg[s + 1].first_task) ++s;
        const RcwSnapshotSeg sg = t.seg[s];
        const uint32_t k = task - sg.first_task;
        if (sg.bytes > kSmallBytes) {                                        // a wavefront an agent
            const int a = (int)k;                                            // < B: the host's task count
            const int r = sel[a];
            if (r < 0 || (owner && owner[r] != a)) continue;
            uint8_t* const live = sg.live + (size_t)a * sg.bytes;
            uint8_t* const row = sg.rows + (size_t)r * sg.bytes;
            uint8_t* const dst = restore ? live : row;
            const uint8_t* const src = restore ? row : live;
            const uint32_t align = (uint32_t)(((uintptr_t)sg.live | (uintptr_t)sg.rows | sg.bytes) & 15u);
            if (align == 0u) copy_units<uint4>(dst, src, sg.bytes >> 4, lane);
            else copy_dwords_and_tail(dst, src, sg.bytes, lane);
        } else {                                                             // a lane an agent
            const int a = (int)(k * 64u) + lane;
            if (a >= B) continue;
            const int r = sel[a];
            if (r < 0 || (owner && owner[r] != a)) continue;
            uint8_t* const live = sg.live + (size_t)a * sg.bytes;
            uint8_t* const row = sg.rows + (size_t)r * sg.bytes;
            uint8_t* const dst = restore ? live : row;
            const uint8_t* const src = restore ? row : live;
            const uint32_t align = (uint32_t)(((uintptr_t)sg.live | (uintptr_t)sg.rows | sg.bytes) & 3u);
            if (align == 0u) {
                for (uint32_t i = 0; i < sg.bytes >> 2; ++i) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
            } else {
                for (uint32_t i = 0; i < sg.bytes; ++i) dst[i] = src[i];
            }
        }
    }
}

}  // namespace

uint32_t rcw_snapshot_tasks(uint32_t bytes, int32_t B)
{
    return bytes > kSmallBytes ? (uint32_t)B : ((uint32_t)B + 63u) / 64u;
}

hipError_t rcw_launch_snapshot_resolve(const RcwDev& p, int32_t B, const int32_t* rows_dev, const uint8_t* mask_dev, int32_t nrows, bool restore,
                                       uint8_t* filled, int32_t* owner, int32_t* sel, hipStream_t s)
{
    if (B < 1) return hipSuccess;
    const ResolveArgs g{B, nrows, restore ? 1 : 0, rows_dev, mask_dev, filled, owner, sel, p.status, p.err};
    hipLaunchKernelGGL(rcw_snapshot_resolve_kernel, dim3((B + kSnapBlock - 1) / kSnapBlock), dim3(kSnapBlock), 0, s, g);
    return hipGetLastError();
}

hipError_t rcw_launch_snapshot_copy(const RcwSnapshotTable& t, int32_t B, const int32_t* sel, const int32_t* owner, bool restore, int grid_cap, hipStream_t s)
{
    if (B < 1 || t.n < 1 || t.tasks < 1) return hipSuccess;
    if (t.n > kSnapshotKernelSegments) return hipErrorInvalidValue;
    const uint32_t want = (t.tasks + kSnapBlock / 64 - 1) / (kSnapBlock / 64);
    const uint32_t cap = grid_cap > 0 ? (uint32_t)grid_cap : 2048u;
    hipLaunchKernelGGL(rcw_snapshot_copy_kernel, dim3(want < cap ? want : cap), dim3(kSnapBlock), 0, s, t, B, sel, owner, restore ? 1 : 0);
    return hipGetLastError();
}
