// The visit map (include/rcw.h, rcw_set_visit_map): per agent a UInt16 count of the calls it has stood in each cell — tile x heading sector —
// this episode, four words (here, visited, first, level_here), and optionally a UInt32 table of the counts summed over the batch and per
// level.  Behind every step / reset / set_state / set_walls of a handle that enabled it; nothing else of the library knows about it.
//
// rcw_visit_map_kernel: ONE WAVEFRONT PER AGENT (a 64-thread workgroup), the decomposition of the goal distance and the frontier.
//   COUNT   an agent whose episode goes on: lane 0 alone reads its pose, does ONE read-modify-write of two bytes, and stores the words.
//   BEGIN   a stale agent — its episode counter moved (a step) or it is in the call's mask (a refill): the wavefront clears the 2 * cells
//           bytes of the agent's map with the widest stores its base allows: up to seven UInt16 entries a lane each in front of the first
//           multiple of 16 bytes, 16 bytes a lane from there (1 KiB a pass), UInt16 entries behind the last one.  An agent whose map begins
//           on a multiple of 16 bytes has no head; with an odd `cells` most agents have one.  The __syncthreads behind the clear orders
//           every lane's stores in front of lane 0's store of the one counted entry (workgroup scope is enough: one wavefront wrote both).
//   table   plain relaxed atomicAdd of 1 on UInt32 in global memory from lane 0: row 0, and the level row where the layout word is in
//           range.  Integer adds: the table does not depend on the order of the agents.
// rcw_visit_table_read_kernel: A LANE PER AGENT, launched behind it on handles with a table only.  It reads — the kernel boundary is what
// makes every agent's adds complete — and stores level_here.  No grid-wide wait anywhere.
#include "rcw_kernels.h"
#include "../../include/rcw.h"

namespace {

constexpr int kVisitBlock = 64;          // one wavefront
constexpr int kVisitReadBlock = 256;

struct VisitArgs {
    int32_t B, H, W, nd, real64, refill;
    const float2* pos;
    const double2* pos64;
    const int32_t* dir;
    const uint32_t* episode;
    const uint8_t* mask;         // refill only; NULL: every agent
    const int32_t* layout;       // NULL: no layout source
    RcwVisitMap v;
};

// The cell of agent a (include/rcw.h, "the visit map"): s * H*W + i + H*j, or -1: the position is not finite or off the map (the
// comparisons are false for a NaN and for either infinity).  The floor of a Float32 is the same number taken in Float64.
__device__ __forceinline__ int visit_cell(const VisitArgs& g, int a)
{
    double x, y;
    if (g.real64) { const double2 q = g.pos64[a]; x = q.x; y = q.y; }
    else          { const float2 q = g.pos[a]; x = (double)q.x; y = (double)q.y; }
    const double fx = floor(x), fy = floor(y);
    if (!(fx >= 0.0 && fx < (double)g.H && fy >= 0.0 && fy < (double)g.W)) return -1;
    const int d = g.dir[a];
    if (d < 0 || d >= g.nd) return -1;                                     // (no call leaves such a heading; never index with it)
    const int s = (int)(((long long)d * g.v.sectors) / g.nd);
    return s * g.H * g.W + (int)fx + g.H * (int)fy;
}

// The table's row of agent a: 1 + (layout - first_level) inside [1, rows], else 0.
__device__ __forceinline__ int visit_row(const VisitArgs& g, int a)
{
    if (!g.layout) return 0;
    const long long k = (long long)g.layout[a] - (long long)g.v.first_level;
    return k >= 0 && k < (long long)g.v.rows ? 1 + (int)k : 0;
}

__global__ __launch_bounds__(kVisitBlock) void rcw_visit_map_kernel(const VisitArgs g)
{
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= g.B) return;
    if (g.refill && g.mask != nullptr && g.mask[a] == 0) return;          // an agent outside the call's mask keeps every byte
    const uint32_t ep = g.episode[a];
    const bool stale = g.refill || g.v.last_episode[a] != ep;             // (the same in every lane)
    const int cells = g.v.cells;
    uint16_t* const map = g.v.map + (size_t)a * cells;

    if (stale) {
        // head: the entries in front of the first multiple of 16 bytes (the base is a multiple of 2), body: 16 bytes a lane, tail: the rest
        const int head = min(cells, (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(map) & 15u)) & 15u) >> 1));
        const int body = (cells - head) >> 3;
        const int tail = head + (body << 3);
        if (lane < head) map[lane] = 0;
        uint4* const wide = reinterpret_cast<uint4*>(map + head);
        for (int c = lane; c < body; c += kVisitBlock) wide[c] = make_uint4(0u, 0u, 0u, 0u);
        if (tail + lane < cells) map[tail + lane] = 0;                     // (fewer than 8 entries)
        __syncthreads();
    }
    if (lane != 0) return;

    const int c = visit_cell(g, a);
    int32_t here = 0, first = 0;
    if (stale) {
        if (c >= 0) { map[c] = 1; here = 1; }
        g.v.visited[a] = here;
        g.v.last_episode[a] = ep;
    } else if (c >= 0) {
        const uint32_t v = map[c];
        first = v == 0u ? 1 : 0;
        here = (int32_t)min(v + 1u, 65535u);
        map[c] = (uint16_t)here;
        if (first) g.v.visited[a] += 1;
    }
    g.v.here[a] = here;
    g.v.first[a] = first;
    if (g.v.table && c >= 0) {
        atomicAdd(g.v.table + c, 1u);
        const int row = visit_row(g, a);
        if (row) atomicAdd(g.v.table + (size_t)row * cells + c, 1u);
    }
}

__global__ __launch_bounds__(kVisitReadBlock) void rcw_visit_table_read_kernel(const VisitArgs g)
{
    const int a = blockIdx.x * kVisitReadBlock + threadIdx.x;
    if (a >= g.B) return;
    const int c = visit_cell(g, a);
    g.v.level_here[a] = c >= 0 ? g.v.table[(size_t)visit_row(g, a) * g.v.cells + c] : 0u;
}

}  // namespace

hipError_t rcw_launch_visit_map(const RcwDev& p, int32_t B, const RcwVisitMap& vm, const int32_t* layout, const uint8_t* mask_dev, bool refill, hipStream_t s)
{
    if (B < 1) return hipSuccess;
    if (vm.sectors < 1 || vm.sectors > p.nd || (int64_t)vm.sectors * p.H * p.W != (int64_t)vm.cells) return hipErrorInvalidValue;
    const VisitArgs g{B, p.H, p.W, p.nd, p.real64, refill ? 1 : 0, p.pos, p.pos64, p.dir, p.episode, refill ? mask_dev : nullptr, layout, vm};
    hipLaunchKernelGGL(rcw_visit_map_kernel, dim3(B), dim3(kVisitBlock), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !vm.table) return e;
    hipLaunchKernelGGL(rcw_visit_table_read_kernel, dim3((unsigned)((B + kVisitReadBlock - 1) / kVisitReadBlock)), dim3(kVisitReadBlock), 0, s, g);
    return hipGetLastError();
}
