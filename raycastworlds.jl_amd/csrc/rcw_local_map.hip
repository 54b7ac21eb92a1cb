// The local map (include/rcw.h, rcw_set_local_map): per agent an UInt8 (S, S) crop of its tile map (RCW_LOCAL_WORLD) or of its seen map
// (RCW_LOCAL_SEEN), centred on the agent and turned so that its heading points up, r cells a tile.  A pure function of the state behind the
// call: one kernel behind every step / reset / set_state / set_walls / new direction table of a handle that enabled it; nothing else of
// the library knows about it.
//
// rcw_local_map_kernel<T, SEEN>: ONE WORKGROUP PER AGENT, in whole wavefronts.
//   LDS    the offset table off[S] in T (built on the host: rcw_rules.hip), and for WORLD the agent's packed tile words, (H*W + 15) / 16 of
//          them — at most 1 KiB + 16.1 KiB, inside the default dynamic-LDS limit.  SEEN gathers the map bytes through the cache.
//   lanes  the batch is one byte array, agent a at a*S*S: a lane owns one ALIGNED 32-bit word of that array — four consecutive cells of the
//          row-major image — and stores it as one uint32.  S*S need not be a multiple of four, so an agent's image may begin and end inside a
//          word: the (at most two) words it shares with its neighbours are stored byte by byte, only the agent's own bytes.  The stride is
//          S*S, unpadded.
//   cell   (row q, column c): ahead = off[S-1-q], lateral = off[S-1-c]; wx = (px + ahead*d1) + lateral*d2, wy = (py + ahead*d2) - lateral*d1,
//          each operation rounded once in T (-ffp-contract=off); floor, compared in T against the map (a NaN fails every comparison), and
//          only then converted: the tile index is inside [0, H*W) or nothing is read.
#include "rcw_device.h"

namespace {

constexpr int kLocalBlock = 256;

struct LocalMapArgs {
    int32_t B, H, W, S;
    int32_t nwords;              // 32-bit words of one agent's tile_map
    const void* pos;             // float2 / double2 [B]
    const int32_t* dir;
    const void* dir_table;       // float2 / double2 [nd]
    const uint32_t* tile_map;
    const uint8_t* seen;         // [B][H*W], SEEN only
    const void* off;             // T [S]
    uint8_t* out;                // [B][S*S], 4-byte aligned
};

template <typename T, bool SEEN>
__global__ __launch_bounds__(kLocalBlock) void rcw_local_map_kernel(const LocalMapArgs g)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_l[];
    const int a = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    if (a >= g.B) return;
    const int H = g.H, W = g.W, S = g.S, SS = S * S, HW = H * W;
    T* const off = reinterpret_cast<T*>(lds_l);                              // [S]
    uint32_t* const words = lds_l + ((S * (int)sizeof(T) + 15) >> 4) * 4;         // [(HW + 15) / 16], WORLD only
    for (int k = tid; k < S; k += nthreads) off[k] = static_cast<const T*>(g.off)[k];
    if (!SEEN) {
        const uint32_t* const tm = g.tile_map + (size_t)a * g.nwords;
        for (int k = tid; k < (HW + 15) >> 4; k += nthreads) words[k] = tm[k];
    }
    __syncthreads();

    const typename Real<T>::vec2 pos = static_cast<const typename Real<T>::vec2*>(g.pos)[a];
    const typename Real<T>::vec2 d = static_cast<const typename Real<T>::vec2*>(g.dir_table)[g.dir[a]];
    const uint8_t* const seen = SEEN ? g.seen + (size_t)a * HW : nullptr;
    const T fH = (T)H, fW = (T)W;

    const size_t base = (size_t)a * (size_t)SS;                              // the agent's first byte
    const int lead = (int)(base & 3u);                                       // bytes of its first word that are the previous agent's
    uint8_t* const word0 = g.out + (base - lead);                            // that word: 4-byte aligned
    const int nw = (lead + SS + 3) >> 2;
    for (int k = tid; k < nw; k += nthreads) {
        const int c0 = 4 * k - lead;                                         // the word's first cell; < 0 or > SS - 4 at the two ends
        const int cf = c0 < 0 ? 0 : c0;
        int q = cf / S, c = cf - q * S;                                      // (row, column) of cell cf
        uint32_t v = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cell = c0 + j;
            if (cell < cf || cell >= SS) continue;                           // a neighbour's byte
            const T ahead = off[S - 1 - q], lat = off[S - 1 - c];
            const T ax = ahead * d.x, ay = ahead * d.y;
            const T lx = lat * d.y, ly = lat * d.x;
            const T bx = pos.x + ax, by = pos.y + ay;
            const T wx = bx + lx, wy = by - ly;
            const T fx = rfloor(wx), fy = rfloor(wy);
            const bool in = fx >= (T)0 && fx < fH && fy >= (T)0 && fy < fW;  // false for any NaN
            uint32_t b = 0u;
            if (in) {
                const int t = (int)fx + H * (int)fy;                         // in [0, H*W)
                b = SEEN ? (uint32_t)seen[t] : 1u + ((words[t >> 4] >> ((t & 15) * 2)) & 3u);
            }
            v |= b << (8 * j);
            if (++c == S) { c = 0; ++q; }
        }
        uint8_t* const dst = word0 + 4 * (size_t)k;
        if (c0 >= 0 && c0 + 4 <= SS) {
            *reinterpret_cast<uint32_t*>(dst) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j >= 0 && c0 + j < SS) dst[j] = (uint8_t)(v >> (8 * j));
        }
    }
}

template <typename T, bool SEEN>
hipError_t launch(const LocalMapArgs& g, int block, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL((rcw_local_map_kernel<T, SEEN>), dim3(g.B), dim3(block), lds, s, g);
    return hipGetLastError();
}

}  // namespace

size_t rcw_local_map_lds_bytes(const RcwDev& p, int32_t size, bool seen)
{
    const size_t table = (((size_t)size * (p.real64 ? sizeof(double) : sizeof(float)) + 15) >> 4) << 4;
    return table + (seen ? 0 : (((size_t)p.H * p.W + 15) >> 4) * sizeof(uint32_t));
}

hipError_t rcw_launch_local_map(const RcwDev& p, int32_t B, const uint8_t* seen_map, const void* off, int32_t size, uint8_t* out, hipStream_t s)
{
    if (B < 1) return hipSuccess;
    const size_t lds = rcw_local_map_lds_bytes(p, size, seen_map != nullptr);
    const int words = (size * size + 3 + 3) >> 2;                            // (the most an agent's image touches)
    const int block = words >= kLocalBlock ? kLocalBlock : ((words + 63) & ~63);   // a lane a word, whole wavefronts
    const LocalMapArgs g{B, p.H, p.W, size, p.nwords, p.real64 ? (const void*)p.pos64 : (const void*)p.pos, p.dir,
                         p.real64 ? (const void*)p.dir_table64 : (const void*)p.dir_table, p.tile_map, seen_map, off, out};
    if (p.real64) return seen_map ? launch<double, true>(g, block, lds, s) : launch<double, false>(g, block, lds, s);
    return seen_map ? launch<float, true>(g, block, lds, s) : launch<float, false>(g, block, lds, s);
}
