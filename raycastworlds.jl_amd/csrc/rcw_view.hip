// The learner view (rcw_set_learner_view): a uint8 RGB or gray image of every agent, an inverse-depth plane, or both (RGB-D, gray-D),
// area-averaged to (h, w), computed from the compact column descriptors (height_line_pu, colour id) the cast kernel leaves — the UInt32
// camera view is never read.
//
// Contract (include/rcw.h, DESIGN.md §learner view): output row r averages camera rows [⌊r·Hc/h⌋, ⌊(r+1)·Hc/h⌋), output column c
// image columns [⌊c·N/w⌋, ⌊(c+1)·N/w⌋); a channel is (S + ⌊n/2⌋) / n over the box's n pixels, S the sum of R, G, B = the bytes of
// 0x00RRGGBB, or of Y = (77 R + 150 G + 29 B + 128) >> 8 for gray.  Image column k of agent a is ceiling on rows [0, pad), its
// colour on [pad, Hc - pad) and floor from max(pad, Hc - pad) on (pad = column_padding, SR:433-439), so a box's sums follow from
// interval overlaps — O(box width) a pixel, whatever the box's height.
//
// The depth plane D (formats with bit 2, the last channel): a colour row of a column of height_line_pu hl holds Dw = depth_byte(u),
// u = min(max(hl, 0), Hc); a ceiling or floor row y holds De(y) = depth_byte(Hc - 2 min(y, Hc - 1 - y)) — the height a line would need
// for y to be its first or last row; depth_byte(u) = (255 u + ⌊Hc/2⌋) / Hc.  De depends on the row alone, so a column's ceiling and floor
// parts of a box are differences of ONE prefix table of De (RcwView::dsum, Hc + 1 words, built by the host when the view is set), its
// colour part nm · Dw: still O(box width) a pixel.  DEPTH is a template parameter of the four pixel kernels; its `false` instantiations
// are the colour-only kernels, instruction for instruction (profiles/learner_view_depth_isa.txt).  C counts the COLOUR channels there
// (0: depth alone), CT = C + DEPTH the channels written.
//
// Five kernels.  The four that compute pixels share the palette (ViewPalette), the two stack kernels the slot shift (shift_chunk).
//   rcw_view_full_kernel   (h, w) = (Hc, N), one byte a pixel per plane (gray, or RGB in CHW), N a power of two from 16 to 4096,
//                          Hc < 32768: write-bandwidth bound like the camera fill.  A lane owns 16 image columns of one plane and
//                          walks rows, one 16-byte store a row; its 16 columns' (ceiling end, floor start, colour value) are loaded once
//                          an item as 16-bit pairs, and a pair of pixels is two packed subtractions, two shifts and two bit selects.
//                          The items — (agent, plane, block of rows) — are swept by a small fixed grid in order, so the chip writes one
//                          compact moving window; the next item's descriptors are loaded before the current item's stores.
//   rcw_view_agent_kernel  every other size whose per-agent tables fit in LDS (3 words a view column + the box bounds) and whose box
//                          sums fit 32 bits: a workgroup per agent stages (ceiling end, floor start, colour channels) per column once,
//                          then a lane per output pixel (all C channels), 32-bit arithmetic on LDS, byte stores the wavefront coalesces.
//   rcw_view_box_kernel    the rest (huge boxes, huge views): a lane per output pixel reading the descriptor arrays directly, 64-bit
//                          sums where a box's could pass 2^31.
//   With DEPTH: the full kernel takes the depth plane as one more plane item (per-row De for ceiling and floor, per-column Dw); the
//   agent kernels keep Dw in the free top byte of a column's packed channels and dsum behind the box bounds in LDS (Hc + 1 more words:
//   geometries that no longer fit go to the box kernel), the box kernel reads dsum from the handle's device table; HWC RGB-D is one
//   4-byte store a pixel.
// and, for a stack of the last k frames an agent (rcw_set_learner_view_stack, k > 1, layout CHW):
//   rcw_view_agent_push_kernel  rcw_view_agent_kernel with the push inside: the old slots move down one while the tables are staged, the
//                          pixels go to the newest slot (or to all k: a refill, an episode that restarted in this step).
//   rcw_view_push_kernel   behind the other two kernels, which write a staging frame: a workgroup an agent shifts the slots and appends
//                          the staged frame (or writes it k times), 16-byte chunks where a frame is a multiple of 16 bytes.
#include "rcw_device.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int kViewFullPasses = 8;   // rows a lane stores an item (an item = 8 x 4 KiB of one plane)

// the channel k of a colour: R, G, B bytes, or the luma Y for gray
template <int C>
__device__ __forceinline__ uint32_t view_channel(uint32_t colour, int k)
{
    const uint32_t R = (colour >> 16) & 0xFFu, G = (colour >> 8) & 0xFFu, B = colour & 0xFFu;
    if (C == 1) return (77u * R + 150u * G + 29u * B + 128u) >> 8;
    return k == 0 ? R : (k == 1 ? G : B);
}

// the channel values every pixel kernel works with: ceiling, floor, and the four colours' a byte each (colour id `id` at bits [8 id, 8 id + 8))
template <int C>
struct ViewPalette {
    static constexpr int CA = C > 0 ? C : 1;            // (C = 0, depth alone: one unused entry)
    uint32_t vc[CA], vf[CA], vm4[CA];
    __device__ __forceinline__ explicit ViewPalette(const RcwDev& p)
    {
#pragma unroll
        for (int k = 0; k < CA; ++k) {
            vc[k] = view_channel<C>(p.ceiling_color, k);
            vf[k] = view_channel<C>(p.floor_color, k);
            vm4[k] = 0u;
#pragma unroll
            for (int id = 0; id < 4; ++id) vm4[k] |= view_channel<C>(p.colour[id], k) << (8 * id);
        }
    }
};

typedef short s16x2 __attribute__((ext_vector_type(2)));

// column_padding in 32-bit arithmetic for Hc < 32768 (a height far below zero pads the whole column, as there)
__device__ __forceinline__ int padding32(int Hc, int h)
{
    return h >= Hc - 1 ? 0 : min((Hc - max(h, -Hc)) >> 1, Hc);
}

__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

// The depth byte of an inverse depth of u pixels, 0 <= u <= Hc: (255 u + ⌊Hc/2⌋) / Hc (fast_div: Hc <= 2^20, so the dividend is below
// 2^28 and the Float32 quotient, at most 255, is off by less than one).
__device__ __forceinline__ uint32_t depth_byte(int u, int Hc, float inv_Hc) { return (uint32_t)fast_div(255 * u + (Hc >> 1), Hc, inv_Hc); }
__device__ __forceinline__ uint32_t depth_wall(int hl, int Hc, float inv_Hc) { return depth_byte(min(max(hl, 0), Hc), Hc, inv_Hc); }        // Dw
__device__ __forceinline__ uint32_t depth_edge(int y, int Hc, float inv_Hc) { return depth_byte(Hc - 2 * min(y, Hc - 1 - y), Hc, inv_Hc); }  // De(y)

// The depth sum of rows [r0, r1) of one column: its ceiling rows [r0, min(r1, pad)) and floor rows [max(r0, fs), r1) from the prefix table
// ds of De (e0 = ds[r0], e1 = ds[r1]), its nm colour rows dw each.
template <typename Acc>
__device__ __forceinline__ Acc depth_rows(const int32_t* ds, int e0, int e1, int r0, int r1, int pad, int fs, Acc nm, uint32_t dw)
{
    return (Acc)(uint32_t)(ds[max(r0, min(r1, pad))] - e0) + nm * dw + (Acc)(uint32_t)(e1 - ds[min(r1, max(r0, fs))]);
}

// 16 columns of one agent: ceiling end, floor start, colour value as 16-bit pairs (column 2j low, 2j + 1 high)
struct FullCols { uint32_t lo[8], hi[8], vm[8]; };

__device__ __forceinline__ void full_cols(FullCols& f, const int4 (&hq)[4], uint4 ids, int Hc, uint32_t vm4)
{
    const uint32_t idw[4] = {ids.x, ids.y, ids.z, ids.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int4 q = hq[j >> 1];
        const int h0 = (j & 1) ? q.z : q.x, h1 = (j & 1) ? q.w : q.y;
        const int p0 = padding32(Hc, h0), p1 = padding32(Hc, h1);
        f.lo[j] = pack16(p0, p1);
        f.hi[j] = pack16(max(p0, Hc - p0), max(p1, Hc - p1));
        const uint32_t id0 = (idw[j >> 1] >> ((j & 1) * 16)) & 3u, id1 = (idw[j >> 1] >> ((j & 1) * 16 + 8)) & 3u;
        f.vm[j] = pack16((int)((vm4 >> (8 * id0)) & 0xFFu), (int)((vm4 >> (8 * id1)) & 0xFFu));
    }
}

// ... of the depth plane: the value is the column's Dw
__device__ __forceinline__ void full_cols_depth(FullCols& f, const int4 (&hq)[4], int Hc, float inv_Hc)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int4 q = hq[j >> 1];
        const int h0 = (j & 1) ? q.z : q.x, h1 = (j & 1) ? q.w : q.y;
        const int p0 = padding32(Hc, h0), p1 = padding32(Hc, h1);
        f.lo[j] = pack16(p0, p1);
        f.hi[j] = pack16(max(p0, Hc - p0), max(p1, Hc - p1));
        f.vm[j] = pack16((int)depth_wall(h0, Hc, inv_Hc), (int)depth_wall(h1, Hc, inv_Hc));
    }
}

template <int C, bool DEPTH>
__global__ __launch_bounds__(kBlock) void rcw_view_full_kernel(const RcwDev p, const int32_t* __restrict__ col_h,
                                                               const uint8_t* __restrict__ col_c, u32x4* __restrict__ out,
                                                               int32_t count, const uint8_t* __restrict__ mask, int l_shift,
                                                               int blocks_per_plane)
{
    const int N = p.N, Hc = p.Hc;
    const int L = 1 << l_shift;                               // lanes a row: N / 16
    const int tid = threadIdx.x;
    const int cb = tid & (L - 1);                             // this lane's columns [16 cb, 16 cb + 16)
    const int rows_pass = kBlock >> l_shift;
    const int row_lane = tid >> l_shift;
    constexpr int CT = C + (DEPTH ? 1 : 0), CA = ViewPalette<C>::CA;   // planes an agent: the colour's, then the depth plane
    const uint32_t items = (uint32_t)count * CT * (uint32_t)blocks_per_plane;   // (< 2^31: rcw_launch_view)
    const ViewPalette<C> pal(p);
    const float inv_Hc = 1.0f / (float)Hc;                    // (DEPTH only)
    uint32_t vc[CA], vf[CA];                                  // ceiling and floor in both halves of a 16-bit pair
#pragma unroll
    for (int k = 0; k < CA; ++k) { vc[k] = pal.vc[k] * 0x00010001u; vf[k] = pal.vf[k] * 0x00010001u; }
    uint32_t it = blockIdx.x;
    int4 hq[4];
    uint4 ids;
    auto load = [&](uint32_t item) {                         // the raw descriptors of the item's agent, this lane's columns
        const long long a = item / ((uint32_t)CT * (uint32_t)blocks_per_plane);
        const int4* hsrc = reinterpret_cast<const int4*>(col_h + a * N + cb * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) hq[q] = hsrc[q];
        ids = *reinterpret_cast<const uint4*>(col_c + a * N + cb * 16);
    };
    if (it < items) load(it);
    for (; it < items; it += gridDim.x) {
        const uint32_t pl = it / (uint32_t)blocks_per_plane;
        const int blk = (int)(it - pl * (uint32_t)blocks_per_plane);
        const uint32_t a = pl / CT;
        const int ch = (int)(pl - a * CT);
        const bool dpl = DEPTH && ch == C;                    // the depth plane (the same for the whole workgroup)
        uint32_t vmc = pal.vm4[0], vcc = vc[0], vfc = vf[0];
#pragma unroll
        for (int k = 1; k < C; ++k) if (ch == k) { vmc = pal.vm4[k]; vcc = vc[k]; vfc = vf[k]; }
        FullCols f;
        if (dpl) full_cols_depth(f, hq, Hc, inv_Hc); else full_cols(f, hq, ids, Hc, vmc);
        if (it + gridDim.x < items) load(it + gridDim.x);    // (in flight during this item's stores)
        if (mask != nullptr && mask[a] == 0) continue;
        u32x4* const dst = out + (unsigned long long)pl * (unsigned long long)Hc * L + cb;
        const int r0 = blk * rows_pass * kViewFullPasses + row_lane;
#pragma unroll 2
        for (int q = 0; q < kViewFullPasses; ++q) {
            const int r = r0 + q * rows_pass;
            if (r >= Hc) break;
            if (dpl) vcc = vfc = depth_edge(r, Hc, inv_Hc) * 0x00010001u;   // ceiling and floor: this row's De
            const s16x2 rr = {(short)r, (short)r};
            uint32_t val[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const s16x2 dc = (rr - __builtin_bit_cast(s16x2, f.lo[j])) >> (short)15;   // 0xFFFF where r < ceiling end
                const s16x2 df = (rr - __builtin_bit_cast(s16x2, f.hi[j])) >> (short)15;   // 0xFFFF where r < floor start
                const uint32_t mc = __builtin_bit_cast(uint32_t, dc), mf = __builtin_bit_cast(uint32_t, df);
                const uint32_t t = (mf & f.vm[j]) | (~mf & vfc);
                val[j] = (mc & vcc) | (~mc & t);
            }
            u32x4 v;
            v.x = __builtin_amdgcn_perm(val[1], val[0], 0x06040200u);
            v.y = __builtin_amdgcn_perm(val[3], val[2], 0x06040200u);
            v.z = __builtin_amdgcn_perm(val[5], val[4], 0x06040200u);
            v.w = __builtin_amdgcn_perm(val[7], val[6], 0x06040200u);
            store16<false>(dst + (long long)r * L, v);
        }
    }
}

// (S + ⌊n/2⌋) / n: the Float32 quotient corrected by one either way (fast_div, rcw_device.h: S + n/2 < 2^31, quotient <= 255)
__device__ __forceinline__ uint32_t view_div(uint32_t s, uint32_t n)
{
    return (uint32_t)fast_div((int)(s + (n >> 1)), (int)n, __builtin_amdgcn_rcpf((float)n));
}
__device__ __forceinline__ uint32_t view_div(unsigned long long s, unsigned long long n) { return (uint32_t)((s + (n >> 1)) / n); }

template <int C, bool HWC, bool WIDE, bool DEPTH>
__global__ __launch_bounds__(kBlock) void rcw_view_box_kernel(const RcwDev p, const RcwView v, const int32_t* __restrict__ col_h,
                                                              const uint8_t* __restrict__ col_c, int32_t count,
                                                              const uint8_t* __restrict__ mask, uint8_t* __restrict__ out)
{
    typedef typename std::conditional<WIDE, unsigned long long, uint32_t>::type Acc;
    const int N = p.N, Hc = p.Hc, h = v.h, w = v.w;
    const long long hw = (long long)h * w;
    const long long total = (long long)count * hw;
    const long long S = (long long)gridDim.x * kBlock;
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    // (agent, row, column) of this lane's pixel, moved on by S pixels a trip without a division
    long long a = i / hw;
    int r = (int)((i - a * hw) / w), c = (int)(i - a * hw - (long long)r * w);
    const long long Sa = S / hw;
    const int Sr = (int)((S - Sa * hw) / w), Sc = (int)(S - Sa * hw - (long long)Sr * w);
    constexpr int CT = C + (DEPTH ? 1 : 0), CA = ViewPalette<C>::CA;
    const ViewPalette<C> pal(p);
    const float inv_Hc = 1.0f / (float)Hc;                    // (DEPTH only, as the three below)
    const int32_t* const ds = v.dsum;
    const bool word = DEPTH && HWC && C == 3 && ((uintptr_t)out & 3u) == 0;   // RGB-D pixels as one 4-byte store
    for (; i < total; i += S) {
        if (mask == nullptr || mask[a] != 0) {
            const int r0 = v.rows[r], r1 = v.rows[r + 1], c0 = v.cols[c], c1 = v.cols[c + 1];
            const int nr = r1 - r0;
            Acc acc[CA], accd = 0;
            int e0 = 0, e1 = 0;
            if (DEPTH) { e0 = ds[r0]; e1 = ds[r1]; }
#pragma unroll
            for (int k = 0; k < C; ++k) acc[k] = 0;
            const int32_t* const hp = col_h + a * N;
            const uint8_t* const cp = col_c + a * N;
#pragma unroll 4
            for (int j = c0; j < c1; ++j) {
                const int hl = hp[j];
                const int pad = column_padding(Hc, hl);
                const uint32_t sh = 8u * (cp[j] & 3u);
                const int nc = max(0, min(r1, pad) - r0);                    // ceiling rows [0, pad)
                const int nf = max(0, r1 - max(r0, max(pad, Hc - pad)));    // floor rows [max(pad, Hc - pad), Hc)
                const int nm = nr - nc - nf;                                 // the colour's rows between
#pragma unroll
                for (int k = 0; k < C; ++k)
                    acc[k] += (Acc)nc * pal.vc[k] + (Acc)nm * ((pal.vm4[k] >> sh) & 0xFFu) + (Acc)nf * pal.vf[k];
                if (DEPTH) accd += depth_rows<Acc>(ds, e0, e1, r0, r1, pad, max(pad, Hc - pad), (Acc)nm, depth_wall(hl, Hc, inv_Hc));
            }
            const Acc n = (Acc)nr * (Acc)(c1 - c0);
            if (HWC) {
                uint8_t* const o = out + ((unsigned long long)(a * h + r) * w + c) * CT;
                if (word) {
                    uint32_t px = view_div(accd, n) << 24;
#pragma unroll
                    for (int k = 0; k < C; ++k) px |= view_div(acc[k], n) << (8 * k);
                    *reinterpret_cast<uint32_t*>(o) = px;
                } else {
#pragma unroll
                    for (int k = 0; k < C; ++k) o[k] = (uint8_t)view_div(acc[k], n);
                    if (DEPTH) o[C] = (uint8_t)view_div(accd, n);
                }
            } else {
#pragma unroll
                for (int k = 0; k < C; ++k) out[((unsigned long long)(a * CT + k) * h + r) * w + c] = (uint8_t)view_div(acc[k], n);
                if (DEPTH) out[((unsigned long long)(a * CT + C) * h + r) * w + c] = (uint8_t)view_div(accd, n);
            }
        }
        c += Sc; if (c >= w) { c -= w; r += 1; }
        r += Sr; if (r >= h) { r -= h; a += 1; }
        a += Sa;
    }
}

// One chunk of every slot of an agent's stack (slot s at c + s * per_v): slots 0 .. k - 2 take their successors in ascending order, four
// loads, then their four stores.  A lane moves the SAME chunk of every slot and no other lane touches that chunk, so the shift in place
// needs no barrier.  shift_slots: every chunk of the agent's stack, a lane a chunk.
template <typename V>
__device__ __forceinline__ void shift_chunk(V* c, int per_v, int k)
{
    for (int s = 0; s + 1 < k; s += 4) {
        V t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (s + j + 1 < k) t[j] = c[(long long)(s + j + 1) * per_v];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (s + j + 1 < k) c[(long long)(s + j) * per_v] = t[j];
    }
}

template <typename V>
__device__ __forceinline__ void shift_slots(V* base, int per_v, int k, int tid)
{
    for (int i = tid; i < per_v; i += kBlock) shift_chunk(base + i, per_v, k);
}

// One image column's share of an agent-kernel pixel's colour sums (a macro, not a function: DESIGN.md §4.6.1 on what a function boundary does
// to the gray instantiations' registers).  The depth instantiations run it in a loop of their own, so that its unrolling can be chosen for them
// alone and the colour-only loop stays the compiler's: unrolled by 8 (51 / 65 / 57 VGPRs for depth / gray-D / RGB-D) it is 12-15 % faster than the
// compiler's 16-wide form (77 / 118 / 44) and than 1 or 4 (profiles/learner_view_depth_bench.txt (3)).
#define RCW_VIEW_AGENT_COLUMN(j)                                                                                              \
    const int pad = s_pad[j], fs = s_fs[j];                                                                                   \
    const uint32_t m = s_vm[j];                                                                                               \
    const uint32_t nc = (uint32_t)max(0, min(r1, pad) - r0);                                                                  \
    const uint32_t nf = (uint32_t)max(0, r1 - max(r0, fs));                                                                   \
    const uint32_t nm = (uint32_t)nr - nc - nf;                                                                               \
    _Pragma("unroll")                                                                                                         \
    for (int k = 0; k < C; ++k) acc[k] += nc * pal.vc[k] + nm * ((m >> (8 * k)) & 0xFFu) + nf * pal.vf[k];

// A workgroup per agent for the reduced sizes whose tables fit in LDS: the agent's columns are turned into (ceiling end, floor start,
// packed colour channels) once, the box bounds staged beside them, and every output pixel of the agent is then 32-bit arithmetic on LDS.
template <int C, bool HWC, bool DEPTH>
__global__ __launch_bounds__(kBlock) void rcw_view_agent_kernel(const RcwDev p, const RcwView v, const int32_t* __restrict__ col_h,
                                                                const uint8_t* __restrict__ col_c, const uint8_t* __restrict__ mask,
                                                                uint8_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds_v[];
    const int N = p.N, Hc = p.Hc, h = v.h, w = v.w, tid = threadIdx.x;
    const long long a = blockIdx.x;
    if (mask != nullptr && mask[a] == 0) return;
    int32_t* const s_pad = lds_v;
    int32_t* const s_fs = s_pad + N;
    uint32_t* const s_vm = reinterpret_cast<uint32_t*>(s_fs + N);        // the colour's C channel values, a byte each (DEPTH: Dw in byte 3)
    int32_t* const s_rows = reinterpret_cast<int32_t*>(s_vm + N);
    int32_t* const s_cols = s_rows + h + 1;
    int32_t* const s_ds = s_cols + w + 1;                                 // DEPTH: the prefix sums of De, Hc + 1 words
    constexpr int CT = C + (DEPTH ? 1 : 0), CA = ViewPalette<C>::CA;
    const float inv_Hc = 1.0f / (float)Hc;                               // (DEPTH only)
    const ViewPalette<C> pal(p);
    for (int j = tid; j < N; j += kBlock) {
        const int hl = col_h[a * N + j];
        const int pad = column_padding(Hc, hl);
        const uint32_t sh = 8u * (col_c[a * N + j] & 3u);
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < C; ++k) m |= ((pal.vm4[k] >> sh) & 0xFFu) << (8 * k);
        if (DEPTH) m |= depth_wall(hl, Hc, inv_Hc) << 24;
        s_pad[j] = pad; s_fs[j] = max(pad, Hc - pad); s_vm[j] = m;
    }
    for (int j = tid; j <= h; j += kBlock) s_rows[j] = v.rows[j];
    for (int j = tid; j <= w; j += kBlock) s_cols[j] = v.cols[j];
    if (DEPTH) for (int j = tid; j <= Hc; j += kBlock) s_ds[j] = v.dsum[j];
    __syncthreads();
    const int hw = h * w;
    const float inv_w = 1.0f / (float)w;
    uint8_t* const o = out + (unsigned long long)a * CT * hw;
    const bool word = DEPTH && HWC && C == 3 && ((uintptr_t)out & 3u) == 0;   // RGB-D pixels as one 4-byte store
    for (int i = tid; i < hw; i += kBlock) {
        const int r = fast_div(i, w, inv_w), c = i - r * w;                   // (hw < 2^23: rcw_launch_view)
        const int r0 = s_rows[r], r1 = s_rows[r + 1], c0 = s_cols[c], c1 = s_cols[c + 1];
        const int nr = r1 - r0;
        uint32_t acc[CA], accd = 0u;
        int e0 = 0, e1 = 0;
        if (DEPTH) { e0 = s_ds[r0]; e1 = s_ds[r1]; }
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = 0u;
        if (DEPTH) {
#pragma unroll 8
            for (int j = c0; j < c1; ++j) { RCW_VIEW_AGENT_COLUMN(j) accd += depth_rows<uint32_t>(s_ds, e0, e1, r0, r1, pad, fs, nm, m >> 24); }
        } else {
            for (int j = c0; j < c1; ++j) { RCW_VIEW_AGENT_COLUMN(j) }
        }
        const uint32_t n = (uint32_t)nr * (uint32_t)(c1 - c0);
        if (word) {
            uint32_t px = view_div(accd, n) << 24;
#pragma unroll
            for (int k = 0; k < C; ++k) px |= view_div(acc[k], n) << (8 * k);
            reinterpret_cast<uint32_t*>(o)[i] = px;
            continue;
        }
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const uint8_t q = (uint8_t)view_div(acc[k], n);
            if (HWC) o[(unsigned)i * CT + k] = q; else o[(unsigned)(k * hw + i)] = q;
        }
        if (DEPTH) {
            const uint8_t q = (uint8_t)view_div(accd, n);
            if (HWC) o[(unsigned)i * CT + C] = q; else o[(unsigned)(C * hw + i)] = q;
        }
    }
}

// rcw_view_agent_kernel with the k-frame stack's push inside (rcw_set_learner_view_stack at these sizes, layout CHW): `stack` is the batch of
// k slots an agent.  While the tables are staged the old slots move down one (shift_slots); the barrier the staging needs anyway also puts
// every read of slot k - 1 in front of the stores that follow; each pixel, computed once as above, goes to slot k - 1 — or to all k slots on a
// refill or when the agent's episode counter is not the one recorded at its previous push (rcw_view_push_kernel below states the rule).
// Against that kernel behind rcw_view_agent_kernel this saves a launch, and the staged frame's store and load.
// The staging and the pixel loop are rcw_view_agent_kernel's, COPIED — a fix to one is owed to the other.  Behind any function boundary the
// gray instantiations of both kernels take 74 VGPRs for 62 / 63, six waves a SIMD for eight: the compiler's 16-wide form of the column
// loop sits at that edge and its schedule follows the order of the blocks around it.
struct RcwViewStack {
    int k, refill;                  // slots an agent; 1: reset / set_state / a new view — all k slots take the frame
    const uint32_t* episode;        // the agents' episode counters now
    uint32_t* last_episode;         // ... as of their previous push (updated)
};

template <int C, bool DEPTH>
__global__ __launch_bounds__(kBlock) void rcw_view_agent_push_kernel(const RcwDev p, const RcwView v, const int32_t* __restrict__ col_h,
                                                                     const uint8_t* __restrict__ col_c, const uint8_t* __restrict__ mask,
                                                                     uint8_t* __restrict__ stack, const RcwViewStack st)
{
    extern __shared__ __attribute__((aligned(16))) int32_t lds_v[];
    const int N = p.N, Hc = p.Hc, h = v.h, w = v.w, tid = threadIdx.x;
    const long long a = blockIdx.x;
    if (mask != nullptr && mask[a] == 0) return;
    const uint32_t ep = st.episode[a];
    const bool all = st.refill || st.last_episode[a] != ep;
    int32_t* const s_pad = lds_v;
    int32_t* const s_fs = s_pad + N;
    uint32_t* const s_vm = reinterpret_cast<uint32_t*>(s_fs + N);
    int32_t* const s_rows = reinterpret_cast<int32_t*>(s_vm + N);
    int32_t* const s_cols = s_rows + h + 1;
    int32_t* const s_ds = s_cols + w + 1;
    constexpr int CT = C + (DEPTH ? 1 : 0), CA = ViewPalette<C>::CA;
    const float inv_Hc = 1.0f / (float)Hc;
    const ViewPalette<C> pal(p);
    for (int j = tid; j < N; j += kBlock) {
        const int hl = col_h[a * N + j];
        const int pad = column_padding(Hc, hl);
        const uint32_t sh = 8u * (col_c[a * N + j] & 3u);
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < C; ++k) m |= ((pal.vm4[k] >> sh) & 0xFFu) << (8 * k);
        if (DEPTH) m |= depth_wall(hl, Hc, inv_Hc) << 24;
        s_pad[j] = pad; s_fs[j] = max(pad, Hc - pad); s_vm[j] = m;
    }
    for (int j = tid; j <= h; j += kBlock) s_rows[j] = v.rows[j];
    for (int j = tid; j <= w; j += kBlock) s_cols[j] = v.cols[j];
    if (DEPTH) for (int j = tid; j <= Hc; j += kBlock) s_ds[j] = v.dsum[j];
    const int hw = h * w, per = CT * hw;
    uint8_t* const base = stack + (unsigned long long)a * st.k * per;
    if (!all) {
        if ((per & 15) == 0) shift_slots(reinterpret_cast<u32x4*>(base), per >> 4, st.k, tid);   // (the batch is 16-byte aligned: rcw_launch_view_stack)
        else shift_slots(base, per, st.k, tid);
    }
    __syncthreads();
    if (tid == 0) st.last_episode[a] = ep;
    const float inv_w = 1.0f / (float)w;
    uint8_t* const o = all ? base : base + (unsigned long long)(st.k - 1) * per;
    const int copies = all ? st.k : 1;
    for (int i = tid; i < hw; i += kBlock) {
        const int r = fast_div(i, w, inv_w), c = i - r * w;
        const int r0 = s_rows[r], r1 = s_rows[r + 1], c0 = s_cols[c], c1 = s_cols[c + 1];
        const int nr = r1 - r0;
        uint32_t acc[CA], accd = 0u;
        int e0 = 0, e1 = 0;
        if (DEPTH) { e0 = s_ds[r0]; e1 = s_ds[r1]; }
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = 0u;
        if (DEPTH) {
#pragma unroll 8
            for (int j = c0; j < c1; ++j) { RCW_VIEW_AGENT_COLUMN(j) accd += depth_rows<uint32_t>(s_ds, e0, e1, r0, r1, pad, fs, nm, m >> 24); }
        } else {
            for (int j = c0; j < c1; ++j) { RCW_VIEW_AGENT_COLUMN(j) }
        }
        const uint32_t n = (uint32_t)nr * (uint32_t)(c1 - c0);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const uint8_t q = (uint8_t)view_div(acc[k], n);
            for (int s = 0; s < copies; ++s) o[(unsigned)(s * per + k * hw + i)] = q;
        }
        if (DEPTH) {
            const uint8_t q = (uint8_t)view_div(accd, n);
            for (int s = 0; s < copies; ++s) o[(unsigned)(s * per + C * hw + i)] = q;
        }
    }
}

// The k-frame stack (rcw_set_learner_view_stack, frames = k > 1): the view kernels above keep writing the single frame into the staging
// batch; this kernel, behind them, moves it into the agent's k slots of `per` bytes each (slot 0 the oldest).  A refill (reset / set_state /
// setting the view: the masked agents) or an agent whose episode counter differs from the one recorded at its previous push (auto_reset
// re-sampled it in this step) takes the staged frame k times; every other agent's slots shift (shift_chunk) and slot k - 1 takes the
// staged frame.  A workgroup owns an agent: all its lanes read the recorded counter, the barrier, then lane 0 records the new one.
// V: 16-byte chunks where per is a multiple of 16, bytes otherwise.
template <typename V>
__global__ __launch_bounds__(kBlock) void rcw_view_push_kernel(const V* __restrict__ staged, V* stack, const uint32_t* __restrict__ episode,
                                                               uint32_t* last_episode, const uint8_t* __restrict__ mask, int per_v, int k,
                                                               int refill)
{
    const long long a = blockIdx.x;
    if (mask != nullptr && mask[a] == 0) return;
    const uint32_t ep = episode[a];
    const bool all = refill || last_episode[a] != ep;
    __syncthreads();
    if (threadIdx.x == 0) last_episode[a] = ep;
    const V* const src = staged + a * per_v;
    V* const dst = stack + a * k * per_v;
    for (int i = threadIdx.x; i < per_v; i += kBlock) {
        V* const c = dst + i;
        const V f = src[i];
        if (all) {
            for (int s = 0; s < k; ++s) c[(long long)s * per_v] = f;
            continue;
        }
        shift_chunk(c, per_v, k);
        c[(long long)(k - 1) * per_v] = f;
    }
}

}  // namespace

// the LDS bytes of rcw_view_agent_kernel's tables for this view, 0 where it does not take it (the tables beyond 64 KiB, 64-bit box sums)
static size_t view_agent_lds(const RcwDev& p, const RcwView& v)
{
    const size_t lds = ((size_t)3 * p.N + v.h + v.w + 2 + (v.depth ? (size_t)p.Hc + 1 : 0)) * sizeof(int32_t);   // (+ the prefix sums of De)
    return !v.wide && (long long)v.h * v.w < (1ll << 23) && lds <= 64 * 1024 ? lds : 0;
}

// rcw_launch_view's first choice: the full-size kernel, for 16-byte aligned buffers and fewer than 2^31 items
static bool view_takes_full_kernel(const RcwDev& p, const RcwView& v, const int32_t* col_h, const uint8_t* col_c, int32_t count,
                                   const uint8_t* out)
{
    const bool aligned = (((uintptr_t)col_h | (uintptr_t)col_c | (uintptr_t)out) & 15u) == 0;
    return v.full_ok && aligned && (long long)count * v.C * ((p.Hc + 7) / 8) < (1ll << 31);
}

int rcw_view_full_eligible(const RcwDev& p, int C, int hwc)
{
    return (C == 1 || !hwc) && p.N >= 16 && p.N <= 4096 && (p.N & (p.N - 1)) == 0 && p.Hc < 32768 ? 1 : 0;
}

// launch(C, HWC, DEPTH) as integral constants, C the colour channels: the instances the agent and box kernels exist for (the two layouts of
// one channel coincide: HWC = false)
template <typename Launch>
static void view_instance(const RcwView& v, Launch launch)
{
    typedef std::integral_constant<int, 0> C0;
    typedef std::integral_constant<int, 1> C1;
    typedef std::integral_constant<int, 3> C3;
    const std::true_type yes{};
    const std::false_type no{};
    if (!v.depth) {
        if (v.C == 1) launch(C1{}, no, no);
        else if (v.hwc) launch(C3{}, yes, no);
        else launch(C3{}, no, no);
    }
    else if (v.C == 1) launch(C0{}, no, yes);
    else if (v.C == 2) { if (v.hwc) launch(C1{}, yes, yes); else launch(C1{}, no, yes); }
    else               { if (v.hwc) launch(C3{}, yes, yes); else launch(C3{}, no, yes); }
}

hipError_t rcw_launch_view(const RcwPlan& p, const RcwView& v, const int32_t* col_h, const uint8_t* col_c, int32_t count,
                           const uint8_t* mask_dev, uint8_t* out, hipStream_t s)
{
    if (count < 1) return hipSuccess;
    if (view_takes_full_kernel(p, v, col_h, col_c, count, out)) {
        int l_shift = 0;
        while ((16 << l_shift) < p.N) ++l_shift;
        const int rows_item = (kBlock >> l_shift) * kViewFullPasses;
        const int blocks_per_plane = (p.Hc + rows_item - 1) / rows_item;
        const long long items = (long long)count * v.C * blocks_per_plane;
        const int grid = (int)std::min<long long>(items, 4ll * p.fill_grid);
        u32x4* const o4 = reinterpret_cast<u32x4*>(out);
        view_instance(v, [&](auto c, auto, auto depth) {                  // (planes only: the layout does not matter)
            hipLaunchKernelGGL((rcw_view_full_kernel<decltype(c)::value, decltype(depth)::value>), dim3(grid), dim3(kBlock), 0, s, p, col_h, col_c, o4, count, mask_dev, l_shift, blocks_per_plane);
        });
        return hipGetLastError();
    }
    const size_t lds = view_agent_lds(p, v);
    if (lds != 0) {
        view_instance(v, [&](auto c, auto hwc, auto depth) {
            hipLaunchKernelGGL((rcw_view_agent_kernel<decltype(c)::value, decltype(hwc)::value, decltype(depth)::value>), dim3(count), dim3(kBlock), lds, s, p, v, col_h, col_c, mask_dev, out);
        });
        return hipGetLastError();
    }
    const long long total = (long long)count * v.h * v.w;
    const int grid = (int)std::min<long long>((total + kBlock - 1) / kBlock, 1ll << 24);   // (a lane a pixel: every load of the batch in flight at once)
    view_instance(v, [&](auto c, auto hwc, auto depth) {
        constexpr int C = decltype(c)::value;
        constexpr bool HWC = decltype(hwc)::value, DEPTH = decltype(depth)::value;
        if (v.wide) hipLaunchKernelGGL((rcw_view_box_kernel<C, HWC, true, DEPTH>), dim3(grid), dim3(kBlock), 0, s, p, v, col_h, col_c, count, mask_dev, out);
        else        hipLaunchKernelGGL((rcw_view_box_kernel<C, HWC, false, DEPTH>), dim3(grid), dim3(kBlock), 0, s, p, v, col_h, col_c, count, mask_dev, out);
    });
    return hipGetLastError();
}

hipError_t rcw_launch_view_stack(const RcwPlan& p, const RcwView& v, const int32_t* col_h, const uint8_t* col_c, int32_t count, int frames,
                                 const uint8_t* mask_dev, uint8_t* staged, uint8_t* stack, const uint32_t* episode, uint32_t* last_episode,
                                 bool refill, hipStream_t s)
{
    if (count < 1 || frames < 2) return hipSuccess;
    const bool full = view_takes_full_kernel(p, v, col_h, col_c, count, staged);
    const size_t lds = view_agent_lds(p, v);
    if (!full && lds != 0 && !v.hwc && ((uintptr_t)stack & 15u) == 0) {
        const RcwViewStack st{frames, refill ? 1 : 0, episode, last_episode};
        view_instance(v, [&](auto c, auto, auto depth) {                      // (CHW)
            hipLaunchKernelGGL((rcw_view_agent_push_kernel<decltype(c)::value, decltype(depth)::value>), dim3(count), dim3(kBlock), lds, s, p, v, col_h, col_c, mask_dev, stack, st);
        });
        return hipGetLastError();
    }
    const hipError_t e = rcw_launch_view(p, v, col_h, col_c, count, mask_dev, staged, s);
    if (e != hipSuccess) return e;
    const long long per = (long long)v.C * v.h * v.w;           // (< 2^31: a frame of at most 2^20 x num_rays pixels — rcw_set_learner_view_stack)
    if ((per & 15) == 0 && (((uintptr_t)staged | (uintptr_t)stack) & 15u) == 0)
        hipLaunchKernelGGL(rcw_view_push_kernel<u32x4>, dim3(count), dim3(kBlock), 0, s, reinterpret_cast<const u32x4*>(staged),
                           reinterpret_cast<u32x4*>(stack), episode, last_episode, mask_dev, (int)(per >> 4), frames, refill ? 1 : 0);
    else
        hipLaunchKernelGGL(rcw_view_push_kernel<uint8_t>, dim3(count), dim3(kBlock), 0, s, staged, stack, episode, last_episode, mask_dev,
                           (int)per, frames, refill ? 1 : 0);
    return hipGetLastError();
}
