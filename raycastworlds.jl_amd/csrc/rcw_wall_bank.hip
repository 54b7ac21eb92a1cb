// The wall bank (include/rcw.h, rcw_set_wall_bank): L wall layouts resident on the device, one of them drawn for an agent at every start of
// an episode.  Three kernels; nothing else of the library knows about the bank.
//
// rcw_wall_bank_pack_kernel   once per rcw_set_wall_bank: the layouts, UInt8 (H*W, L) as rcw_set_walls takes them, into the tile map's own
//          word format — nwords uint32 a layout, 16 tiles a word, bit 0 of each 2-bit field = WALL, the GOAL bits and the padding past H*W
//          clear (what rcw_set_walls_kernel writes).  A thread a word, 16 byte loads each: paid once, not per episode.
// rcw_wall_bank_kernel<T>     behind the core launches of every call that can move an episode counter.  ONE WAVEFRONT PER AGENT (a 64-thread
//          workgroup: every __syncthreads below orders the wave's own LDS traffic and costs no barrier instruction).  The usual case — the
//          agent has not begun an episode — reads two words (its counter and the recorded one), writes mask[a] = 0 and leaves.  An agent whose
//          counter moved (by one: the kernel runs behind every such call) began episode e = counter - 1 in the launch in front, against the
//          walls it had; that reset is discarded:
//            k       the layout: draw 2^63 of the episode's key — reset_agent's own indices count from 0 and stay far below —, scaled to the
//                    weights' sum, looked up in the cumulative weights by binary search (uniform: scalar registers, log2 L loads);
//            LDS     layout k's words, copied by the whole wave (lane + 64 i: maps of more than 64 words loop);
//            lane 0  puts the counter back to e and runs reset_agent against the LDS copy: the SAME key, draw indices from 0 — the
//                    rejection loops are sequential per agent, so one lane runs them, as in rcw_reset_kernel —, which writes goal, pose,
//                    heading, reward, done and the counter e + 1; then the time limit's two words, wall_layout[a], the recorded counter;
//            HBM     the LDS words (walls + the new goal bit) over the agent's tile map, coalesced: the tile map in HBM is only ever
//                    written whole, no read-modify-write meets the copy;
//          and mask[a] = 1: the host re-casts the masked agents through the existing masked path and repaints their camera view with
//          rcw_wall_bank_paint_kernel below (a handle with a top view: through the existing masked fill, which may carry the drawing).
//          The discarded reset leaves one possible trace, the sticky status word (RCW_WARN_SAMPLER_GAVE_UP is set only over 0).  `status_seen`
//          holds each agent's status word as of its last start here (rcw_clear_error zeroes it with the words): a warning that is there now
//          and was not then can only be the discarded reset's — the restarted agent's action was ignored, no other writer ran — and is
//          taken back before the real reset may set its own.
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

template <typename T>
__global__ __launch_bounds__(kBankBlock) void rcw_wall_bank_kernel(const RcwDev p, const RcwLimit lim, const RcwWallBank b, const int force)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_b[];
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= p.B) return;
    const uint32_t ep = p.episode[a];
    if (!force && b.last_episode[a] == ep) {
        if (lane == 0) b.mask[a] = 0;
        return;
    }
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
    if (lane == 0) {
        if (p.status[a] == RCW_WARN_SAMPLER_GAVE_UP && b.status_seen[a] != RCW_WARN_SAMPLER_GAVE_UP) p.status[a] = 0;
        p.episode[a] = e;
        reset_agent<T>(p, a, lds_b, nullptr);                              // (reads the counter back: e; leaves e + 1)
        lim.episode_steps[a] = 0u;
        lim.truncated[a] = 0;
        b.status_seen[a] = p.status[a];
        b.layout[a] = k;
        b.last_episode[a] = ep;
        b.mask[a] = 1;
    }
    __syncthreads();
    uint32_t* const tm = p.tile_map + (size_t)a * (size_t)p.nwords;
    for (int w = lane; w < p.nwords; w += kBankBlock) tm[w] = lds_b[w];
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

hipError_t rcw_launch_wall_bank(const RcwPlan& p, const RcwWallBank& bank, bool force, hipStream_t s)
{
    if (p.B < 1 || bank.layouts < 1) return hipSuccess;
    const size_t lds = (size_t)p.nwords * sizeof(uint32_t);                 // at most 16 KiB: the largest map rcw_create accepts has 4080 words
    if (p.real64) hipLaunchKernelGGL(rcw_wall_bank_kernel<double>, dim3(p.B), dim3(kBankBlock), lds, s, p, p.limit, bank, force ? 1 : 0);
    else          hipLaunchKernelGGL(rcw_wall_bank_kernel<float>, dim3(p.B), dim3(kBankBlock), lds, s, p, p.limit, bank, force ? 1 : 0);
    return hipGetLastError();
}
