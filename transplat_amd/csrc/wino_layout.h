// Sources, tile-block geometry and packed-filter layout of the 3x3 Winograd F(2x2, 3x3) family
// (winoconv.hip exact fp32, winoconv3.hip split bf16; convfew.hip shares the source marshalling): the
// limits, the source list every launcher fills and validates, the tile-block search, and where a
// transformed filter value lands in each precision's packed U (the weight kernels write through it).
// Plain C++ apart from the function qualifiers, so a host compiler can build it too
// (tests/wino_layout_check.cc).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TSPLAT_WL_HD __host__ __device__ __forceinline__
#else
#define TSPLAT_WL_HD inline
#endif

namespace tsplat {
namespace wino_layout {

constexpr int kMaxSrc = 6;          // input sources concatenated along channels (read in place)
constexpr int kMaxCiPad = 1024;     // input channels (padded to 16) of one launch: the plane table's size
constexpr int kPersistCiPad = 512;  // the persistent form's plane table (keeps it at 2 workgroups / CU)

// input channels are padded to the 16-channel group, output channels to 64 (an even number of
// 32-channel blocks, so every workgroup shape reads the same packing)
TSPLAT_WL_HD int ci_pad(int ci) { return (ci + 15) / 16 * 16; }
TSPLAT_WL_HD int cobs(int co) { return (co + 63) / 64 * 2; }

// ---- sources: source s is [n][cs[s]][h][w]; channel c of the convolution's input is channel
// c - (cs[0] + .. + cs[s-1]) of the source it falls in. The leading fields of every kernel's Args.
struct Sources {
    const float* src[kMaxSrc];
    int cs[kMaxSrc];
    int nsrc;
    int ci;  // cs[0] + .. + cs[nsrc-1]
};

// the one place a Sources is filled; false for a null list or entry, a non-positive channel count,
// nsrc outside 1 .. kMaxSrc, or (align16: the kernel moves float4) a source that is not 16-B aligned
inline bool fill_sources(Sources& s, const float* const* srcs, const int32_t* chans, int nsrc, bool align16 = false) {
    if (!srcs || !chans || nsrc <= 0 || nsrc > kMaxSrc) return false;
    s.nsrc = nsrc;
    s.ci = 0;
    for (int q = 0; q < kMaxSrc; ++q) {
        s.src[q] = q < nsrc ? srcs[q] : nullptr;
        s.cs[q] = q < nsrc ? chans[q] : 0;
        if (q < nsrc && (!srcs[q] || chans[q] <= 0 || (align16 && (reinterpret_cast<uintptr_t>(srcs[q]) & 15))))
            return false;
        s.ci += s.cs[q];
    }
    return true;
}

inline bool aligned16(const Sources& s) {
    bool ok = true;
    for (int q = 0; q < s.nsrc; ++q) ok = ok && (reinterpret_cast<uintptr_t>(s.src[q]) & 15) == 0;
    return ok;
}

// ---- tiles: an output tile is 2x2 pixels; a workgroup takes a tby x tbx block of them
struct Tiles {
    int th, tw;    // tiles per image column / row
    int tbx, tby;  // tile-block shape
    int bx, by;    // tile blocks per image row / column
};

// tile block of ttiles tiles: the widest of ttiles x 1, ttiles/2 x 2, .. down to min_tbx wide with the
// fewest padded tiles (the fp32 kernels stop at 8 wide, the bf16x3 ones at ttiles / 8)
TSPLAT_WL_HD void fill_tiles(Tiles& g, int h, int w, int ttiles, int min_tbx) {
    g.th = (h + 1) / 2;
    g.tw = (w + 1) / 2;
    long best = -1;
    g.tbx = ttiles;
    for (int tbx = ttiles; tbx >= min_tbx; tbx /= 2) {
        const int tby = ttiles / tbx;
        const long padded = (long)((g.tw + tbx - 1) / tbx) * tbx * ((g.th + tby - 1) / tby) * tby;
        if (best < 0 || padded < best) {
            best = padded;
            g.tbx = tbx;
        }
    }
    g.tby = ttiles / g.tbx;
    g.bx = (g.tw + g.tbx - 1) / g.tbx;
    g.by = (g.th + g.tby - 1) / g.tby;
}

// Staged region of a tile block (bf16x3 kernels, map width a multiple of 4): 2 tby + 2 rows of
// tbx / 2 + 2 float4 per channel, which the kernels hold in at most 72 (32-tile blocks) / 136 (64-tile
// blocks) float4. Every block shape fill_tiles can choose fits, so no launch has to check.
constexpr bool region_fits(int tbx, int tby, int ttiles) {
    return (2 * tby + 2) * (tbx / 2 + 2) <= (ttiles == 32 ? 72 : 136);
}
static_assert(region_fits(32, 1, 32) && region_fits(16, 2, 32) && region_fits(8, 4, 32) && region_fits(4, 8, 32),
              "32-tile regions");
static_assert(region_fits(64, 1, 64) && region_fits(32, 2, 64) && region_fits(16, 4, 64) && region_fits(8, 8, 64),
              "64-tile regions");

// ---- packed U, exact fp32 (floats): [16 xi][cobs][ci_pad / 16 groups][64 lanes][8 slots], the A operand
// of v_mfma_f32_32x32x2_f32: lane l (co = 32 b + (l & 31), k half h = l >> 5) of group gr holds slot
// 4 q + k <- ci = 16 gr + 8 q + 4 h + k, so an 8-channel chunk q is one float4 per lane, a 16-channel
// chunk two
TSPLAT_WL_HD size_t u_index(int xi, int co, int ci, int cobs, int ci_pad) {
    const int rem = ci % 16, q = rem >> 3, h = (rem >> 2) & 1, k = rem & 3;
    const size_t plane = (size_t)cobs * ci_pad * 32;  // floats per xi
    return xi * plane + ((((size_t)(co / 32) * (ci_pad / 16) + ci / 16) * 64 + 32 * h + co % 32) * 8) + 4 * q + k;
}
TSPLAT_WL_HD size_t u_floats(int co, int ci) { return (size_t)16 * cobs(co) * ci_pad(ci) * 32; }

// ---- packed U, split bf16 (bf16 elements; the kernels read uint4 = 8 of them):
// [16 xi][cobs][nchunk][2 hi / lo][64 lanes][8], the A operand of v_mfma_f32_32x32x16_bf16: lane l
// (co = 32 b + (l & 31), h = l >> 5), element j <- ci = 16 chunk + 8 h + j
TSPLAT_WL_HD size_t u3_index(int xi, int co, int ci, int hl, int cobs, int nchunk) {
    const size_t frag = ((((size_t)xi * cobs + co / 32) * nchunk + ci / 16) * 2 + hl) * 64;  // its lane 0, in uint4
    return (frag + 32 * ((ci >> 3) & 1) + co % 32) * 8 + (ci & 7);
}
TSPLAT_WL_HD size_t u3_bytes(int co, int ci) { return (size_t)16 * cobs(co) * ci_pad(ci) * 32 * 2 * 2; }

}  // namespace wino_layout
}  // namespace tsplat
