// Window geometry and split-key partials layout of the window attention, shared by its kernels
// (winattn.hip) and by the merge projection that reads the partials in its operand staging
// (linear.hip): every index into the map or into the workspace goes through these functions, on the
// host and on the device alike. Plain C++ apart from the function qualifiers, so a host compiler can
// build it too (tests/winattn_layout_check.cc walks every index).
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define TSPLAT_WA_HD __host__ __device__ __forceinline__
#else
#define TSPLAT_WA_HD inline
#endif

namespace tsplat {
namespace winattn {

constexpr int kC = 128;     // channels (d_model of the reference transformer)
constexpr int kTileQ = 128; // queries per block of the lane-contiguous layout (4 waves x 32)

// One launch's windows and key split (the leading fields of the kernels' Params, in its order)
struct Window {
    int H, W, splits, shift, m, L;  // L = window pixels; shift != 0: shifted (masked) layer
    int shift_h, shift_w;           // roll of the shifted layer: half a window per axis
    int ksplit, keys_per_split;     // key range [s * keys_per_split, (s+1) * keys_per_split)
    int wh, ww, ww_log2;            // window rows / columns; log2(ww), or -1 if not a power of 2
};

// the one place a Window is filled (height, width divisible by splits; ksplit divides L * key_views)
TSPLAT_WA_HD void fill_window(Window& g, int height, int width, int splits, int key_views, int with_shift,
                              int ksplit) {
    g.H = height;
    g.W = width;
    g.splits = splits;
    g.shift = with_shift ? 1 : 0;
    g.m = key_views;
    g.wh = height / splits;
    g.ww = width / splits;
    g.L = g.wh * g.ww;
    g.shift_h = with_shift ? g.wh / 2 : 0;
    g.shift_w = with_shift ? g.ww / 2 : 0;
    g.ksplit = ksplit;
    g.keys_per_split = g.L * key_views / ksplit;
    g.ww_log2 = (g.ww & (g.ww - 1)) == 0 ? __builtin_ctz(g.ww) : -1;
}

// t / ww and t % ww without a per-lane integer division when the window width is a power of 2
TSPLAT_WA_HD void win_split(const Window& p, int t, int& ty, int& tx) {
    ty = p.ww_log2 >= 0 ? (t >> p.ww_log2) : t / p.ww;
    tx = t - ty * p.ww;
}

// original pixel of in-window position t of window wi after the roll by -shift
TSPLAT_WA_HD int win_pixel(const Window& p, int wi, int t) {
    const int sy = wi / p.splits, sx = wi - sy * p.splits;
    int ty, tx;
    win_split(p, t, ty, tx);
    int y = sy * p.wh + ty + p.shift_h;
    int x = sx * p.ww + tx + p.shift_w;
    if (y >= p.H) y -= p.H;
    if (x >= p.W) x -= p.W;
    return y * p.W + x;
}

// the inverse of win_pixel: window and in-window position of original pixel pix
TSPLAT_WA_HD void win_locate(const Window& p, int pix, int& wi, int& t) {
    const int y = pix / p.W, x = pix - y * p.W;
    int Y = y - p.shift_h, X = x - p.shift_w;  // position on the rolled grid
    if (Y < 0) Y += p.H;
    if (X < 0) X += p.W;
    const int sy = Y / p.wh, sx = X / p.ww;
    wi = sy * p.splits + sx;
    t = (Y - sy * p.wh) * p.ww + (X - sx * p.ww);
}

// Swin region id of in-window position t of window wi (on the rolled grid)
TSPLAT_WA_HD int win_region(const Window& p, int wi, int t) {
    const int sy = wi / p.splits, sx = wi - sy * p.splits;
    int ty, tx;
    win_split(p, t, ty, tx);
    const int Y = sy * p.wh + ty, X = sx * p.ww + tx;
    const int by = Y < p.H - p.wh ? 0 : (Y < p.H - p.wh / 2 ? 1 : 2);
    const int bx = X < p.W - p.ww ? 0 : (X < p.W - p.ww / 2 ? 1 : 2);
    return by * 3 + bx;
}

// ---- split-key partials in the workspace: o [rows][128] | m [rows] | l [rows] (floats), where
// rows = batch * windows * ksplit * L; O unnormalised, m the running maximum (natural log), l the sum
struct Partials {
    float* o;
    float* m;
    float* l;
};

TSPLAT_WA_HD size_t partial_rows(const Window& p, int batch) {
    return (size_t)batch * p.splits * p.splits * p.ksplit * p.L;
}
TSPLAT_WA_HD size_t partials_bytes(const Window& p, int batch) {
    return p.ksplit > 1 ? partial_rows(p, batch) * (kC + 2) * sizeof(float) : 0;
}
TSPLAT_WA_HD Partials carve_partials(const Window& p, int batch, void* workspace) {
    const size_t n = partial_rows(p, batch);
    Partials part{static_cast<float*>(workspace), nullptr, nullptr};
    part.m = part.o + n * kC;
    part.l = part.m + n;
    return part;
}

// row of query t (in-window index) of window wi, batch b, key split ks: its index in m and l, and
// (the 64-query kernel, whose o is row-major) in o
TSPLAT_WA_HD size_t pidx(const Window& p, int b, int wi, int ks, int t) {
    return (((size_t)b * p.splits * p.splits + wi) * p.ksplit + ks) * p.L + t;
}

// The 128-query kernels store each wave's unnormalised O^T tile lane-contiguously: float4 number
// (dt * 4 + u) * 64 + lane of the wave's 16-KB slot holds O^T[d = 32 dt + 8u + 4h .. +3][query c]
// (lane = c + 32 h). The four wave slots of a query block are consecutive. Slot of (b, wi, ks, query
// block, wave) in o (floats):
TSPLAT_WA_HD size_t lane_tile_base(const Window& p, int b, int wi, int ks, int qblk, int wid) {
    const size_t nqb = (size_t)p.L / kTileQ;
    return ((((size_t)b * p.splits * p.splits + wi) * p.ksplit + ks) * nqb + qblk) * kTileQ * kC + (size_t)wid * 32 * kC;
}
// floats from a slot to the same (query block, wave)'s slot of the next key split
TSPLAT_WA_HD size_t lane_tile_split_stride(const Window& p) { return (size_t)(p.L / kTileQ) * kTileQ * kC; }
constexpr int kSlotFloat4 = 32 * kC / 4;  // float4s of one wave slot
// float4 within a wave slot of d tile dt, 8-channel run u, lane; and back
TSPLAT_WA_HD int slot_float4(int dt, int u, int lane) { return (dt * 4 + u) * 64 + lane; }
TSPLAT_WA_HD void slot_float4_split(int f4, int& dt, int& u, int& lane) {
    dt = f4 >> 8;
    u = (f4 >> 6) & 3;
    lane = f4 & 63;
}
// in-window query t <-> (query block, wave, lane column c) of the lane-contiguous layout
TSPLAT_WA_HD int tile_query(int qblk, int wid, int c) { return qblk * kTileQ + wid * 32 + c; }
TSPLAT_WA_HD void tile_query_split(int t, int& qblk, int& wid, int& c) {
    qblk = t >> 7;
    wid = (t >> 5) & 3;
    c = t & 31;
}
// float4 within query column c's wave slot that holds channels d .. d + 3 (d % 4 == 0) of O^T
TSPLAT_WA_HD int slot_float4_of_channel(int d, int c) {
    return slot_float4(d >> 5, (d >> 3) & 3, c + 32 * ((d >> 2) & 1));
}

}  // namespace winattn
}  // namespace tsplat
