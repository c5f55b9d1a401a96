// Host check of transplat_amd/csrc/winattn_layout.h, built and run by tests/test_kernels_host.py:
// for each map, with and without shift, win_locate undoes win_pixel for every (window, t), every
// pixel belongs to exactly one of them, and the partials indices (pidx for m / l and the 64-query
// kernel's o rows; lane_tile_base + slot_float4 for the 128-query kernels' o) tile the carved
// workspace [0, partials_bytes / 4) floats exactly once.
#include <stdio.h>

#include <vector>

#include "winattn_layout.h"

using namespace tsplat::winattn;

static int fails = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond) && fails++ < 10) printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

static void check_map(int H, int W, int splits, int shift, int ksplit, int batch) {
    Window g;
    fill_window(g, H, W, splits, 1, shift, ksplit);
    CHECK(g.L == (H / splits) * (W / splits));
    CHECK((g.ww_log2 >= 0) == ((g.ww & (g.ww - 1)) == 0));
    CHECK(g.ww_log2 < 0 || (1 << g.ww_log2) == g.ww);
    const int windows = splits * splits;

    // geometry round trip
    std::vector<int> seen(H * W, 0);
    for (int wi = 0; wi < windows; ++wi)
        for (int t = 0; t < g.L; ++t) {
            const int pix = win_pixel(g, wi, t);
            CHECK(pix >= 0 && pix < H * W);
            if (pix < 0 || pix >= H * W) continue;
            ++seen[pix];
            int wi2, t2;
            win_locate(g, pix, wi2, t2);
            CHECK(wi2 == wi && t2 == t);
            const int r = win_region(g, wi, t);
            CHECK(r >= 0 && r < 9);
        }
    for (int pix = 0; pix < H * W; ++pix) CHECK(seen[pix] == 1);

    // partials: the carve and the indices into it
    const size_t rows = partial_rows(g, batch), floats = rows * (kC + 2);
    CHECK(partials_bytes(g, batch) == (ksplit > 1 ? floats * sizeof(float) : 0));
    std::vector<float> ws(floats);
    const Partials part = carve_partials(g, batch, ws.data());
    CHECK(part.o == ws.data() && part.m == part.o + rows * kC && part.l == part.m + rows);
    CHECK(part.l + rows == ws.data() + floats);
    std::vector<int> hit(floats, 0);
    for (int b = 0; b < batch; ++b)
        for (int wi = 0; wi < windows; ++wi)
            for (int ks = 0; ks < ksplit; ++ks)
                for (int t = 0; t < g.L; ++t) {
                    const size_t row = pidx(g, b, wi, ks, t);
                    CHECK(row < rows);
                    if (row >= rows) continue;
                    ++hit[(part.m - ws.data()) + row];
                    ++hit[(part.l - ws.data()) + row];
                    if (g.L % kTileQ)  // row-major o of the 64-query kernel
                        for (int d = 0; d < kC; ++d) ++hit[row * kC + d];
                }
    if (g.L % kTileQ == 0) {
        for (int b = 0; b < batch; ++b)
            for (int wi = 0; wi < windows; ++wi)
                for (int ks = 0; ks < ksplit; ++ks)
                    for (int qblk = 0; qblk < g.L / kTileQ; ++qblk)
                        for (int wid = 0; wid < 4; ++wid) {
                            const size_t base = lane_tile_base(g, b, wi, ks, qblk, wid);
                            CHECK(base % 4 == 0 && base + 4 * kSlotFloat4 <= rows * kC);
                            if (base + 4 * kSlotFloat4 > rows * kC) continue;
                            if (ks + 1 < ksplit)
                                CHECK(lane_tile_base(g, b, wi, ks + 1, qblk, wid) == base + lane_tile_split_stride(g));
                            if (wid < 3) CHECK(lane_tile_base(g, b, wi, ks, qblk, wid + 1) == base + 4 * kSlotFloat4);
                            for (int dt = 0; dt < 4; ++dt)
                                for (int u = 0; u < 4; ++u)
                                    for (int lane = 0; lane < 64; ++lane) {
                                        const int f4 = slot_float4(dt, u, lane);
                                        CHECK(f4 >= 0 && f4 < kSlotFloat4);
                                        int dt2, u2, lane2;
                                        slot_float4_split(f4, dt2, u2, lane2);
                                        CHECK(dt2 == dt && u2 == u && lane2 == lane);
                                        for (int j = 0; j < 4; ++j) ++hit[base + 4 * (size_t)f4 + j];
                                        // channels of this float4: d = 32 dt + 8 u + 4 (lane >> 5) .. + 3
                                        CHECK(slot_float4_of_channel(32 * dt + 8 * u + 4 * (lane >> 5), lane & 31) == f4);
                                    }
                            int qblk2, wid2, c2;
                            tile_query_split(tile_query(qblk, wid, 31), qblk2, wid2, c2);
                            CHECK(tile_query(qblk, wid, 31) < g.L && qblk2 == qblk && wid2 == wid && c2 == 31);
                        }
    }
    for (size_t i = 0; i < floats; ++i) CHECK(hit[i] == 1);
}

int main() {
    const int maps[3][2] = {{16, 16}, {32, 96}, {96, 128}};
    for (const auto& m : maps)
        for (int shift = 0; shift < 2; ++shift)
            for (int ksplit : {1, 4}) check_map(m[0], m[1], 2, shift, ksplit, 2);
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
