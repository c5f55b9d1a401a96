// Host check of transplat_amd/csrc/wino_layout.h, built and run by tests/test_kernels_host.py. Over
// every map of 1..40 x 1..140 plus the production sizes, for 32- and 64-tile blocks: fill_tiles agrees
// with a literal transcription of the two launchers' former loops, the block has ttiles tiles, its
// blocks span the map's tiles without an empty row or column of blocks, and its staged region fits.
// The packed-U index of each precision, through which the weight kernels write, is injective and fills
// the packed buffer exactly; fill_sources rejects what the three launchers' loops rejected.
#include <stdio.h>

#include <vector>

#include "wino_layout.h"

using namespace tsplat::wino_layout;

static int fails = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond) && fails++ < 10) printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

// the tile-block search as the launchers spelled it out before wino_layout.h (tbx down to min_tbx:
// 8 in winoconv.hip's wino_launch, ttiles / 8 in winoconv3.hip's geometry lambda)
static void former_search(int h, int w, int ttiles, int min_tbx, int& out_tbx, int& out_tby) {
    const int th = (h + 1) / 2, tw = (w + 1) / 2;
    int best_tbx = ttiles;
    long best = -1;
    for (int tbx = ttiles; tbx >= min_tbx; tbx /= 2) {
        const int tby = ttiles / tbx;
        const long padded = (long)((tw + tbx - 1) / tbx) * tbx * ((th + tby - 1) / tby) * tby;
        if (best < 0 || padded < best) {
            best = padded;
            best_tbx = tbx;
        }
    }
    out_tbx = best_tbx;
    out_tby = ttiles / best_tbx;
}

static void check_map(int h, int w, int ttiles, int min_tbx) {
    Tiles g;
    fill_tiles(g, h, w, ttiles, min_tbx);
    int tbx, tby;
    former_search(h, w, ttiles, min_tbx, tbx, tby);
    CHECK(g.tbx == tbx && g.tby == tby);
    CHECK(g.tbx * g.tby == ttiles);
    CHECK(g.th == (h + 1) / 2 && g.tw == (w + 1) / 2);
    CHECK(g.bx * g.tbx >= g.tw && (g.bx - 1) * g.tbx < g.tw && g.by * g.tby >= g.th && (g.by - 1) * g.tby < g.th);
    CHECK(region_fits(g.tbx, g.tby, ttiles));
}

static void check_packing(int co, int ci) {
    const int cb = cobs(co), cp = ci_pad(ci), nchunk = cp / 16;
    CHECK(cp % 16 == 0 && cp >= ci && cp < ci + 16 && cb % 2 == 0 && cb * 32 >= co && cb * 32 < co + 64);
    {  // exact fp32: floats
        const size_t n = u_floats(co, ci);
        CHECK(n == (size_t)16 * cb * 32 * cp);
        std::vector<char> hit(n, 0);
        for (int xi = 0; xi < 16; ++xi)
            for (int o = 0; o < cb * 32; ++o)
                for (int c = 0; c < cp; ++c) {
                    const size_t i = u_index(xi, o, c, cb, cp);
                    CHECK(i < n);
                    if (i >= n) continue;
                    CHECK(!hit[i]);
                    hit[i] = 1;
                }
    }
    {  // split bf16: bf16 elements, 2 bytes each
        const size_t n = u3_bytes(co, ci) / 2;
        CHECK(n == (size_t)16 * cb * 32 * cp * 2);
        std::vector<char> hit(n, 0);
        for (int xi = 0; xi < 16; ++xi)
            for (int o = 0; o < cb * 32; ++o)
                for (int c = 0; c < cp; ++c)
                    for (int hl = 0; hl < 2; ++hl) {
                        const size_t i = u3_index(xi, o, c, hl, cb, nchunk);
                        CHECK(i < n);
                        if (i >= n) continue;
                        CHECK(!hit[i]);
                        hit[i] = 1;
                    }
    }
}

static void check_sources() {
    alignas(16) static float buf[64];
    const float* ok[kMaxSrc + 1] = {buf, buf + 4, buf + 8, buf + 12, buf + 16, buf + 20, buf + 24};
    const int32_t ch[kMaxSrc + 1] = {3, 1, 4, 1, 5, 9, 2};
    Sources s;
    for (int nsrc = 1; nsrc <= kMaxSrc; ++nsrc) {
        CHECK(fill_sources(s, ok, ch, nsrc) && fill_sources(s, ok, ch, nsrc, true));
        int ci = 0;
        for (int q = 0; q < kMaxSrc; ++q) {
            CHECK(s.src[q] == (q < nsrc ? ok[q] : nullptr) && s.cs[q] == (q < nsrc ? ch[q] : 0));
            ci += q < nsrc ? ch[q] : 0;
        }
        CHECK(s.nsrc == nsrc && s.ci == ci && aligned16(s));
    }
    CHECK(!fill_sources(s, ok, ch, 0) && !fill_sources(s, ok, ch, -1) && !fill_sources(s, ok, ch, kMaxSrc + 1));
    CHECK(!fill_sources(s, nullptr, ch, 1) && !fill_sources(s, ok, nullptr, 1));
    for (int bad = 0; bad < 3; ++bad) {
        const float* p[3] = {buf, buf + 4, buf + 8};
        int32_t c[3] = {2, 2, 2};
        p[bad] = nullptr;
        CHECK(!fill_sources(s, p, c, 3));
        p[bad] = buf;
        c[bad] = 0;
        CHECK(!fill_sources(s, p, c, 3));
        c[bad] = -1;
        CHECK(!fill_sources(s, p, c, 3));
        c[bad] = 2;
        p[bad] = buf + 1;  // 4-B aligned only: fine unless the kernel moves float4
        CHECK(fill_sources(s, p, c, 3) && !aligned16(s));
        CHECK(!fill_sources(s, p, c, 3, true));
        c[bad] = 0;
        if (bad) CHECK(fill_sources(s, p, c, bad, true));  // a bad entry past nsrc is not looked at
    }
}

int main() {
    const int prod[11][2] = {{32, 32}, {36, 36}, {64, 64}, {72, 72}, {128, 128}, {144, 144}, {160, 160}, {256, 256},
                             {16, 40}, {9, 70}, {17, 21}};
    for (int ttiles : {32, 64}) {
        for (int h = 1; h <= 40; ++h)
            for (int w = 1; w <= 140; ++w) {
                check_map(h, w, ttiles, ttiles / 8);        // the bf16x3 launcher's four shapes
                if (ttiles == 32) check_map(h, w, 32, 8);  // the fp32 launcher's three
            }
        for (const auto& m : prod) {
            check_map(m[0], m[1], ttiles, ttiles / 8);
            if (ttiles == 32) check_map(m[0], m[1], 32, 8);
        }
    }
    const int packs[5][2] = {{2, 64}, {32, 38}, {84, 168}, {168, 163}, {256, 128}};
    for (const auto& p : packs) check_packing(p[0], p[1]);
    check_sources();
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
