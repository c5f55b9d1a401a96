// Host check of transplat_amd/csrc/corr_cell.h, built and run by tests/test_kernels_host.py. On every
// map from 1 x 1 to 9 x 9 plus 7 x 5, 12 x 20 and 64 x 64, at every pair of positions out of, per axis,
// the integers -2 .. size + 1, each integer's two nextafterf neighbours, the half-integers, +-1e4,
// +-inf and NaN: the cell equals a literal transcription of mmcv's ms_deform_attn_im2col_bilinear
// (written out below, not calling the header) in the "taken" decision, the corner, the inside mask and
// the four weights bit for bit; a sample that is not taken has the corner (-1, -1) and an empty mask;
// the weights of a taken sample sum to 1 within 2 ulp.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "corr_cell.h"

using tsplat::corr::Cell;

static int fails = 0;
#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        if (!(cond) && fails++ < 10) printf("line %d: %s (H %d W %d h %a w %a)\n", __LINE__, #cond, H, W, h, w); \
    } while (0)

// mmcv/ops/csrc/common/cuda/ms_deform_attn_cuda_kernel.cuh, scalar_t = float: the caller's window test,
// then the function's corner and weight expressions, in its names
struct Mmcv {
    bool taken;
    int h_low, w_low;
    bool in1, in2, in3, in4;
    float w1, w2, w3, w4;
};

static Mmcv mmcv_bilinear(int height, int width, float h, float w) {
    Mmcv m = {};
    m.taken = h > -1 && w > -1 && h < height && w < width;
    if (!m.taken) return m;
    const int h_low = floorf(h);
    const int w_low = floorf(w);
    const int h_high = h_low + 1;
    const int w_high = w_low + 1;
    const float lh = h - h_low;
    const float lw = w - w_low;
    const float hh = 1 - lh, hw = 1 - lw;
    m.h_low = h_low;
    m.w_low = w_low;
    m.in1 = h_low >= 0 && w_low >= 0;
    m.in2 = h_low >= 0 && w_high <= width - 1;
    m.in3 = h_high <= height - 1 && w_low >= 0;
    m.in4 = h_high <= height - 1 && w_high <= width - 1;
    m.w1 = hh * hw, m.w2 = hh * lw, m.w3 = lh * hw, m.w4 = lh * lw;
    return m;
}

static std::vector<float> positions(int size) {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> p = {1e4f, -1e4f, inf, -inf, std::numeric_limits<float>::quiet_NaN()};
    for (int i = -2; i <= size + 1; ++i) {
        const float f = (float)i;
        p.push_back(f);
        p.push_back(nextafterf(f, -inf));
        p.push_back(nextafterf(f, inf));
        p.push_back(f - 0.5f);
    }
    p.push_back((float)size + 1.5f);
    return p;
}

static void check_map(int H, int W) {
    const std::vector<float> ys = positions(H), xs = positions(W);
    for (float h : ys)
        for (float w : xs) {
            const Mmcv m = mmcv_bilinear(H, W, h, w);
            Cell c;
            const bool taken = tsplat::corr::cell_at(w, h, H, W, c);
            CHECK(taken == m.taken);
            if (!m.taken) {
                CHECK(c.y0 == -1 && c.x0 == -1 && c.in == 0u);
                continue;
            }
            CHECK(c.y0 == m.h_low && c.x0 == m.w_low);
            CHECK(c.in == ((unsigned)m.in1 | (unsigned)m.in2 << 1 | (unsigned)m.in3 << 2 | (unsigned)m.in4 << 3));
            float cw[4];
            tsplat::corr::cell_weights(c.ly, c.lx, cw);
            const float want[4] = {m.w1, m.w2, m.w3, m.w4};
            CHECK(memcmp(cw, want, sizeof(cw)) == 0);
            const float sum = cw[0] + cw[1] + cw[2] + cw[3];
            CHECK(fabsf(sum - 1.0f) <= 2 * std::numeric_limits<float>::epsilon());
        }
}

int main() {
    for (int H = 1; H <= 9; ++H)
        for (int W = 1; W <= 9; ++W) check_map(H, W);
    check_map(7, 5);
    check_map(12, 20);
    check_map(64, 64);
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}
