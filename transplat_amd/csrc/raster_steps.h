// The steps the rasterizer's forward kernels and their backward share, each defined once: the depth value
// and its derivative, the SH basis enumeration, the projection and EWA covariance of one (view, Gaussian),
// and for the render kernels the tile prologue (tile index, list range, the three sort paths), the wave's
// pixel block, the compacted-record layout, the chunk walk (one-ahead fetch, cull, ballot compaction,
// fences) and the blend decision of one entry at one pixel. The backward recomputes the forward through
// these very functions, so its T, alpha, tile order and every branch are the forward's by construction.
//
// Included by raster.hip only, inside namespace tsplat::raster, after its `#pragma clang fp contract(off)`
// (which therefore covers every expression here: the view-space depth must stay the reference's bit for
// bit), after Params, Workspace and the SH constants, and after raster_sort.h.
#pragma once

// The value the depth output blends for one (view, Gaussian), and its derivative in vz. The reference
// renders depth as a colour (render_depth_cuda, cuda_splatting.py:375-417): fake colour f of the UNSCALED
// camera-space depth z (:388-400) as the degree-0 SH coefficient, so d = max(C0 f + 0.5, 0). z = vz / s
// undoes the scale-invariant rendering (vz is the depth of the scaled scene). "log" keeps the reference's
// minimum(near).maximum(far) order, which gives log(far) for every Gaussian. IEEE division and logf.
// dz = C0 f'(z) where the clamp of d is open, 0 where it is active (C0 f + 0.5 <= 0); "log" follows z only
// where far < z < near strictly. The forward uses d alone.
struct DepthValue {
    float d, dz;
};
__device__ __forceinline__ DepthValue depth_value(int mode, float vz, float s, float near, float far) {
    const float z = vz / s;
    float f = z, df = 1.0f;
    if (mode == 1) {
        f = 1.0f / z;
        df = -1.0f / (z * z);
    } else if (mode == 2) {
        const float eps = 1e-10f;  // depth_to_relative_disparity (matching/conversions.py:18-28)
        const float disp_near = 1.0f / (near + eps), disp_far = 1.0f / (far + eps);
        const float den = disp_near - disp_far + eps;
        f = 1.0f - (1.0f / (z + eps) - disp_far) / den;
        df = 1.0f / ((z + eps) * (z + eps)) / den;
    } else if (mode == 3) {
        f = logf(fmaxf(fminf(z, near), far));
        df = (z > far && z < near) ? 1.0f / z : 0.0f;
    }
    const float c = kSH_C0 * f + 0.5f;
    return {fmaxf(c, 0.0f), c > 0.0f ? kSH_C0 * df : 0.0f};
}

// The real SH basis up to `deg` at the unit direction (x, y, z), in coefficient order:
// visit(k, B_k, dB_k/dx, dB_k/dy, dB_k/dz), k a std::integral_constant. A visitor that ignores the
// gradients costs nothing for them. The values are the expressions of the reference's computeColorFromSH
// with the sign folded into the basis value (-(C1 y) s = (-C1 y) s exactly), so a visitor that adds
// B_k s[k] in visiting order reproduces its sums bit for bit.
template <class Visit>
__device__ __forceinline__ void sh_basis(int deg, float x, float y, float z, Visit&& visit) {
#define TSPLAT_SH(k, ...) visit(std::integral_constant<int, k>{}, __VA_ARGS__)
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    TSPLAT_SH(0, kSH_C0, 0.f, 0.f, 0.f);
    if (deg > 0) {
        TSPLAT_SH(1, -kSH_C1 * y, 0.f, -kSH_C1, 0.f);
        TSPLAT_SH(2, kSH_C1 * z, 0.f, 0.f, kSH_C1);
        TSPLAT_SH(3, -kSH_C1 * x, -kSH_C1, 0.f, 0.f);
    }
    if (deg > 1) {
        TSPLAT_SH(4, kSH_C2[0] * xy, kSH_C2[0] * y, kSH_C2[0] * x, 0.f);
        TSPLAT_SH(5, kSH_C2[1] * yz, 0.f, kSH_C2[1] * z, kSH_C2[1] * y);
        TSPLAT_SH(6, kSH_C2[2] * (2.0f * zz - xx - yy), kSH_C2[2] * -2.0f * x, kSH_C2[2] * -2.0f * y,
                  kSH_C2[2] * 4.0f * z);
        TSPLAT_SH(7, kSH_C2[3] * xz, kSH_C2[3] * z, 0.f, kSH_C2[3] * x);
        TSPLAT_SH(8, kSH_C2[4] * (xx - yy), kSH_C2[4] * 2.0f * x, kSH_C2[4] * -2.0f * y, 0.f);
    }
    if (deg > 2) {
        TSPLAT_SH(9, kSH_C3[0] * y * (3.0f * xx - yy), kSH_C3[0] * 6.0f * xy, kSH_C3[0] * (3.0f * xx - 3.0f * yy),
                  0.f);
        TSPLAT_SH(10, kSH_C3[1] * xy * z, kSH_C3[1] * yz, kSH_C3[1] * xz, kSH_C3[1] * xy);
        TSPLAT_SH(11, kSH_C3[2] * y * (4.0f * zz - xx - yy), kSH_C3[2] * -2.0f * xy,
                  kSH_C3[2] * (4.0f * zz - xx - 3.0f * yy), kSH_C3[2] * 8.0f * yz);
        TSPLAT_SH(12, kSH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy), kSH_C3[3] * -6.0f * xz,
                  kSH_C3[3] * -6.0f * yz, kSH_C3[3] * (6.0f * zz - 3.0f * xx - 3.0f * yy));
        TSPLAT_SH(13, kSH_C3[4] * x * (4.0f * zz - xx - yy), kSH_C3[4] * (4.0f * zz - 3.0f * xx - yy),
                  kSH_C3[4] * -2.0f * xy, kSH_C3[4] * 8.0f * xz);
        TSPLAT_SH(14, kSH_C3[5] * z * (xx - yy), kSH_C3[5] * 2.0f * xz, kSH_C3[5] * -2.0f * yz,
                  kSH_C3[5] * (xx - yy));
        TSPLAT_SH(15, kSH_C3[6] * x * (xx - 3.0f * yy), kSH_C3[6] * (3.0f * xx - 3.0f * yy),
                  kSH_C3[6] * -6.0f * xy, 0.f);
    }
    if (deg > 3) {
        const float s7 = 7.0f * zz - 1.0f, t7 = 7.0f * zz - 3.0f;
        TSPLAT_SH(16, kSH_C4[0] * xy * (xx - yy), kSH_C4[0] * y * (3.0f * xx - yy),
                  kSH_C4[0] * x * (xx - 3.0f * yy), 0.f);
        TSPLAT_SH(17, kSH_C4[1] * yz * (3.0f * xx - yy), kSH_C4[1] * 6.0f * xy * z,
                  kSH_C4[1] * z * (3.0f * xx - 3.0f * yy), kSH_C4[1] * y * (3.0f * xx - yy));
        TSPLAT_SH(18, kSH_C4[2] * xy * s7, kSH_C4[2] * y * s7, kSH_C4[2] * x * s7, kSH_C4[2] * 14.0f * xy * z);
        TSPLAT_SH(19, kSH_C4[3] * yz * t7, 0.f, kSH_C4[3] * z * t7, kSH_C4[3] * y * (21.0f * zz - 3.0f));
        TSPLAT_SH(20, kSH_C4[4] * (zz * (35.0f * zz - 30.0f) + 3.0f), 0.f, 0.f,
                  kSH_C4[4] * z * (140.0f * zz - 60.0f));
        TSPLAT_SH(21, kSH_C4[5] * xz * t7, kSH_C4[5] * z * t7, 0.f, kSH_C4[5] * x * (21.0f * zz - 3.0f));
        TSPLAT_SH(22, kSH_C4[6] * (xx - yy) * s7, kSH_C4[6] * 2.0f * x * s7, kSH_C4[6] * -2.0f * y * s7,
                  kSH_C4[6] * 14.0f * z * (xx - yy));
        TSPLAT_SH(23, kSH_C4[7] * xz * (xx - 3.0f * yy), kSH_C4[7] * z * (3.0f * xx - 3.0f * yy),
                  kSH_C4[7] * -6.0f * xy * z, kSH_C4[7] * x * (xx - 3.0f * yy));
        TSPLAT_SH(24, kSH_C4[8] * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy)),
                  kSH_C4[8] * x * (4.0f * xx - 12.0f * yy), kSH_C4[8] * y * (4.0f * yy - 12.0f * xx), 0.f);
    }
#undef TSPLAT_SH
}

// The unit view direction n = d / |d| the SH basis is evaluated at, d = scaled mean - camera position.
struct ShDir {
    float len, x, y, z;
};
__device__ __forceinline__ ShDir sh_dir(float dx, float dy, float dz) {
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    return {len, dx / len, dy / len, dz / len};
}

__device__ __forceinline__ void sh_to_rgb(const float* __restrict__ sh, int M, int deg, const ShDir& n,
                                          float out[3]) {
    // sh is colour-major [3][M]; coefficient k of channel c is sh[c*M + k]
    float r[3];
    sh_basis(deg, n.x, n.y, n.z, [&](auto k, float B, float, float, float) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (decltype(k)::value == 0)
                r[c] = B * sh[c * M];
            else
                r[c] = r[c] + B * sh[c * M + decltype(k)::value];
        }
    });
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = fmaxf(r[c] + 0.5f, 0.0f);
}

// The scaled mean and its view-space point. Scale-invariant rendering: means * s (cov * s^2 in project();
// cuda_splatting.py:73-80). vz is the sort key and the in_frustum test (auxiliary.h in_frustum: the
// forward renders vz > 0.2 only): the reference's transformPoint4x3 expression.
struct ViewPoint {
    float mx, my, mz, vx, vy, vz;
};
__device__ __forceinline__ ViewPoint view_point(float m0, float m1, float m2, float s,
                                                const float* __restrict__ vm) {
    ViewPoint q;
    q.mx = m0 * s, q.my = m1 * s, q.mz = m2 * s;
    q.vx = vm[0] * q.mx + vm[4] * q.my + vm[8] * q.mz + vm[12];
    q.vy = vm[1] * q.mx + vm[5] * q.my + vm[9] * q.mz + vm[13];
    q.vz = vm[2] * q.mx + vm[6] * q.my + vm[10] * q.mz + vm[14];
    return q;
}

// Projection and EWA splatting (computeCov2D) of one (view, Gaussian): the homogeneous point (hx, hy) with
// pw = 1 / (hw + 1e-7); the clamped ray (rx, ry) = clamp(v / vz, +-1.3 tan fov) with in_x / in_y set where
// the clamp is open; N = J R_w2c (R[r][c] = vm[c*4 + r]); U = N C with C = s^2 K (the upper triangle of K
// read); the 2-D covariance (a, b, c) = N C N^T + 0.3 I and its determinant. The forward uses the values
// and keeps its early-outs around the call; the backward chains its gradients through the same values.
struct Projection {
    float hx, hy, pw, fx, fy, rx, ry;
    bool in_x, in_y;
    float n00, n01, n02, n10, n11, n12, u00, u01, u02, u10, u11, u12, a, b, c, det;
};
__device__ __forceinline__ Projection project(const ViewPoint& q, float k00, float k01, float k02, float k11,
                                              float k12, float k22, float s2, const float* __restrict__ vm,
                                              const float* __restrict__ pm, float tfx, float tfy, int W, int H) {
    Projection r;
    const float mx = q.mx, my = q.my, mz = q.mz;
    r.hx = pm[0] * mx + pm[4] * my + pm[8] * mz + pm[12];
    r.hy = pm[1] * mx + pm[5] * my + pm[9] * mz + pm[13];
    const float hw = pm[3] * mx + pm[7] * my + pm[11] * mz + pm[15];
    r.pw = 1.0f / (hw + 0.0000001f);
    const float c00 = k00 * s2, c01 = k01 * s2, c02 = k02 * s2;
    const float c11 = k11 * s2, c12 = k12 * s2, c22 = k22 * s2;
    r.fx = (float)W / (2.0f * tfx), r.fy = (float)H / (2.0f * tfy);
    const float limx = 1.3f * tfx, limy = 1.3f * tfy;
    const float tz = q.vz;
    const float rxu = q.vx / tz, ryu = q.vy / tz;
    r.rx = fminf(limx, fmaxf(-limx, rxu)), r.ry = fminf(limy, fmaxf(-limy, ryu));
    r.in_x = rxu >= -limx && rxu <= limx, r.in_y = ryu >= -limy && ryu <= limy;
    const float tx = r.rx * tz, ty = r.ry * tz;
    const float j00 = r.fx / tz, j02 = -(r.fx * tx) / (tz * tz);
    const float j11 = r.fy / tz, j12 = -(r.fy * ty) / (tz * tz);
    r.n00 = j00 * vm[0] + j02 * vm[2];
    r.n01 = j00 * vm[4] + j02 * vm[6];
    r.n02 = j00 * vm[8] + j02 * vm[10];
    r.n10 = j11 * vm[1] + j12 * vm[2];
    r.n11 = j11 * vm[5] + j12 * vm[6];
    r.n12 = j11 * vm[9] + j12 * vm[10];
    r.u00 = r.n00 * c00 + r.n01 * c01 + r.n02 * c02;
    r.u01 = r.n00 * c01 + r.n01 * c11 + r.n02 * c12;
    r.u02 = r.n00 * c02 + r.n01 * c12 + r.n02 * c22;
    r.u10 = r.n10 * c00 + r.n11 * c01 + r.n12 * c02;
    r.u11 = r.n10 * c01 + r.n11 * c11 + r.n12 * c12;
    r.u12 = r.n10 * c02 + r.n11 * c12 + r.n12 * c22;
    r.a = r.u00 * r.n00 + r.u01 * r.n01 + r.u02 * r.n02 + 0.3f;
    r.b = r.u00 * r.n10 + r.u01 * r.n11 + r.u02 * r.n12;
    r.c = r.u10 * r.n10 + r.u11 * r.n11 + r.u12 * r.n12 + 0.3f;
    r.det = r.a * r.c - r.b * r.b;
    return r;
}

// The conic, the inverse of the 2-D covariance (det != 0).
struct Conic {
    float a, b, c;
};
__device__ __forceinline__ Conic conic_of(const Projection& r) {
    const float det_inv = 1.0f / r.det;
    return {r.c * det_inv, -r.b * det_inv, r.a * det_inv};
}

// Exact culling of one Gaussian against a pixel block: does the alpha >= 1/255 ellipse
// {d : a dx^2 + 2 b dx dy + c dy^2 <= q}, q = 2 ln(255 o), meet the rectangle of pixel centres
// [x0, x1] x [y0, y1]? The minimum of the (convex) quadratic over the rectangle is 0 when the
// centre is inside, else it lies on an edge (1-D minimisation, clamped). Conservative margins
// (relative 1e-3 on q plus 1e-3 absolute) keep every contributing Gaussian (the blend's float
// arithmetic differs from this by a few ulps), so images are unchanged; culls the corners the
// axis-aligned box test keeps for rotated / elongated splats.
__device__ __forceinline__ bool ellipse_meets_block(float mx, float my, float4 co, float4 cull, float x0, float x1,
                                                    float y0, float y1) {
    // co = log2(e) (-a/2, -b, -c/2) and o as stored; cull = (2 log2(255 o) * 1.001 + 1.5e-3, -b/a,
    // -b/c): Q and q both carry the log2(e) factor,
    // precomputed per (view, Gaussian) by the preprocess kernel (approximate reciprocals: a clamped
    // minimiser off by an ulp raises Q by O(ulp^2), far inside the margins above)
    const float a = -2.0f * co.x, b = -co.y, c = -2.0f * co.z;
    const float q = cull.x, kba = cull.y, kbc = cull.z;
    const float X0 = x0 - mx, X1 = x1 - mx, Y0 = y0 - my, Y1 = y1 - my;
    if (X0 <= 0.f && X1 >= 0.f && Y0 <= 0.f && Y1 >= 0.f) return true;
    if (!(a > 0.f && c > 0.f)) return true;  // degenerate: keep (the box test decided)
    // Q(dx, dy) = dx (a dx + 2 b dy) + c dy^2; along x = X the minimiser is dy = X (-b / c)
    const float b2 = 2.0f * b;
    auto Qf = [&](float dx, float dy) { return fmaf(dx, fmaf(b2, dy, a * dx), c * dy * dy); };
    const float qx0 = Qf(X0, fminf(fmaxf(X0 * kbc, Y0), Y1));
    const float qx1 = Qf(X1, fminf(fmaxf(X1 * kbc, Y0), Y1));
    const float qy0 = Qf(fminf(fmaxf(Y0 * kba, X0), X1), Y0);
    const float qy1 = Qf(fminf(fmaxf(Y1 * kba, X0), X1), Y1);
    return fminf(fminf(qx0, qx1), fminf(qy0, qy1)) <= q;
}

// --- the render kernels' shared steps -----------------------------------------------------------

// LDS of a tile's sort, declared by the kernel and handed to tile_prologue().
struct SortLds {
    uint64_t* keys;  // [kSortCap]; after the sort, the sorted ids as a uint32 list at its start
    uint32_t* cnt;   // [kBuckets]
    uint32_t* red;   // [4]
};

// A workgroup's tile and its sorted list: n entries; the ids in LDS (in_lds) or the keys in gkeys.
struct TileList {
    int tile, n;
    uint64_t* gkeys;
    bool in_lds;
};

// Tile of workgroup (blockIdx.x, view v), its [start, end) range clamped to the capacity, and the sort.
// False: a forward timing diagnostic (p.diag 2, 3) ends the kernel here; the backward's host code sets
// p.diag = 0, here and for chunk_walk().
// After it no workgroup barrier follows: each wave walks the sorted list on its own.
__device__ __forceinline__ bool tile_prologue(const Params& p, const Workspace& ws, int v, const SortLds& s,
                                              TileList& tl) {
    const int diag = p.diag;
    // Workgroup (tile, v) and (tile, v') share an XCD and a CU slot in dispatch order, and a
    // tile's cost is similar across the target views of a scene (central tiles are the heavy
    // ones), so without the per-view rotation every CU would get the same tile three times.
    // Rotating by whole tile rows keeps each XCD's band of rows contiguous (L2 reuse of records).
    int tile = xcd_remap(blockIdx.x, gridDim.x) + v * p.view_rot;
    tile %= p.T;
    const int t_idx = v * p.T + tile;
    uint32_t start = ws.offsets[t_idx];
    uint32_t end = ws.offsets[t_idx + 1];
    if (end > (uint32_t)p.capacity) end = (uint32_t)p.capacity;
    if (start > end) start = end;
    const int n = (int)(end - start);
    uint64_t* gkeys = ws.keys + start;
    tl = {tile, n, gkeys, n <= kSortCap};
    if (tl.in_lds) {
        // lists longer than one register pass: counting sort on the depth bits (falls back to the
        // bitonic network when the tile's depths cluster)
        const bool try_count = p.count_sort && n > kTileThreads && diag != 3;
        const bool counted = try_count && counting_sort(gkeys, n, s.keys, s.cnt, s.red);
        if (!counted) {
            for (int i = threadIdx.x; i < n; i += kTileThreads) s.keys[i] = gkeys[i];
            __syncthreads();
            if (diag == 3) return false;  // key load only
            bitonic_sort_regs(s.keys, n);
        }
        if (diag == 2) return false;  // key load + sort
    } else {
        // rare: very long tile list, sorted in place in global memory (by the forward; the backward's
        // pass over the sorted keys leaves them as they are)
        bitonic_sort(gkeys, n);
    }
    return true;
}

// A wave's 8x8 pixel block of the tile and this lane's pixel in it.
struct WavePixel {
    int wid, lane, pxi, pyi;
    float wx0, wx1, wy0, wy1, pfx, pfy;
    bool inside;
};
__device__ __forceinline__ WavePixel wave_pixel(const Params& p, int tile) {
    WavePixel w;
    const int tx = tile % p.tiles_x, ty = tile / p.tiles_x;
    w.wid = threadIdx.x / kWave, w.lane = threadIdx.x % kWave;
    const int lx = (w.wid & 1) * 8 + (w.lane & 7), ly = (w.wid >> 1) * 8 + (w.lane >> 3);
    w.pxi = tx * kTile + lx, w.pyi = ty * kTile + ly;
    w.wx0 = (float)(tx * kTile + (w.wid & 1) * 8), w.wx1 = w.wx0 + 7.0f;
    w.wy0 = (float)(ty * kTile + (w.wid >> 1) * 8), w.wy1 = w.wy0 + 7.0f;
    w.inside = w.pxi < p.W && w.pyi < p.H;
    w.pfx = (float)w.pxi, w.pfy = (float)w.pyi;
    return w;
}

// Fields of a compacted record in a wave's LDS slot, field-major (one ds_read_b128 of a field gives 4
// consecutive entries): x, y, conic a b c, opacity; then r g b (kColor); then the depth value d (kExtra);
// then the entry's Gaussian id as bits (kIds: the backward, which also pads the last quad).
constexpr int kGeomFields = 6;
template <bool kColor_, bool kExtra_, bool kIds_>
struct RecLayout {
    static constexpr bool kColor = kColor_, kExtra = kExtra_, kIds = kIds_;
    static constexpr int kRgbField = kGeomFields;
    static constexpr int kDepthField = kGeomFields + (kColor ? 3 : 0);
    static constexpr int kIdField = kDepthField + (kExtra ? 1 : 0);
    static constexpr int kDataFields = kIdField;                  // 9, 10 or 7
    static constexpr int kRecFields = kIdField + (kIds ? 1 : 0);
    // fields an instantiation does not carry are read from field 0 and never used
    static constexpr int iR = kColor ? kRgbField : 0, iG = kColor ? kRgbField + 1 : 0,
                         iB = kColor ? kRgbField + 2 : 0, iD = kExtra ? kDepthField : 0;
};

// The four entries of a quad q[field] (groups of 4 entries: one ds_read_b128 per field):
// fn(e, x, y, conic a b c, opacity, r, g, b, d), e a std::integral_constant.
template <class L, class Fn>
__device__ __forceinline__ void quad_each(const float4* q, Fn&& fn) {
#define TSPLAT_QUAD(e, m) \
    fn(std::integral_constant<int, e>{}, q[0].m, q[1].m, q[2].m, q[3].m, q[4].m, q[5].m, q[L::iR].m, q[L::iG].m, \
       q[L::iB].m, q[L::iD].m);
    TSPLAT_QUAD(0, x) TSPLAT_QUAD(1, y) TSPLAT_QUAD(2, z) TSPLAT_QUAD(3, w)
#undef TSPLAT_QUAD
}
template <class L>
__device__ __forceinline__ void load_quad(float (*w_rec)[kWave], int i, float4 (&q)[L::kDataFields]) {
#pragma unroll
    for (int f = 0; f < L::kDataFields; ++f) q[f] = *reinterpret_cast<const float4*>(&w_rec[f][i]);
}

// One entry at one pixel: power = -0.5 (a dx^2 + c dy^2) - b dx dy, alpha = min(0.99, o e^power),
// T' = T (1 - alpha), weight w = alpha T (reference renderCUDA), here with the power scaled by log2(e) so
// that e^power = 2^power2 is one v_exp_f32, and the quadratic in Horner form (2 FMAs + 3 multiplies):
// (ca, cb, cc) = log2(e) (-a/2, -b, -c/2), power2 = dy (cc dy + cb dx) + (ca dx) dx.
// Scalar fp32 on purpose: v_pk_fma_f32 has the same FLOP rate as v_fma_f32 (twice the cycles),
// and packing the operands costs register moves.
// Reference order of the decisions: skip power > 0, skip alpha < 1/255, stop if test_T < 1e-4. A skipped
// entry has w = 0 (it adds c * 0 = +0: sums unchanged). Updates the pixel's T and done; T_in is the T the
// entry saw.
struct BlendStep {
    float dx, dy, ex, oe, alpha, T_in, w;
    bool acc;
};
__device__ __forceinline__ BlendStep blend_step(float x, float y, float ca, float cb, float cc, float o, float pfx,
                                                float pfy, float& T, bool& done) {
    BlendStep b;
    b.dx = x - pfx, b.dy = y - pfy;
    const float power2 = fmaf(b.dy, fmaf(cc, b.dy, cb * b.dx), (ca * b.dx) * b.dx);
    b.ex = __builtin_amdgcn_exp2f(power2);
    b.oe = o * b.ex;
    b.alpha = fminf(0.99f, b.oe);
    const float test_T = fmaf(-b.alpha, T, T);
    const bool contrib = !done && !(power2 > 0.0f) && !(b.alpha < 1.0f / 255.0f);
    const bool stop = contrib && (test_T < 0.0001f);
    b.acc = contrib && !stop;
    b.w = b.acc ? b.alpha * T : 0.0f;
    b.T_in = T;
    T = b.acc ? test_T : T;
    done = done || stop;
    return b;
}

// A wave's walk over its tile's sorted list in 64-entry chunks: this lane's record of the next chunk is
// fetched one chunk ahead, the entries whose alpha >= 1/255 box and ellipse can touch the wave's block are
// compacted in depth order into the wave's LDS slot w_rec (conservative, so exact), and body(m) consumes
// the chunk's m compacted entries: the forward blends them, the backward also reduces and scatters their
// gradients. With L::kIds the slot carries each entry's Gaussian id and the last quad is padded with
// entries that contribute nothing (opacity 0: alpha < 1/255). The wave leaves as soon as all its 64 pixels
// are done. No workgroup barriers, so a wave never waits for a busier neighbour.
template <bool kInLds, class L, class Body>
__device__ __forceinline__ void chunk_walk(const Params& p, const Workspace& ws, int v, const TileList& tl,
                                           const uint64_t* skeys, const WavePixel& wp, float (*w_rec)[kWave],
                                           const bool& done, Body&& body) {
    const uint32_t* sids = reinterpret_cast<const uint32_t*>(skeys);  // sorted ids (n <= kSortCap)
    const size_t vbase = (size_t)v * p.G;
    const int n = tl.n, lane = wp.lane;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    float4 r_xy = make_float4(0.f, 0.f, 0.f, 0.f), r_co = r_xy, r_rgb = r_xy, r_cull = r_xy;
    uint32_t r_gid = 0;
    bool r_valid = false;
    auto fetch = [&](int k) {
        r_valid = k < n;
        if (r_valid) {
            // the list's address space is static here, so the LDS read is a ds_read (a generic
            // load would wait on every outstanding load, the previous chunk's prefetch included)
            if constexpr (kInLds)
                r_gid = sids[k];
            else
                r_gid = (uint32_t)tl.gkeys[k];
            const float4* rec = ws.rec + 4 * (vbase + r_gid);
            r_xy = rec[0];
            r_co = rec[1];
            r_rgb = rec[2];
            r_cull = rec[3];
        }
    };
    fetch(lane);
    for (int c0 = 0; c0 < n; c0 += kWave) {
        if (__all(done)) break;
        const float4 xy = r_xy, co = r_co, rgb = r_rgb, cull = r_cull;
        const uint32_t gid = r_gid;
        const bool valid = r_valid;
        fetch(c0 + kWave + lane);
        // order-preserving compaction of the chunk's entries whose alpha >= 1/255 box touches
        // this wave's 8x8 block
        bool hit = valid && !(xy.x + xy.z < wp.wx0 || xy.x - xy.z > wp.wx1 || xy.y + xy.w < wp.wy0 ||
                              xy.y - xy.w > wp.wy1);
        if (hit) hit = ellipse_meets_block(xy.x, xy.y, co, cull, wp.wx0, wp.wx1, wp.wy0, wp.wy1);
        const uint64_t mask = __ballot(hit);
        const int m = p.diag == 4 ? 0 : __popcll(mask);  // diag 4 (forward timing only): walk without blending
        if (hit) {
            const int pos = __popcll(mask & lt_mask);
            w_rec[0][pos] = xy.x;
            w_rec[1][pos] = xy.y;
            w_rec[2][pos] = co.x;
            w_rec[3][pos] = co.y;
            w_rec[4][pos] = co.z;
            w_rec[5][pos] = co.w;
            if constexpr (L::kColor) {
                w_rec[L::kRgbField][pos] = rgb.x;
                w_rec[L::kRgbField + 1][pos] = rgb.y;
                w_rec[L::kRgbField + 2][pos] = rgb.z;
            }
            if constexpr (L::kExtra) w_rec[L::kDepthField][pos] = cull.w;
            if constexpr (L::kIds) w_rec[L::kIdField][pos] = __uint_as_float(gid);
        }
        if constexpr (L::kIds) {
            if (lane < ((m + 3) & ~3) - m) {
#pragma unroll
                for (int f = 0; f < L::kRecFields; ++f) w_rec[f][m + lane] = 0.0f;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        body(m);
        __builtin_amdgcn_wave_barrier();  // reads of this chunk's LDS slots precede the next writes
    }
}

// The walk of a tile list through whichever memory holds it.
template <class L, class Body>
__device__ __forceinline__ void walk_tile(const Params& p, const Workspace& ws, int v, const TileList& tl,
                                          const uint64_t* skeys, const WavePixel& wp, float (*w_rec)[kWave],
                                          const bool& done, Body&& body) {
    if (tl.in_lds)
        chunk_walk<true, L>(p, ws, v, tl, skeys, wp, w_rec, done, body);
    else
        chunk_walk<false, L>(p, ws, v, tl, skeys, wp, w_rec, done, body);
}
