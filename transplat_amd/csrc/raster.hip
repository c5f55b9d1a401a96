// Gaussian-splat rasterizer for gfx950 (MI355X): the forward, and the backward of its colour, depth and
// alpha renders in the Gaussians (tsplat_raster_bwd, tsplat_raster_depth_bwd: render_bwd_kernel and
// preprocess_bwd_kernel, after the forward kernels below, which they leave as they are and whose steps
// they reuse).
//
// Algorithm = the graphdeco forward rasterizer behind `GaussianRasterizer` as called by
// `render_cuda` (reference src/model/decoder/cuda_splatting.py:56-136): preprocess (cull at
// z_view <= 0.2, EWA 2-D covariance with the 1.3*tan(fov) clamp and +0.3 low-pass, conic, 3-sigma
// radius, 16x16 tile rect, SH -> RGB), binning of (Gaussian, tile) instances, front-to-back depth
// order per tile, alpha blending with the 1/255 skip, 0.99 cap and T < 1e-4 stop.
//
// MI355X-first structure (not a translation of the CUDA one):
//   * every view of every scene is rendered by ONE set of launches (blockIdx.y = view); the
//     reference loops views in Python with two host syncs per view;
//   * no global radix sort: tiles are binned by a block-aggregated counting pass (LDS histogram,
//     one global atomic per (block, tile)), and each tile's list is ordered inside the render
//     kernel, keyed (depth bits << 32 | gaussian id) -- exactly the (depth, id) order of the
//     reference's stable sort over id-ordered duplicates -- by an LDS counting sort on the depth
//     bits with a per-bucket rank fix-up (a bitonic network for short or clustered lists);
//   * one 64-byte record per (view, Gaussian) (mean, ellipse extents, conic, opacity, rgb, cull
//     constants), so the render kernel's gather of an entry touches one cache line;
//   * the blend is scalar fp32 (v_pk_fma_f32 has v_fma_f32's FLOP rate and packing costs moves;
//     built with -fno-slp-vectorize), 4 entries per LDS read group.
//
// Floating point: contraction is OFF in this file, so the view-space depth (the sort key) is the
// reference's transformPoint4x3 expression bit for bit -- the front-to-back order, ties included,
// is exactly the reference's. Everything else is this kernel's own arithmetic: the EWA covariance
// as (J R) Sigma (J R)^T, the power in the log2 domain (log2 e folded into the stored conic) and
// the hardware exp2 (v_exp_f32). Parity is held against oracle/raster_ref.c's LITERAL restatement
// of the upstream expressions to L-inf 1e-4, excluding only the pixels whose blend decisions the
// oracle flags as within a rounding margin of their thresholds (tests/test_raster.py).
#pragma clang fp contract(off)

#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "common.h"
#include "prof.h"

namespace tsplat {
namespace raster {

constexpr int kTile = 16;                 // BLOCK_X = BLOCK_Y of the reference rasterizer
constexpr int kTileThreads = kTile * kTile;
constexpr int kSortCap = 4096;            // tile lists up to this length are sorted in LDS
constexpr int kPreThreads = 256;
constexpr size_t kMaxLdsBytes = 160 * 1024;  // gfx950 LDS per workgroup
constexpr int kRecBytes = 64;             // per-(view, Gaussian) record (Workspace::rec)
constexpr int kGeomFields = 6;            // x, y, conic a b c, opacity (then r g b, then the depth value)

__constant__ float kSH_C0 = 0.28209479177387814f;
__constant__ float kSH_C1 = 0.4886025119029199f;
__constant__ float kSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                -1.0925484305920792f, 0.5462742152960396f};
__constant__ float kSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                -0.5900435899266435f};
// Degree-4 real SH constants (same sign convention as the lower degrees).
__constant__ float kSH_C4[9] = {2.5033429417967046f, -1.7701307697799304f, 0.9461746957575601f,
                                -0.6690465435572892f, 0.10578554691520431f, -0.6690465435572892f,
                                0.47308734787878004f, -1.7701307697799304f, 0.6258357354491761f};

struct Workspace {
    // [V*G] 64-byte records, one per (view, Gaussian), so the render kernel's gather of an entry
    // touches one cache line (three SoA arrays cost three lines per entry):
    //   rec[4i + 0] pixel-space mean + half-extents of the alpha >= 1/255 ellipse
    //   rec[4i + 1] conic (a, b, c) as log2(e) (-a/2, -b, -c/2) (the blend's log2-domain power
    //               form) + opacity
    //   rec[4i + 2] rgb + view-space depth
    //   rec[4i + 3] block-cull constants: threshold q, -b/a, -b/c (ellipse_meets_block) + the depth
    //               value d the depth output blends (0 when no depth is asked for)
    float4* rec;
    uint32_t* counts;    // [V*T]
    uint32_t* offsets;   // [V*T + 1]
    uint32_t* cursor;    // [V*T]
    uint64_t* keys;      // [capacity]
};

__host__ __device__ inline Workspace carve(void* base, int G, int V, int T, int capacity,
                                           size_t* total) {
    Workspace w;
    size_t off = 0;
    char* p = (char*)base;
    auto take = [&](size_t bytes) {
        char* r = p ? p + off : nullptr;
        off = align_up(off + bytes, 256);
        return r;
    };
    size_t n = (size_t)V * G;
    w.rec = (float4*)take(n * kRecBytes);
    // counts + cursor contiguous so one memset clears both
    w.counts = (uint32_t*)take((size_t)2 * V * T * sizeof(uint32_t));
    w.cursor = w.counts ? w.counts + (size_t)V * T : nullptr;
    w.offsets = (uint32_t*)take(((size_t)V * T + 1) * sizeof(uint32_t));
    w.keys = (uint64_t*)take((size_t)capacity * sizeof(uint64_t));
    if (total) *total = off;
    return w;
}

struct Params {
    int G, V, vps, H, W, M, deg, tiles_x, tiles_y, T, capacity;
    int diag;  // timing diagnostics only (TSPLAT_RASTER_DIAG; output is wrong when != 0)
    int count_sort;  // 1: counting sort for long tile lists (default); 0: bitonic only (A/B)
    int view_rot;    // render: view v's workgroups take tiles rotated by v * view_rot (load balance)
    int sh_vec4;     // preprocess: every wave's SH block is 16-byte aligned (16-byte staging loads)
    int depth_mode;  // preprocess: -1 no depth value; 0 depth, 1 disparity, 2 relative disparity, 3 log
};

// The value the depth output blends for one (view, Gaussian): the reference renders depth as a
// colour (render_depth_cuda, cuda_splatting.py:375-417): fake colour f of the UNSCALED camera-space
// depth z (:388-400) as the degree-0 SH coefficient, so d = max(C0 f + 0.5, 0). z = vz / s undoes
// the scale-invariant rendering (vz is the depth of the scaled scene). "log" keeps the reference's
// minimum(near).maximum(far) order, which gives log(far) for every Gaussian. IEEE division and logf.
__device__ __forceinline__ float depth_value(int mode, float vz, float s, float near, float far) {
    const float z = vz / s;
    float f = z;
    if (mode == 1) {
        f = 1.0f / z;
    } else if (mode == 2) {
        const float eps = 1e-10f;  // depth_to_relative_disparity (matching/conversions.py:18-28)
        const float disp_near = 1.0f / (near + eps), disp_far = 1.0f / (far + eps);
        f = 1.0f - (1.0f / (z + eps) - disp_far) / (disp_near - disp_far + eps);
    } else if (mode == 3) {
        f = logf(fmaxf(fminf(z, near), far));
    }
    return fmaxf(kSH_C0 * f + 0.5f, 0.0f);
}

__device__ __forceinline__ void get_rect(float px, float py, int r, int tx, int ty, int& x0,
                                         int& y0, int& x1, int& y1) {
    // (int) truncation and clamps exactly as the reference getRect (auxiliary.h)
    x0 = min(tx, max(0, (int)((px - (float)r) / (float)kTile)));
    y0 = min(ty, max(0, (int)((py - (float)r) / (float)kTile)));
    x1 = min(tx, max(0, (int)((px + (float)r + (float)(kTile - 1)) / (float)kTile)));
    y1 = min(ty, max(0, (int)((py + (float)r + (float)(kTile - 1)) / (float)kTile)));
}

__device__ __forceinline__ void sh_to_rgb(const float* __restrict__ sh, int M, int deg, float dx,
                                          float dy, float dz, float out[3]) {
    // sh is colour-major [3][M]; coefficient k of channel c is sh[c*M + k]
    float len = sqrtf(dx * dx + dy * dy + dz * dz);
    float x = dx / len, y = dy / len, z = dz / len;
    float xx = x * x, yy = y * y, zz = z * z;
    float xy = x * y, yz = y * z, xz = x * z;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* s = sh + c * M;
        float r = kSH_C0 * s[0];
        if (deg > 0) {
            r = r - kSH_C1 * y * s[1] + kSH_C1 * z * s[2] - kSH_C1 * x * s[3];
            if (deg > 1) {
                r = r + kSH_C2[0] * xy * s[4] + kSH_C2[1] * yz * s[5] +
                    kSH_C2[2] * (2.0f * zz - xx - yy) * s[6] + kSH_C2[3] * xz * s[7] +
                    kSH_C2[4] * (xx - yy) * s[8];
                if (deg > 2) {
                    r = r + kSH_C3[0] * y * (3.0f * xx - yy) * s[9] + kSH_C3[1] * xy * z * s[10] +
                        kSH_C3[2] * y * (4.0f * zz - xx - yy) * s[11] +
                        kSH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * s[12] +
                        kSH_C3[4] * x * (4.0f * zz - xx - yy) * s[13] +
                        kSH_C3[5] * z * (xx - yy) * s[14] + kSH_C3[6] * x * (xx - 3.0f * yy) * s[15];
                    if (deg > 3) {
                        r = r + kSH_C4[0] * xy * (xx - yy) * s[16] +
                            kSH_C4[1] * yz * (3.0f * xx - yy) * s[17] +
                            kSH_C4[2] * xy * (7.0f * zz - 1.0f) * s[18] +
                            kSH_C4[3] * yz * (7.0f * zz - 3.0f) * s[19] +
                            kSH_C4[4] * (zz * (35.0f * zz - 30.0f) + 3.0f) * s[20] +
                            kSH_C4[5] * xz * (7.0f * zz - 3.0f) * s[21] +
                            kSH_C4[6] * (xx - yy) * (7.0f * zz - 1.0f) * s[22] +
                            kSH_C4[7] * xz * (xx - 3.0f * yy) * s[23] +
                            kSH_C4[8] * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy)) * s[24];
                    }
                }
            }
        }
        r = r + 0.5f;
        out[c] = fmaxf(r, 0.0f);
    }
}

// --- K0: clear the per-tile counters (a kernel, not hipMemsetAsync: a memset captured into a
// hipGraph was observed on ROCm 7.2 to leave garbage in the counters on the second replay) ---
__global__ void __launch_bounds__(256) zero_kernel(uint4* __restrict__ p, size_t n4) {
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
        p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// --- K1: preprocess + per-tile instance counts ----------------------------------------------
// One thread per Gaussian for ALL views of its scene (blockIdx.y = scene): the scene-level inputs
// (mean, covariance, opacity, SH) are read once, not once per view. The SH block of a wave's 64
// Gaussians ([64][3][M] floats, contiguous) is staged into LDS by coalesced 16-byte loads: read
// per thread in place, every load instruction of the wave touches 64 cache lines (a 3M-float
// stride), which made the SH reads half of this kernel's time (TSPLAT_RASTER_DIAG=7 skips them).
constexpr int kMaxShFloats = 75;  // 3 (deg 4 + 1)^2
constexpr int kShStageIt = (kWave * kMaxShFloats / 4 + kWave - 1) / kWave;  // float4s per lane
// kColor: the records get colours (SH staged and evaluated); without it the SH block is neither
// loaded nor evaluated (what TSPLAT_RASTER_DIAG=7 skips). kExtra: the instantiations behind
// tsplat_raster_depth_fwd, which write the depth value into rec[3].w when p.depth_mode >= 0.
template <bool kColor, bool kExtra>
__global__ void __launch_bounds__(kPreThreads)
preprocess_kernel(Params p, const float* __restrict__ means, const float* __restrict__ cov,
                  const float* __restrict__ shs, const float* __restrict__ opacity,
                  const float* __restrict__ viewmat, const float* __restrict__ projmat,
                  const float* __restrict__ campos, const float* __restrict__ tanfov,
                  const float* __restrict__ scene_scale, const float* __restrict__ near,
                  const float* __restrict__ far, int32_t* __restrict__ out_radii, Workspace ws) {
    extern __shared__ uint32_t hist[];  // [T]
    __shared__ __attribute__((aligned(16))) float s_sh[kColor ? kPreThreads * kMaxShFloats : 4];
    const int scene = blockIdx.y;
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const int g = blockIdx.x * kPreThreads + threadIdx.x;
    const int nf = 3 * p.M;
    const size_t sg = (size_t)scene * p.G + g;
    float* my_sh = s_sh + (size_t)threadIdx.x * nf;
    // the SH block's 16-byte loads are issued first and stay in flight through the geometry pass
    // below (pass 1: projection, EWA covariance, records without colour, tile counts, per view);
    // pass 2 stores them to LDS and evaluates the colours of every view
    const int gw0 = blockIdx.x * kPreThreads + wid * kWave;
    const int sh_total = max(0, min(kWave, p.G - gw0)) * nf;
    const float* sh_src = shs + (size_t)nf * ((size_t)scene * p.G + gw0);
    float* sh_dst = s_sh + (size_t)wid * kWave * nf;
    const bool no_sh = !kColor || p.diag == 7;
    const bool stage4 = p.sh_vec4 && !no_sh;
    const int t4 = stage4 ? sh_total / 4 : 0;
    // 19 named registers, loaded unconditionally at a clamped index (held in an array across the
    // geometry pass, the staging lived in scratch memory)
    const float4* sh_src4 = reinterpret_cast<const float4*>(sh_src);
    const int t4c = max(t4 - 1, 0);
    const bool any4 = t4 > 0;
#define TSPLAT_SH_LD(e) \
    float4 shr##e = any4 ? sh_src4[min(lane + (e) * kWave, t4c)] : make_float4(0.f, 0.f, 0.f, 0.f);
    TSPLAT_SH_LD(0) TSPLAT_SH_LD(1) TSPLAT_SH_LD(2) TSPLAT_SH_LD(3) TSPLAT_SH_LD(4) TSPLAT_SH_LD(5)
    TSPLAT_SH_LD(6) TSPLAT_SH_LD(7) TSPLAT_SH_LD(8) TSPLAT_SH_LD(9) TSPLAT_SH_LD(10) TSPLAT_SH_LD(11)
    TSPLAT_SH_LD(12) TSPLAT_SH_LD(13) TSPLAT_SH_LD(14) TSPLAT_SH_LD(15) TSPLAT_SH_LD(16) TSPLAT_SH_LD(17)
    TSPLAT_SH_LD(18)
#undef TSPLAT_SH_LD
    static_assert(kShStageIt == 19, "staging registers are spelled out for 19 float4s per lane");
    // scene-level inputs, once for all views
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, k00 = 0.f, k01 = 0.f, k02 = 0.f, k11 = 0.f, k12 = 0.f, k22 = 0.f,
          o = 0.f;
    if (g < p.G) {
        m0 = means[3 * sg];
        m1 = means[3 * sg + 1];
        m2 = means[3 * sg + 2];
        const float* C = cov + 9 * sg;
        k00 = C[0];
        k01 = C[1];
        k02 = C[2];
        k11 = C[4];
        k12 = C[5];
        k22 = C[8];
        o = opacity[sg];
    }

    uint32_t okmask = 0;  // bit vv: the Gaussian is rendered in view vv (vps <= 32, host-checked)
    for (int vv = 0; vv < p.vps; ++vv) {
        const int v = scene * p.vps + vv;
        for (int i = threadIdx.x; i < p.T; i += kPreThreads) hist[i] = 0;
        __syncthreads();  // hist cleared
        if (g < p.G) {
            const size_t vg = (size_t)v * p.G + g;
            const float* vm = viewmat + 16 * v;
            const float* pm = projmat + 16 * v;
            const float s = scene_scale[2 * v], s2 = scene_scale[2 * v + 1];
            int radius = 0;
            // scale-invariant rendering: means * s, cov * s^2 (cuda_splatting.py:73-80)
            const float mx = m0 * s, my = m1 * s, mz = m2 * s;
            // in_frustum: view-space depth test (auxiliary.h in_frustum)
            const float vx = vm[0] * mx + vm[4] * my + vm[8] * mz + vm[12];
            const float vy = vm[1] * mx + vm[5] * my + vm[9] * mz + vm[13];
            const float vz = vm[2] * mx + vm[6] * my + vm[10] * mz + vm[14];
            bool ok = vz > 0.2f;
            float px = 0.f, py = 0.f, conic_a = 0.f, conic_b = 0.f, conic_c = 0.f;
            float cov_a = 0.f, cov_c = 0.f;
            int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
            if (ok) {
                const float hx = pm[0] * mx + pm[4] * my + pm[8] * mz + pm[12];
                const float hy = pm[1] * mx + pm[5] * my + pm[9] * mz + pm[13];
                const float hw = pm[3] * mx + pm[7] * my + pm[11] * mz + pm[15];
                const float pw = 1.0f / (hw + 0.0000001f);
                const float ndc_x = hx * pw, ndc_y = hy * pw;
                const float c00 = k00 * s2, c01 = k01 * s2, c02 = k02 * s2;
                const float c11 = k11 * s2, c12 = k12 * s2, c22 = k22 * s2;
                // EWA splatting (computeCov2D)
                const float tfx = tanfov[2 * v], tfy = tanfov[2 * v + 1];
                const float fx = (float)p.W / (2.0f * tfx), fy = (float)p.H / (2.0f * tfy);
                const float limx = 1.3f * tfx, limy = 1.3f * tfy;
                const float tz = vz;
                const float tx = fminf(limx, fmaxf(-limx, vx / tz)) * tz;
                const float ty = fminf(limy, fmaxf(-limy, vy / tz)) * tz;
                const float j00 = fx / tz, j02 = -(fx * tx) / (tz * tz);
                const float j11 = fy / tz, j12 = -(fy * ty) / (tz * tz);
                // M = J * R_w2c, R[r][c] = vm[c*4 + r]
                const float n00 = j00 * vm[0] + j02 * vm[2];
                const float n01 = j00 * vm[4] + j02 * vm[6];
                const float n02 = j00 * vm[8] + j02 * vm[10];
                const float n10 = j11 * vm[1] + j12 * vm[2];
                const float n11 = j11 * vm[5] + j12 * vm[6];
                const float n12 = j11 * vm[9] + j12 * vm[10];
                const float u00 = n00 * c00 + n01 * c01 + n02 * c02;
                const float u01 = n00 * c01 + n01 * c11 + n02 * c12;
                const float u02 = n00 * c02 + n01 * c12 + n02 * c22;
                const float u10 = n10 * c00 + n11 * c01 + n12 * c02;
                const float u11 = n10 * c01 + n11 * c11 + n12 * c12;
                const float u12 = n10 * c02 + n11 * c12 + n12 * c22;
                const float a = u00 * n00 + u01 * n01 + u02 * n02 + 0.3f;
                const float b = u00 * n10 + u01 * n11 + u02 * n12;
                const float c = u10 * n10 + u11 * n11 + u12 * n12 + 0.3f;
                const float det = a * c - b * b;
                cov_a = a;
                cov_c = c;
                ok = det != 0.0f;
                if (ok) {
                    const float det_inv = 1.0f / det;
                    conic_a = c * det_inv;
                    conic_b = -b * det_inv;
                    conic_c = a * det_inv;
                    const float mid = 0.5f * (a + c);
                    const float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
                    const float l2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
                    radius = (int)ceilf(3.0f * sqrtf(fmaxf(l1, l2)));
                    px = ((ndc_x + 1.0f) * (float)p.W - 1.0f) * 0.5f;
                    py = ((ndc_y + 1.0f) * (float)p.H - 1.0f) * 0.5f;
                    get_rect(px, py, radius, p.tiles_x, p.tiles_y, x0, y0, x1, y1);
                    ok = (x1 - x0) * (y1 - y0) != 0;
                }
            }
            if (ok) {
                okmask |= 1u << vv;
                // Conservative half-extents of the region where o * exp(power) >= 1/255 (power =
                // -Q/2, Q <= 2 ln(255 o)); lets a wave skip Gaussians that miss its 8x8 pixels.
                // Pure culling: pixels inside keep the exact reference arithmetic.
                float ex = INFINITY, ey = INFINITY;
                if (o == o) {
                    const float q = 2.0f * logf(255.0f * o);
                    if (q < 0.0f) {
                        ex = ey = -1.0f;  // alpha < 1/255 everywhere
                    } else if (cov_a > 0.0f && cov_c > 0.0f && q < INFINITY) {
                        ex = sqrtf(q * cov_a) * 1.001f + 0.01f;
                        ey = sqrtf(q * cov_c) * 1.001f + 0.01f;
                    }
                }
                float4* rec = ws.rec + 4 * vg;
                rec[0] = make_float4(px, py, ex, ey);
                // power * log2(e): alpha = o * 2^(power2) is one v_exp_f32 in the blend
                constexpr float kLog2e = 1.44269504088896341f;
                rec[1] = make_float4(-0.5f * kLog2e * conic_a, -kLog2e * conic_b, -0.5f * kLog2e * conic_c, o);
                // cull threshold in the same log2 units as the stored conic: 2 log2(255 o), + margins
                float d = 0.0f;
                if constexpr (kExtra)
                    if (p.depth_mode >= 0) d = depth_value(p.depth_mode, vz, s, near[v], far[v]);
                rec[3] = make_float4(2.0f * __log2f(255.0f * o) * 1.001f + 1.5e-3f,
                                     -conic_b * __builtin_amdgcn_rcpf(conic_a),
                                     -conic_b * __builtin_amdgcn_rcpf(conic_c), d);
                for (int ty = y0; ty < y1; ++ty)
                    for (int tx = x0; tx < x1; ++tx) atomicAdd(&hist[ty * p.tiles_x + tx], 1u);
            } else {
                radius = 0;
            }
            out_radii[vg] = radius;
        }
        __syncthreads();
        uint32_t* gcount = ws.counts + (size_t)v * p.T;
        for (int i = threadIdx.x; i < p.T; i += kPreThreads)
            if (hist[i]) atomicAdd(&gcount[i], hist[i]);
        // the next view's clear of hist[i] is by this same thread, after its read above
    }

    // pass 2: the staged SH to LDS (this wave's own block: a wave barrier orders it), then colours
    float4* sh_dst4 = reinterpret_cast<float4*>(sh_dst);
#define TSPLAT_SH_ST(e) \
    if (lane + (e) * kWave < t4) sh_dst4[lane + (e) * kWave] = shr##e;
    TSPLAT_SH_ST(0) TSPLAT_SH_ST(1) TSPLAT_SH_ST(2) TSPLAT_SH_ST(3) TSPLAT_SH_ST(4) TSPLAT_SH_ST(5)
    TSPLAT_SH_ST(6) TSPLAT_SH_ST(7) TSPLAT_SH_ST(8) TSPLAT_SH_ST(9) TSPLAT_SH_ST(10) TSPLAT_SH_ST(11)
    TSPLAT_SH_ST(12) TSPLAT_SH_ST(13) TSPLAT_SH_ST(14) TSPLAT_SH_ST(15) TSPLAT_SH_ST(16) TSPLAT_SH_ST(17)
    TSPLAT_SH_ST(18)
#undef TSPLAT_SH_ST
    if (!no_sh)
        for (int i = 4 * t4 + lane; i < sh_total; i += kWave) sh_dst[i] = sh_src[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int vv = 0; vv < p.vps; ++vv) {
        if (!((okmask >> vv) & 1u)) continue;
        const int v = scene * p.vps + vv;
        const float* vm = viewmat + 16 * v;
        const float s = scene_scale[2 * v];
        const float mx = m0 * s, my = m1 * s, mz = m2 * s;
        const float vz = vm[2] * mx + vm[6] * my + vm[10] * mz + vm[14];  // as in pass 1, bit for bit
        float rgb[3] = {0.5f, 0.5f, 0.5f};
        const float* cp = campos + 3 * v;
        if (!no_sh) sh_to_rgb(my_sh, p.M, p.deg, mx - cp[0], my - cp[1], mz - cp[2], rgb);
        ws.rec[4 * ((size_t)v * p.G + g) + 2] = make_float4(rgb[0], rgb[1], rgb[2], vz);
    }
}

// --- K3: scatter (gaussian, tile) instances into per-tile ranges ------------------------------
// The exclusive scan of the V*T tile counts is folded in (it was a single-workgroup launch of its
// own): each workgroup sums the counts of the views before its own and scans its view's T counts
// in LDS; the x = 0 workgroup of each view publishes that view's offsets for the render kernel,
// and the last view's also the total (offsets[V T]) and the capacity-overflow status.
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t x, uint32_t* red) {
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
    if (lane == 0) red[wid] = x;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kPreThreads / kWave; ++w) t += red[w];
    return t;
}

__global__ void __launch_bounds__(kPreThreads)
scatter_kernel(Params p, const int32_t* __restrict__ radii, Workspace ws, int32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];  // hist[T], base[T], pre[T]
    uint32_t* hist = lds;
    uint32_t* base = lds + p.T;
    uint32_t* pre = lds + 2 * p.T;
    __shared__ uint32_t red[2][kPreThreads / kWave];
    const int v = blockIdx.y;
    const int g = blockIdx.x * kPreThreads + threadIdx.x;
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    for (int i = threadIdx.x; i < p.T; i += kPreThreads) hist[i] = 0;
    // this view's tile counts: thread t owns the contiguous segment [t k, t k + k), k = ceil(T / 256)
    const uint32_t* vcount = ws.counts + (size_t)v * p.T;
    const int seg = (p.T + kPreThreads - 1) / kPreThreads;
    const int s0 = min(p.T, (int)threadIdx.x * seg), s1 = min(p.T, s0 + seg);
    uint32_t own = 0;
    for (int i = s0; i < s1; ++i) own += vcount[i];
    uint32_t prior = 0;  // counts of the views before this one
    for (size_t i = threadIdx.x; i < (size_t)v * p.T; i += kPreThreads) prior += ws.counts[i];
    prior = block_sum_u32(prior, red[0]);  // (its barrier also orders the hist clear)
    uint32_t incl = own;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d, kWave);
        if (lane >= d) incl += y;
    }
    if (lane == kWave - 1) red[1][wid] = incl;
    __syncthreads();
    uint32_t run = prior + incl - own;
    for (int w = 0; w < wid; ++w) run += red[1][w];
    for (int i = s0; i < s1; ++i) {
        pre[i] = run;
        run += vcount[i];
    }
    if (blockIdx.x == 0) {
        uint32_t* off = ws.offsets + (size_t)v * p.T;
        for (int i = s0; i < s1; ++i) off[i] = pre[i];
        if (v == p.V - 1 && threadIdx.x == kPreThreads - 1) {  // holds the view's last segment
            ws.offsets[(size_t)p.V * p.T] = run;
            if (run > (uint32_t)p.capacity) atomicOr(status, 1);
        }
    }
    __syncthreads();
    int r = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    uint64_t key_lo = 0, depth_bits = 0;
    const size_t vg = (size_t)v * p.G + g;
    if (g < p.G) {
        r = radii[vg];
        if (r > 0) {
            const float4 xy = ws.rec[4 * vg];
            get_rect(xy.x, xy.y, r, p.tiles_x, p.tiles_y, x0, y0, x1, y1);
            depth_bits = (uint64_t)__float_as_uint(ws.rec[4 * vg + 2].w);
            key_lo = (uint64_t)(uint32_t)g;
            for (int ty = y0; ty < y1; ++ty)
                for (int tx = x0; tx < x1; ++tx) atomicAdd(&hist[ty * p.tiles_x + tx], 1u);
        }
    }
    __syncthreads();
    uint32_t* gcur = ws.cursor + (size_t)v * p.T;
    for (int i = threadIdx.x; i < p.T; i += kPreThreads) {
        uint32_t h = hist[i];
        base[i] = h ? pre[i] + atomicAdd(&gcur[i], h) : 0u;
        hist[i] = 0;
    }
    __syncthreads();
    if (r > 0) {
        const uint64_t key = (depth_bits << 32) | key_lo;
        for (int ty = y0; ty < y1; ++ty)
            for (int tx = x0; tx < x1; ++tx) {
                const int t = ty * p.tiles_x + tx;
                const uint32_t pos = base[t] + atomicAdd(&hist[t], 1u);
                if (pos < (uint32_t)p.capacity) ws.keys[pos] = key;
            }
    }
}

// Bitonic sort (all-ascending "mirror" network) of n keys held in `buf`, virtual length
// next_pow2(n); positions >= n behave as +inf and never move, so no padding is written.
template <typename Ptr>
__device__ __forceinline__ void bitonic_sort(Ptr buf, int n) {
    int logP = 0;
    while ((1 << logP) < n) ++logP;
    const int half = (1 << logP) >> 1;
    for (int lk = 1; lk <= logP; ++lk) {
        for (int lj = lk - 1; lj >= 0; --lj) {
            const int j = 1 << lj;
            for (int i = threadIdx.x; i < half; i += kTileThreads) {
                const int blk = i >> lj, q = i & (j - 1);
                int a, b;
                if (lj == lk - 1) {  // first step of a merge: compare mirrored pairs
                    a = (blk << (lj + 1)) + q;
                    b = (blk << (lj + 1)) + (2 * j - 1 - q);
                } else {
                    a = (blk << (lj + 1)) + q;
                    b = a + j;
                }
                if (b < n) {
                    const uint64_t ka = buf[a], kb = buf[b];
                    if (ka > kb) {
                        buf[a] = kb;
                        buf[b] = ka;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// Register-resident bitonic sort of the n <= kSortCap keys in `buf` (LDS), ascending. Thread t
// holds positions t*E .. t*E + E - 1 (E = P / 256 for P = next_pow2(n) >= 256; positions >= n
// are +inf). The network is unrolled at compile time (template over log2 P), so every register
// index is static: stages whose partner distance j is below E run in registers, j < 64 E
// exchange with the partner lane by shuffles, and only j >= 64 E (at most 3 stages for 4096
// keys) go through LDS with barriers -- instead of one barrier-separated LDS pass per stage.
template <int E>
__device__ __forceinline__ void cas_step(uint64_t (&v)[E], int t, int k, int j, uint64_t* buf) {
    if (j < E) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int f = e ^ j;
            if (f > e) {
                const bool asc = (((t * E + e) & k) == 0);
                const uint64_t a = v[e], b = v[f];
                const bool sw = asc ? (a > b) : (a < b);
                v[e] = sw ? b : a;
                v[f] = sw ? a : b;
            }
        }
    } else if (j < 64 * E) {
        const int lane_xor = j / E;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = t * E + e;
            const uint32_t lo = __shfl_xor((uint32_t)v[e], lane_xor);
            const uint32_t hi = __shfl_xor((uint32_t)(v[e] >> 32), lane_xor);
            const uint64_t other = ((uint64_t)hi << 32) | lo;
            const bool take_min = ((i & j) == 0) == ((i & k) == 0);
            const uint64_t mn = v[e] < other ? v[e] : other, mx = v[e] < other ? other : v[e];
            v[e] = take_min ? mn : mx;
        }
    } else {
        __syncthreads();  // previous readers of buf are done
#pragma unroll
        for (int e = 0; e < E; ++e) buf[t * E + e] = v[e];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = t * E + e;
            const uint64_t other = buf[i ^ j];
            const bool take_min = ((i & j) == 0) == ((i & k) == 0);
            const uint64_t mn = v[e] < other ? v[e] : other, mx = v[e] < other ? other : v[e];
            v[e] = take_min ? mn : mx;
        }
    }
}

template <int LOGP>
__device__ __forceinline__ void bitonic_sort_regs_p(uint64_t* buf, int n) {
    constexpr int P = 1 << LOGP;
    constexpr int E = P / kTileThreads;
    const int t = threadIdx.x;
    uint64_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t * E + e;
        v[e] = i < n ? buf[i] : ~0ull;
    }
#pragma unroll
    for (int lk = 1; lk <= LOGP; ++lk)
#pragma unroll
        for (int lj = lk - 1; lj >= 0; --lj) cas_step<E>(v, t, 1 << lk, 1 << lj, buf);
    __syncthreads();
    // sorted gaussian ids (the keys' low words) as a uint32 list at the start of buf
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t * E + e;
        if (i < n) reinterpret_cast<uint32_t*>(buf)[i] = (uint32_t)v[e];
    }
    __syncthreads();
}

__device__ __forceinline__ void bitonic_sort_regs(uint64_t* buf, int n) {
    if (n <= 256) bitonic_sort_regs_p<8>(buf, n);
    else if (n <= 512) bitonic_sort_regs_p<9>(buf, n);
    else if (n <= 1024) bitonic_sort_regs_p<10>(buf, n);
    else if (n <= 2048) bitonic_sort_regs_p<11>(buf, n);
    else bitonic_sort_regs_p<12>(buf, n);
}

// Counting sort of a tile list on its depth bits, for lists longer than one bitonic register pass.
// Depths are positive floats, so their bit patterns order like the depths. bucket(d) = (d - dmin)
// >> s, with s the smallest shift that maps the tile's depth-bit range onto <= kBuckets buckets:
// monotone in depth, so concatenating the buckets in order is a depth order. Each thread holds E
// keys in registers (key i = t + 256 e, one coalesced load batch); the keys are scattered to their
// bucket's slice of `out` by LDS atomics, and a key's final slot in its bucket -- almost always 0-2
// keys -- is its bucket start + the number of bucket members with a smaller (depth bits << 32 | id)
// key, so the result is exactly the ascending key order the bitonic network produces. A tile
// whose depths cluster (some bucket holds more than kFixMax keys) returns false before anything
// is written and takes the bitonic path.
constexpr int kBuckets = 2048;
constexpr int kBucketBits = 11;
constexpr int kFixMax = 32;

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}

template <int E>
__device__ bool counting_sort_e(const uint64_t* __restrict__ keys, int n, uint64_t* out, uint32_t* cnt,
                                uint32_t* red) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    constexpr int kPer = kBuckets / kTileThreads;  // consecutive buckets per thread in the scan
    uint64_t k[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid + e * kTileThreads;
        k[e] = i < n ? keys[i] : ~0ull;
    }
    for (int i = tid; i < kBuckets; i += kTileThreads) cnt[i] = 0;
    if (tid == 0) {
        red[0] = 0xffffffffu;
        red[1] = 0u;
        red[2] = 0u;
    }
    uint32_t lo = 0xffffffffu, hi = 0u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (tid + e * kTileThreads < n) {
            const uint32_t d = (uint32_t)(k[e] >> 32);
            lo = min(lo, d);
            hi = max(hi, d);
        }
    }
    lo = wave_min_u32(lo);
    hi = wave_max_u32(hi);
    __syncthreads();  // red and cnt initialised
    if (lane == 0) {
        atomicMin(&red[0], lo);
        atomicMax(&red[1], hi);
    }
    __syncthreads();
    const uint32_t dmin = red[0], range = red[1] - dmin;
    const int bits = range ? 32 - __clz(range) : 0;
    const int sh = bits > kBucketBits ? bits - kBucketBits : 0;
    uint32_t bk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool valid = tid + e * kTileThreads < n;
        bk[e] = valid ? ((uint32_t)(k[e] >> 32) - dmin) >> sh : 0u;
        if (valid) atomicAdd(&cnt[bk[e]], 1u);
    }
    __syncthreads();
    // exclusive scan of the bucket counts (thread t owns buckets kPer t .. kPer t + kPer - 1) and
    // the largest bucket
    uint32_t c[kPer];
    uint32_t sum = 0, mx = 0;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        c[e] = cnt[tid * kPer + e];
        sum += c[e];
        mx = max(mx, c[e]);
    }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += y;
    }
    mx = wave_max_u32(mx);
    __shared__ uint32_t wtot[kTileThreads / kWave];
    if (lane == kWave - 1) wtot[wid] = incl;
    if (lane == 0) atomicMax(&red[2], mx);
    __syncthreads();
    if (red[2] > (uint32_t)kFixMax) return false;  // uniform: every thread read the same value
    uint32_t run = incl - sum;
    for (int w = 0; w < wid; ++w) run += wtot[w];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        cnt[tid * kPer + e] = run;
        run += c[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (tid + e * kTileThreads < n) out[atomicAdd(&cnt[bk[e]], 1u)] = k[e];
    __syncthreads();  // cnt[b] is now the end of bucket b
    uint32_t slot[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t b = tid + e * kTileThreads < n ? bk[e] : 0u;  // padding keys: any bucket
        const uint32_t s0 = b ? cnt[b - 1] : 0u, s1 = cnt[b];
        uint32_t r = 0;
        for (uint32_t j = s0; j < s1; ++j) r += out[j] < k[e];
        slot[e] = s0 + r;
    }
    __syncthreads();
    // every read of the 64-bit keys is done: leave the sorted gaussian ids (the keys' low words)
    // as a uint32 list at the start of the same LDS region
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (tid + e * kTileThreads < n) reinterpret_cast<uint32_t*>(out)[slot[e]] = (uint32_t)k[e];
    __syncthreads();
    return true;
}

__device__ __forceinline__ bool counting_sort(const uint64_t* __restrict__ keys, int n, uint64_t* out,
                                              uint32_t* cnt, uint32_t* red) {
    if (n <= 2 * kTileThreads) return counting_sort_e<2>(keys, n, out, cnt, red);
    if (n <= 4 * kTileThreads) return counting_sort_e<4>(keys, n, out, cnt, red);
    if (n <= 8 * kTileThreads) return counting_sort_e<8>(keys, n, out, cnt, red);
    return counting_sort_e<16>(keys, n, out, cnt, red);
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

// --- K4: per-tile depth sort + front-to-back alpha blending ---------------------------------
// One workgroup per (tile, view); the tile list is sorted in LDS (counting sort, or the bitonic
// network), then each wave owns
// an 8x8 pixel block and walks the sorted list on its own in 64-entry chunks (no workgroup
// barriers, so a wave never waits for a busier neighbour): the chunk's records are fetched one
// chunk ahead, the entries whose alpha >= 1/255 box can touch the block are compacted in depth
// order into the wave's LDS slot (conservative, so exact) and blended branch-free; the wave
// leaves as soon as all its 64 pixels are saturated.
//
// Three instantiations. <colour, no extras> is tsplat_raster_fwd's kernel. With kExtra
// (tsplat_raster_depth_fwd) the compaction carries a further field, the depth value d of
// rec[3].w, the blend accumulates D += d w with the colour's own weight w = alpha T, and the
// kernel stores out_depth = D (no background term: the reference renders depth over black) and
// out_alpha = 1 - T, each where its pointer is set. Without kColor the three rgb fields and
// their accumulators are gone (the depth-only call). Every blend decision is the same code in all
// three, so their weights agree bit for bit.
template <bool kColor, bool kExtra>
__global__ void __launch_bounds__(kTileThreads)
render_kernel(Params p, const float* __restrict__ bg, float* __restrict__ out_color,
              float* __restrict__ out_depth, float* __restrict__ out_alpha, Workspace ws) {
    constexpr int kRgbField = kGeomFields;                          // r g b (kColor)
    constexpr int kDepthField = kGeomFields + (kColor ? 3 : 0);     // d (kExtra)
    constexpr int kRecFields = kDepthField + (kExtra ? 1 : 0);      // 9, 10 or 7
    __shared__ uint64_t skeys[kSortCap];
    __shared__ uint32_t s_cnt[kBuckets];
    __shared__ uint32_t s_red[4];
    // per-wave compacted records of the current 64-entry chunk (waves progress independently),
    // field-major: one ds_read_b128 of a field gives 4 consecutive entries = 2 packed pairs
    __shared__ __attribute__((aligned(16))) float s_rec[kTileThreads / kWave][kRecFields][kWave];

    const int v = blockIdx.y;
    // Workgroup (tile, v) and (tile, v') share an XCD and a CU slot in dispatch order, and a
    // tile's cost is similar across the target views of a scene (central tiles are the heavy
    // ones), so without the per-view rotation every CU would get the same tile three times.
    // Rotating by whole tile rows keeps each XCD's band of rows contiguous (L2 reuse of records).
    int tile = xcd_remap(blockIdx.x, gridDim.x) + v * p.view_rot;
    tile %= p.T;
    const uint64_t t_begin = p.diag == 5 ? __builtin_amdgcn_s_memtime() : 0;
    int d_entries = 0, d_chunks = 0;  // diag 5 only
    const int tx = tile % p.tiles_x, ty = tile / p.tiles_x;
    const int t_idx = v * p.T + tile;
    uint32_t start = ws.offsets[t_idx];
    uint32_t end = ws.offsets[t_idx + 1];
    if (end > (uint32_t)p.capacity) end = (uint32_t)p.capacity;
    if (start > end) start = end;
    const int n = (int)(end - start);

    uint64_t* gkeys = ws.keys + start;
    const bool in_lds = n <= kSortCap;
    if (in_lds) {
        // lists longer than one register pass: counting sort on the depth bits (falls back to the
        // bitonic network when the tile's depths cluster)
        const bool try_count = p.count_sort && n > kTileThreads && p.diag != 3;
        const bool counted = try_count && counting_sort(gkeys, n, skeys, s_cnt, s_red);
        if (!counted) {
            for (int i = threadIdx.x; i < n; i += kTileThreads) skeys[i] = gkeys[i];
            __syncthreads();
            if (p.diag == 3) return;  // key load only
            bitonic_sort_regs(skeys, n);
        }
        if (p.diag == 2) return;  // key load + sort
    } else {
        bitonic_sort(gkeys, n);  // rare: very long tile list, sorted in place in global memory
    }
    // no workgroup barrier below this point: each wave walks the sorted list on its own

    const int wid = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int lx = (wid & 1) * 8 + (lane & 7), ly = (wid >> 1) * 8 + (lane >> 3);
    const int pxi = tx * kTile + lx, pyi = ty * kTile + ly;
    const float wx0 = (float)(tx * kTile + (wid & 1) * 8), wx1 = wx0 + 7.0f;
    const float wy0 = (float)(ty * kTile + (wid >> 1) * 8), wy1 = wy0 + 7.0f;
    const bool inside = pxi < p.W && pyi < p.H;
    bool done = !inside;
    const float pfx = (float)pxi, pfy = (float)pyi;
    float T = 1.0f;
    float C0 = 0.f, C1 = 0.f, C2 = 0.f;
    float D = 0.f;  // kExtra: sum of d w
    const size_t vbase = (size_t)v * p.G;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    float (*w_rec)[kWave] = s_rec[wid];

    // power = -0.5 (a dx^2 + c dy^2) - b dx dy, alpha = min(0.99, o e^power), T' = T (1 - alpha),
    // C += rgb alpha T (reference renderCUDA), here with the power scaled by log2(e) so that
    // e^power = 2^power2 is one v_exp_f32, and the quadratic in Horner form (2 FMAs + 3 multiplies).
    // Scalar fp32 on purpose: v_pk_fma_f32 has the same FLOP rate as v_fma_f32 (twice the cycles),
    // and packing the operands costs register moves.
    auto blend = [&](float x, float y, float ca, float cb, float cc, float o, float r, float g, float bl,
                     float d) {
        // (ca, cb, cc) = log2(e) (-a/2, -b, -c/2): power2 = dy (cc dy + cb dx) + (ca dx) dx
        const float dx = x - pfx, dy = y - pfy;
        const float power2 = fmaf(dy, fmaf(cc, dy, cb * dx), (ca * dx) * dx);
        const float alpha = fminf(0.99f, o * __builtin_amdgcn_exp2f(power2));
        const float test_T = fmaf(-alpha, T, T);
        // reference order: skip power > 0, skip alpha < 1/255, stop if test_T < 1e-4
        const bool contrib = !done && !(power2 > 0.0f) && !(alpha < 1.0f / 255.0f);
        const bool stop = contrib && (test_T < 0.0001f);
        const bool acc = contrib && !stop;
        const float w = acc ? alpha * T : 0.0f;  // a skipped entry adds c * 0 = +0: C unchanged
        if constexpr (kColor) {
            C0 = fmaf(r, w, C0);
            C1 = fmaf(g, w, C1);
            C2 = fmaf(bl, w, C2);
        }
        if constexpr (kExtra) D = fmaf(d, w, D);
        T = acc ? test_T : T;
        done = done || stop;
    };
    // fields an instantiation does not carry are read from field 0 and never used
    constexpr int iR = kColor ? kRgbField : 0, iG = kColor ? kRgbField + 1 : 0, iB = kColor ? kRgbField + 2 : 0;
    constexpr int iD = kExtra ? kDepthField : 0;

    struct Quad {
        float4 f[kRecFields];
    };
    auto load_quad = [&](int i, Quad& q) {
#pragma unroll
        for (int f = 0; f < kRecFields; ++f) q.f[f] = *reinterpret_cast<const float4*>(&w_rec[f][i]);
    };
    auto blend_quad = [&](const Quad& q) {
        const float4* f = q.f;
        blend(f[0].x, f[1].x, f[2].x, f[3].x, f[4].x, f[5].x, f[iR].x, f[iG].x, f[iB].x, f[iD].x);
        blend(f[0].y, f[1].y, f[2].y, f[3].y, f[4].y, f[5].y, f[iR].y, f[iG].y, f[iB].y, f[iD].y);
        blend(f[0].z, f[1].z, f[2].z, f[3].z, f[4].z, f[5].z, f[iR].z, f[iG].z, f[iB].z, f[iD].z);
        blend(f[0].w, f[1].w, f[2].w, f[3].w, f[4].w, f[5].w, f[iR].w, f[iG].w, f[iB].w, f[iD].w);
    };

    const uint32_t* sids = reinterpret_cast<const uint32_t*>(skeys);  // sorted ids (n <= kSortCap)
    auto walk = [&](auto lds_tag) {
        constexpr bool kInLds = decltype(lds_tag)::value;
        // this lane's record of the next 64-entry chunk, fetched one chunk ahead
        float4 r_xy = make_float4(0.f, 0.f, 0.f, 0.f), r_co = r_xy, r_rgb = r_xy, r_cull = r_xy;
        bool r_valid = false;
        auto fetch = [&](int k) {
            r_valid = k < n;
            if (r_valid) {
                // the list's address space is static here, so the LDS read is a ds_read (a generic
                // load would wait on every outstanding load, the previous chunk's prefetch included)
                uint32_t gid;
                if constexpr (kInLds)
                    gid = sids[k];
                else
                    gid = (uint32_t)gkeys[k];
                const float4* rec = ws.rec + 4 * (vbase + gid);
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
            const bool valid = r_valid;
            fetch(c0 + kWave + lane);
            // order-preserving compaction of the chunk's entries whose alpha >= 1/255 box touches
            // this wave's 8x8 block
            bool hit = valid && !(xy.x + xy.z < wx0 || xy.x - xy.z > wx1 || xy.y + xy.w < wy0 ||
                                  xy.y - xy.w > wy1);
            if (hit) hit = ellipse_meets_block(xy.x, xy.y, co, cull, wx0, wx1, wy0, wy1);
            const uint64_t mask = __ballot(hit);
            const int m = p.diag == 4 ? 0 : __popcll(mask);
            d_entries += m;
            ++d_chunks;
            if (hit) {
                const int pos = __popcll(mask & lt_mask);
                w_rec[0][pos] = xy.x;
                w_rec[1][pos] = xy.y;
                w_rec[2][pos] = co.x;
                w_rec[3][pos] = co.y;
                w_rec[4][pos] = co.z;
                w_rec[5][pos] = co.w;
                if constexpr (kColor) {
                    w_rec[kRgbField][pos] = rgb.x;
                    w_rec[kRgbField + 1][pos] = rgb.y;
                    w_rec[kRgbField + 2][pos] = rgb.z;
                }
                if constexpr (kExtra) w_rec[kDepthField][pos] = cull.w;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // groups of 4 entries: one ds_read_b128 per field
            const int m4 = m & ~3;
            for (int i = 0; i < m4; i += 4) {
                Quad q;
                load_quad(i, q);
                blend_quad(q);
            }
            for (int i = m4; i < m; ++i)
                blend(w_rec[0][i], w_rec[1][i], w_rec[2][i], w_rec[3][i], w_rec[4][i], w_rec[5][i], w_rec[iR][i],
                      w_rec[iG][i], w_rec[iB][i], w_rec[iD][i]);
            __builtin_amdgcn_wave_barrier();  // reads of this chunk's records precede the next writes
        }
    };
    if (in_lds)
        walk(std::true_type{});
    else
        walk(std::false_type{});
    if (p.diag == 5) {  // per-wave cost instead of colours: cycles since the start, entries, chunks
        C0 = (float)(__builtin_amdgcn_s_memtime() - t_begin);
        C1 = (float)d_entries;
        C2 = (float)d_chunks;
        T = 0.0f;
    }
    if (inside) {
        const size_t hw = (size_t)p.H * p.W;
        const size_t pix = (size_t)pyi * p.W + pxi;
        if constexpr (kColor) {
            float* o = out_color + (size_t)v * 3 * hw + pix;
            const float* bgv = bg + 3 * v;
            o[0] = C0 + T * bgv[0];
            o[hw] = C1 + T * bgv[1];
            o[2 * hw] = C2 + T * bgv[2];
        }
        if constexpr (kExtra) {
            if (out_depth) out_depth[(size_t)v * hw + pix] = D;
            if (out_alpha) out_alpha[(size_t)v * hw + pix] = 1.0f - T;
        }
    }
}

// =============================================================================================
// Backward of render_kernel<true, false> / preprocess_kernel<true, false> (tsplat_raster_bwd): the
// exact vector-Jacobian product of the colour render in (means, covariances, SH, opacities) with
// every discrete decision of the forward held fixed. Two launches after a zero fill of the
// gradient records:
//   render_bwd_kernel      per (view, Gaussian): sums over pixels of d px, d py, d conic (a, b, c),
//                          d opacity, d rgb -> 64-byte gradient records (float atomics)
//   preprocess_bwd_kernel  per Gaussian: the chain conic <- 2-D covariance <- J R <- (3-D
//                          covariance, mean), pixel mean <- projection, colour <- SH and view
//                          direction, s and s^2; summed over the scene's views in registers
// =============================================================================================
constexpr int kGradRecFloats = 16;  // gradient record of a (view, Gaussian): 64 bytes = one atomic request
// fields of a gradient record: 0 px, 1 py (pixel-space mean); 2 3 4 the PLAIN conic (a, b, c) of
// power = -(a dx^2 + c dy^2) / 2 - b dx dy (not the log2-scaled form the forward stores: the
// factors log2(e) ln(2) cancel here, so preprocess_bwd_kernel needs no constant); 5 opacity;
// 6 7 8 the clamped colour max(r + 0.5, 0); 9 the depth value d = max(C0 f + 0.5, 0)
// (tsplat_raster_depth_bwd only, else 0); 10..15 padding
constexpr int kGradFields = 9;      // fields of the colour-only backward; field kGradFields is d's
constexpr int kAccStride = 12;      // floats per entry of a wave's LDS sums (up to 10 used)

// Data-parallel-primitive reads of another lane's value inside the VALU (no LDS crossbar trip, unlike
// __shfl_xor's ds_bpermute): a lane with no source lane reads 0. Controls: quad_perm [1, 0, 3, 2] and
// [2, 3, 0, 1] (lane ^ 1, lane ^ 2), row_shl:n (lane + n of the same 16-lane row).
constexpr int kDppQuadXor1 = 0xB1, kDppQuadXor2 = 0x4E, kDppRowShl4 = 0x104, kDppRowShl8 = 0x108;
template <int kCtrl>
__device__ __forceinline__ float dpp_f32(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xf, 0xf, true));
}

// --- B1: per-tile re-sort + front-to-back walk with the saved forward colour -------------------
// One workgroup per (tile, view), the forward's mapping. The tile list is re-sorted from the
// forward's workspace through the forward's own three paths (same functions, same total order on
// (depth bits, id)), and each wave walks it with the forward's cull, compaction and blend decisions
// (the same expressions under this file's contraction-off rule, so T, alpha and every branch are
// the forward's bit for bit; early exit included). Walk direction: FRONT TO BACK. With g the
// colour gradient at the pixel, O = out . g from the saved forward output (background term
// included) and S_i = O - sum_{j <= i} w_j (c_j . g) the part of O behind entry i,
//   dL/d alpha_i = T_i (c_i . g) - S_i / (1 - alpha_i),
// so neither a final T nor a contributor count is stored. S_i cancels for late entries: its
// absolute error is a few ulps of |O| while it is scaled by T_i <= 1 into the result, i.e. the
// error is relative to the largest terms of the pixel, not to the entry's own (small) gradient;
// the measured error (DESIGN.md 3 #3 "Backward") is far below the bar that would call for a
// back-to-front walk.
// Reduction: the 64 pixels of a wave are summed on chip before anything leaves the CU. A quad of
// 4 entries x 9 fields is reduced by a reduce-scatter (2 + 1 exchanges inside each lane quad fold the
// 4 entries onto lanes (l & 3), two row shifts sum a 16-lane row onto its lanes 0-3, all five as DPP
// reads inside the VALU, then two shuffles sum the four rows: 2 ds_bpermute per field per quad
// instead of 24), lanes 0-3 park the sums in the wave's LDS slot, and after the chunk the wave adds them to the
// gradient records: 16 lanes per record, 4 records per wave instruction (contiguous 36-byte
// segments of 64-byte records), at most one add per (wave, entry, field), none for an exact 0.
//
// <kColor, kExtra>, as the forward's: <true, false> is the colour-only backward of tsplat_raster_bwd.
// kExtra (tsplat_raster_depth_bwd): depth and alpha are two more blended channels over a zero
// background, the entry "colour" being (r, g, b, d, 1) and the pixel gradient (g0, g1, g2, gd, ga),
// so O gains out_depth gd + out_alpha ga, c_i . g gains d_i gd + ga (d from rec[3].w, one more
// compacted field; alpha's share of both is folded into one constant of S, see its load below), and
// there is one more sum, w gd, in field 9 of the gradient record: ten sums
// through the same reduce-scatter, 40 contiguous bytes per record. grad_depth / grad_alpha NULL read
// as zero (their saved outputs are not read). Without kColor (no colour gradient) the rgb fields,
// their three sums and the colour reads are gone: seven sums, fields 0-5 and 9.
template <bool kColor, bool kExtra>
__global__ void __launch_bounds__(kTileThreads)
render_bwd_kernel(Params p, const float* __restrict__ out_color, const float* __restrict__ grad_color,
                  float* __restrict__ grec, Workspace ws,
                  // kExtra only, and last: the colour-only instantiation's argument block is unchanged
                  const float* __restrict__ out_depth, const float* __restrict__ grad_depth,
                  const float* __restrict__ out_alpha, const float* __restrict__ grad_alpha) {
    constexpr int kRgbField = kGeomFields;                        // r g b (kColor)
    constexpr int kDepthField = kGeomFields + (kColor ? 3 : 0);   // d (kExtra)
    constexpr int kIdField = kDepthField + (kExtra ? 1 : 0);      // the entry's Gaussian id (bits)
    constexpr int kRecFields = kIdField + 1;                      // 10, 11 or 8
    constexpr int kSums = kGeomFields + (kColor ? 3 : 0) + (kExtra ? 1 : 0);  // 9, 10 or 7
    constexpr int kDepthSum = kSums - 1;                          // kExtra: the local index of sum w gd
    static_assert(kSums <= kAccStride && kGradFields + 1 <= kGradRecFloats, "sums fit their slots");
    __shared__ uint64_t skeys[kSortCap];
    __shared__ uint32_t s_cnt[kBuckets];
    __shared__ uint32_t s_red[4];
    __shared__ __attribute__((aligned(16))) float s_rec[kTileThreads / kWave][kRecFields][kWave];
    __shared__ __attribute__((aligned(16))) float s_acc[kTileThreads / kWave][kWave][kAccStride];

    const int v = blockIdx.y;
    int tile = xcd_remap(blockIdx.x, gridDim.x) + v * p.view_rot;
    tile %= p.T;
    const int tx = tile % p.tiles_x, ty = tile / p.tiles_x;
    const int t_idx = v * p.T + tile;
    uint32_t start = ws.offsets[t_idx];
    uint32_t end = ws.offsets[t_idx + 1];
    if (end > (uint32_t)p.capacity) end = (uint32_t)p.capacity;
    if (start > end) start = end;
    const int n = (int)(end - start);

    uint64_t* gkeys = ws.keys + start;
    const bool in_lds = n <= kSortCap;
    if (in_lds) {
        const bool try_count = p.count_sort && n > kTileThreads;
        const bool counted = try_count && counting_sort(gkeys, n, skeys, s_cnt, s_red);
        if (!counted) {
            for (int i = threadIdx.x; i < n; i += kTileThreads) skeys[i] = gkeys[i];
            __syncthreads();
            bitonic_sort_regs(skeys, n);
        }
    } else {
        bitonic_sort(gkeys, n);  // already sorted in place by the forward: the network leaves it as it is
    }
    // no workgroup barrier below this point

    const int wid = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int lx = (wid & 1) * 8 + (lane & 7), ly = (wid >> 1) * 8 + (lane >> 3);
    const int pxi = tx * kTile + lx, pyi = ty * kTile + ly;
    const float wx0 = (float)(tx * kTile + (wid & 1) * 8), wx1 = wx0 + 7.0f;
    const float wy0 = (float)(ty * kTile + (wid >> 1) * 8), wy1 = wy0 + 7.0f;
    const bool inside = pxi < p.W && pyi < p.H;
    bool done = !inside;
    const float pfx = (float)pxi, pfy = (float)pyi;
    float T = 1.0f;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    float gd = 0.f;  // kExtra
    float S = 0.f;  // out . g minus the entries walked so far
    if (inside) {
        const size_t hw = (size_t)p.H * p.W;
        if constexpr (kColor) {
            const size_t at = (size_t)v * 3 * hw + (size_t)pyi * p.W + pxi;
            g0 = grad_color[at];
            g1 = grad_color[at + hw];
            g2 = grad_color[at + 2 * hw];
            S = out_color[at] * g0 + out_color[at + hw] * g1 + out_color[at + 2 * hw] * g2;
        }
        if constexpr (kExtra) {
            const size_t at1 = (size_t)v * hw + (size_t)pyi * p.W + pxi;
            if (grad_depth) {
                gd = grad_depth[at1];
                S = S + out_depth[at1] * gd;
            }
            if (grad_alpha) {
                // alpha's channel value is 1 for every entry, so its part of S_i has a closed form:
                // ga sum_{j > i} w_j = ga (T_{i+1} - T_final), and T_i ga - ga (T_{i+1} - T_final) /
                // (1 - alpha_i) = ga T_final / (1 - alpha_i). S carries the constant -ga T_final and
                // c_i . g no ga term. Walked as a channel (S = out_alpha ga - sum w_j ga) every
                // alpha gradient is a difference of O(1) sums that leaves O(T_final): measured
                // e = 3.9e-4 on an alpha-only loss, against 1e-5 this way.
                const float ga = grad_alpha[at1];
                S = S - ga * (1.0f - out_alpha[at1]);
            }
        }
    }
    const size_t vbase = (size_t)v * p.G;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    float (*w_rec)[kWave] = s_rec[wid];
    float (*w_acc)[kAccStride] = s_acc[wid];
    const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0;
    const int my_e = (b0 ? 2 : 0) + (b1 ? 1 : 0);  // the quad entry whose sums this lane ends up with

    // one entry at this lane's pixel: the forward's blend() decisions, then the nine contributions
    auto entry = [&](float x, float y, float ca, float cb, float cc, float o, float r, float g, float bl,
                     float d, float (&val)[kSums]) {
        const float dx = x - pfx, dy = y - pfy;
        const float power2 = fmaf(dy, fmaf(cc, dy, cb * dx), (ca * dx) * dx);
        const float ex = __builtin_amdgcn_exp2f(power2);
        const float oe = o * ex;
        const float alpha = fminf(0.99f, oe);
        const float test_T = fmaf(-alpha, T, T);
        const bool contrib = !done && !(power2 > 0.0f) && !(alpha < 1.0f / 255.0f);
        const bool stop = contrib && (test_T < 0.0001f);
        const bool acc = contrib && !stop;
        const float w = acc ? alpha * T : 0.0f;
        float cg = 0.0f;
        if constexpr (kColor) cg = r * g0 + g * g1 + bl * g2;
        if constexpr (kExtra) cg = cg + d * gd;  // alpha's term: the constant in S
        S = fmaf(-w, cg, S);
        const float dalpha = acc ? T * cg - S * __builtin_amdgcn_rcpf(1.0f - alpha) : 0.0f;
        const bool pass = acc && !(oe > 0.99f);  // the 0.99 cap passes nothing to conic, mean, opacity
        const float gp = pass ? dalpha * alpha : 0.0f;  // dL/d power (natural log domain)
        constexpr float kLn2 = 0.69314718055994531f;
        const float gl = gp * kLn2;  // the stored conic carries log2(e)
        val[0] = gl * fmaf(2.0f * ca, dx, cb * dy);
        val[1] = gl * fmaf(2.0f * cc, dy, cb * dx);
        val[2] = gp * (-0.5f * dx * dx);
        val[3] = gp * (-dx * dy);
        val[4] = gp * (-0.5f * dy * dy);
        val[5] = pass ? dalpha * ex : 0.0f;
        if constexpr (kColor) {
            val[6] = w * g0;
            val[7] = w * g1;
            val[8] = w * g2;
        }
        if constexpr (kExtra) val[kDepthSum] = w * gd;
        T = acc ? test_T : T;
        done = done || stop;
    };

    const uint32_t* sids = reinterpret_cast<const uint32_t*>(skeys);
    auto walk = [&](auto lds_tag) {
        constexpr bool kInLds = decltype(lds_tag)::value;
        float4 r_xy = make_float4(0.f, 0.f, 0.f, 0.f), r_co = r_xy, r_rgb = r_xy, r_cull = r_xy;
        uint32_t r_gid = 0;
        bool r_valid = false;
        auto fetch = [&](int k) {
            r_valid = k < n;
            if (r_valid) {
                if constexpr (kInLds)
                    r_gid = sids[k];
                else
                    r_gid = (uint32_t)gkeys[k];
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
            bool hit = valid && !(xy.x + xy.z < wx0 || xy.x - xy.z > wx1 || xy.y + xy.w < wy0 ||
                                  xy.y - xy.w > wy1);
            if (hit) hit = ellipse_meets_block(xy.x, xy.y, co, cull, wx0, wx1, wy0, wy1);
            const uint64_t mask = __ballot(hit);
            const int m = __popcll(mask);
            const int m4 = (m + 3) & ~3;
            if (hit) {
                const int pos = __popcll(mask & lt_mask);
                w_rec[0][pos] = xy.x;
                w_rec[1][pos] = xy.y;
                w_rec[2][pos] = co.x;
                w_rec[3][pos] = co.y;
                w_rec[4][pos] = co.z;
                w_rec[5][pos] = co.w;
                if constexpr (kColor) {
                    w_rec[kRgbField][pos] = rgb.x;
                    w_rec[kRgbField + 1][pos] = rgb.y;
                    w_rec[kRgbField + 2][pos] = rgb.z;
                }
                if constexpr (kExtra) w_rec[kDepthField][pos] = cull.w;
                w_rec[kIdField][pos] = __uint_as_float(gid);
            }
            // pad the last quad with entries that contribute nothing (opacity 0: alpha < 1/255)
            if (lane < m4 - m) {
#pragma unroll
                for (int f = 0; f < kRecFields; ++f) w_rec[f][m + lane] = 0.0f;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int i = 0; i < m4; i += 4) {
                float4 q[kIdField];
#pragma unroll
                for (int f = 0; f < kIdField; ++f) q[f] = *reinterpret_cast<const float4*>(&w_rec[f][i]);
                float va[4][kSums];
                // fields an instantiation does not carry are read from field 0 and never used
                constexpr int iR = kColor ? kRgbField : 0, iG = kColor ? kRgbField + 1 : 0,
                              iB = kColor ? kRgbField + 2 : 0, iD = kExtra ? kDepthField : 0;
                entry(q[0].x, q[1].x, q[2].x, q[3].x, q[4].x, q[5].x, q[iR].x, q[iG].x, q[iB].x, q[iD].x, va[0]);
                entry(q[0].y, q[1].y, q[2].y, q[3].y, q[4].y, q[5].y, q[iR].y, q[iG].y, q[iB].y, q[iD].y, va[1]);
                entry(q[0].z, q[1].z, q[2].z, q[3].z, q[4].z, q[5].z, q[iR].z, q[iG].z, q[iB].z, q[iD].z, va[2]);
                entry(q[0].w, q[1].w, q[2].w, q[3].w, q[4].w, q[5].w, q[iR].w, q[iG].w, q[iB].w, q[iD].w, va[3]);
                // reduce-scatter: lanes with bit 0 clear keep entries {0, 1}, the others {2, 3};
                // then bit 1 picks one of the pair; then the 16 lane quads are summed onto lanes 0-3
                float tot[kSums];
#pragma unroll
                for (int f = 0; f < kSums; ++f) {
                    const float keep0 = b0 ? va[2][f] : va[0][f], keep1 = b0 ? va[3][f] : va[1][f];
                    const float send0 = b0 ? va[0][f] : va[2][f], send1 = b0 ? va[1][f] : va[3][f];
                    const float u0 = keep0 + dpp_f32<kDppQuadXor1>(send0);
                    const float u1 = keep1 + dpp_f32<kDppQuadXor1>(send1);
                    float t = (b1 ? u1 : u0) + dpp_f32<kDppQuadXor2>(b1 ? u0 : u1);
                    t += dpp_f32<kDppRowShl4>(t);  // lanes 0-11 of a 16-lane row: + lane l + 4
                    t += dpp_f32<kDppRowShl8>(t);  // lanes 0-3 of a row: the row's four quads
                    t += __shfl_xor(t, 16);
                    t += __shfl_xor(t, 32);        // lanes 0-3: all four rows
                    tot[f] = t;
                }
                if (lane < 4) {
                    float* a = w_acc[i + my_e];
                    *reinterpret_cast<float4*>(a) = make_float4(tot[0], tot[1], tot[2], tot[3]);
                    if constexpr (kColor) {
                        *reinterpret_cast<float4*>(a + 4) = make_float4(tot[4], tot[5], tot[6], tot[7]);
                        if constexpr (kExtra)
                            *reinterpret_cast<float2*>(a + 8) = make_float2(tot[8], tot[9]);
                        else
                            a[8] = tot[8];
                    } else {
                        *reinterpret_cast<float4*>(a + 4) = make_float4(tot[4], tot[5], tot[6], 0.0f);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // the chunk's sums to the gradient records: 16 lanes per record, 4 records per instruction
            {
                const int f = lane & 15;
                for (int j = 0; j < m; j += 4) {
                    const int e = j + (lane >> 4);
                    if (e < m && f < kSums) {
                        const float val = w_acc[e][f];
                        const uint32_t id = __float_as_uint(w_rec[kIdField][e]);
                        // the record's field: the local sum's own index, but for the depth sum without colour
                        const int rf = (!kColor && f == kDepthSum) ? kGradFields : f;
                        if (val != 0.0f) atomicAdd(grec + (vbase + id) * kGradRecFloats + rf, val);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();  // reads of this chunk's LDS slots precede the next writes
        }
    };
    if (in_lds)
        walk(std::true_type{});
    else
        walk(std::false_type{});
}

// --- B2: gradient records -> gradients of the Gaussians ----------------------------------------
// One thread per Gaussian for all views of its scene (blockIdx.y = scene), the mirror of
// preprocess_kernel: the forward geometry of each view is recomputed with the forward's
// expressions, the view's gradient record is chained through them, and the contributions of the
// views are summed in registers (SH: in the thread's LDS slot) and written once. No atomics. Views
// with radii == 0 are skipped. The SH block of a wave's 64 Gaussians is staged to LDS and its
// gradient written back by coalesced loops, as the forward reads it. 128 threads per workgroup:
// two [threads][75] float LDS arrays (coefficients and their gradients), 76,800 bytes.
constexpr int kPreBwdThreads = 128;

// The derivative f'(z) of the fake colour behind depth_value(), times C0, where the clamp of
// d = max(C0 f + 0.5, 0) is open; 0 where it is active (C0 f + 0.5 <= 0). z = vz / s, the forward's
// expression. "log": f = log(max(min(z, near), far)) follows z only where far < z < near strictly.
__device__ __forceinline__ float depth_value_dz(int mode, float vz, float s, float near, float far) {
    const float z = vz / s;
    float f = z, df = 1.0f;
    if (mode == 1) {
        f = 1.0f / z;
        df = -1.0f / (z * z);
    } else if (mode == 2) {
        const float eps = 1e-10f;
        const float disp_near = 1.0f / (near + eps), disp_far = 1.0f / (far + eps);
        const float den = disp_near - disp_far + eps;
        f = 1.0f - (1.0f / (z + eps) - disp_far) / den;
        df = 1.0f / ((z + eps) * (z + eps)) / den;
    } else if (mode == 3) {
        f = logf(fmaxf(fminf(z, near), far));
        df = (z > far && z < near) ? 1.0f / z : 0.0f;
    }
    return kSH_C0 * f + 0.5f > 0.0f ? kSH_C0 * df : 0.0f;
}

// <kColor, kExtra>, as render_bwd_kernel's: <true, false> is tsplat_raster_bwd's. kExtra chains field
// 9 of the record (sum w gd) through the depth value into d vz, when p.depth_mode >= 0. Without kColor
// the SH block is neither staged nor evaluated, the view direction has no part in d means, and
// grad_shs is written as zeros.
template <bool kColor, bool kExtra>
__global__ void __launch_bounds__(kPreBwdThreads)
preprocess_bwd_kernel(Params p, const float* __restrict__ means, const float* __restrict__ cov,
                      const float* __restrict__ shs, const float* __restrict__ opacity,
                      const float* __restrict__ viewmat, const float* __restrict__ projmat,
                      const float* __restrict__ campos, const float* __restrict__ tanfov,
                      const float* __restrict__ scene_scale, const int32_t* __restrict__ radii,
                      const float* __restrict__ grec, float* __restrict__ grad_means,
                      float* __restrict__ grad_cov, float* __restrict__ grad_shs,
                      float* __restrict__ grad_opacity,
                      // kExtra only, and last: the colour-only instantiation's argument block is unchanged
                      const float* __restrict__ near, const float* __restrict__ far) {
    __shared__ float s_sh[kColor ? kPreBwdThreads * kMaxShFloats : 1];
    __shared__ float s_dsh[kColor ? kPreBwdThreads * kMaxShFloats : 1];
    const int scene = blockIdx.y;
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const int g = blockIdx.x * kPreBwdThreads + threadIdx.x;
    const int nf = 3 * p.M;
    const size_t sg = (size_t)scene * p.G + g;
    const float* my_sh = s_sh + (size_t)threadIdx.x * nf;
    float* my_dsh = s_dsh + (size_t)threadIdx.x * nf;
    const int gw0 = blockIdx.x * kPreBwdThreads + wid * kWave;
    const int sh_total = max(0, min(kWave, p.G - gw0)) * nf;
    const size_t sh_off = (size_t)nf * ((size_t)scene * p.G + gw0);
    if constexpr (kColor) {
        const float* sh_src = shs + sh_off;
        float* sh_dst = s_sh + (size_t)wid * kWave * nf;
        float* dsh_dst = s_dsh + (size_t)wid * kWave * nf;
        for (int i = lane; i < sh_total; i += kWave) {
            sh_dst[i] = sh_src[i];
            dsh_dst[i] = 0.0f;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    if (g < p.G) {
        const float m0 = means[3 * sg], m1 = means[3 * sg + 1], m2 = means[3 * sg + 2];
        const float* C = cov + 9 * sg;
        const float k00 = C[0], k01 = C[1], k02 = C[2], k11 = C[4], k12 = C[5], k22 = C[8];
        float gm0 = 0.f, gm1 = 0.f, gm2 = 0.f, go = 0.f;
        float gk00 = 0.f, gk01 = 0.f, gk02 = 0.f, gk11 = 0.f, gk12 = 0.f, gk22 = 0.f;
        const int nb = (p.deg + 1) * (p.deg + 1);  // SH coefficients evaluated per channel
        for (int vv = 0; vv < p.vps; ++vv) {
            const int v = scene * p.vps + vv;
            const size_t vg = (size_t)v * p.G + g;
            if (radii[vg] == 0) continue;
            const float4* gr = reinterpret_cast<const float4*>(grec + kGradRecFloats * vg);
            const float4 ga = gr[0], gb = gr[1];
            const float g_r2 = gr[2].x;
            const float g_px = ga.x, g_py = ga.y, g_qa = ga.z, g_qb = ga.w, g_qc = gb.x, g_o = gb.y;
            const float g_rgb[3] = {gb.z, gb.w, g_r2};
            go += g_o;

            const float* vm = viewmat + 16 * v;
            const float* pm = projmat + 16 * v;
            const float s = scene_scale[2 * v], s2 = scene_scale[2 * v + 1];
            // forward geometry, the expressions of preprocess_kernel
            const float mx = m0 * s, my = m1 * s, mz = m2 * s;
            const float vx = vm[0] * mx + vm[4] * my + vm[8] * mz + vm[12];
            const float vy = vm[1] * mx + vm[5] * my + vm[9] * mz + vm[13];
            const float vz = vm[2] * mx + vm[6] * my + vm[10] * mz + vm[14];
            const float hx = pm[0] * mx + pm[4] * my + pm[8] * mz + pm[12];
            const float hy = pm[1] * mx + pm[5] * my + pm[9] * mz + pm[13];
            const float hw = pm[3] * mx + pm[7] * my + pm[11] * mz + pm[15];
            const float pw = 1.0f / (hw + 0.0000001f);
            const float c00 = k00 * s2, c01 = k01 * s2, c02 = k02 * s2;
            const float c11 = k11 * s2, c12 = k12 * s2, c22 = k22 * s2;
            const float tfx = tanfov[2 * v], tfy = tanfov[2 * v + 1];
            const float fx = (float)p.W / (2.0f * tfx), fy = (float)p.H / (2.0f * tfy);
            const float limx = 1.3f * tfx, limy = 1.3f * tfy;
            const float tz = vz;
            const float rxu = vx / tz, ryu = vy / tz;
            const float rx = fminf(limx, fmaxf(-limx, rxu)), ry = fminf(limy, fmaxf(-limy, ryu));
            const bool in_x = rxu >= -limx && rxu <= limx, in_y = ryu >= -limy && ryu <= limy;
            const float tx = rx * tz, ty = ry * tz;
            const float j00 = fx / tz, j02 = -(fx * tx) / (tz * tz);
            const float j11 = fy / tz, j12 = -(fy * ty) / (tz * tz);
            const float n00 = j00 * vm[0] + j02 * vm[2];
            const float n01 = j00 * vm[4] + j02 * vm[6];
            const float n02 = j00 * vm[8] + j02 * vm[10];
            const float n10 = j11 * vm[1] + j12 * vm[2];
            const float n11 = j11 * vm[5] + j12 * vm[6];
            const float n12 = j11 * vm[9] + j12 * vm[10];
            const float u00 = n00 * c00 + n01 * c01 + n02 * c02;
            const float u01 = n00 * c01 + n01 * c11 + n02 * c12;
            const float u02 = n00 * c02 + n01 * c12 + n02 * c22;
            const float u10 = n10 * c00 + n11 * c01 + n12 * c02;
            const float u11 = n10 * c01 + n11 * c11 + n12 * c12;
            const float u12 = n10 * c02 + n11 * c12 + n12 * c22;
            const float a = u00 * n00 + u01 * n01 + u02 * n02 + 0.3f;
            const float b = u00 * n10 + u01 * n11 + u02 * n12;
            const float c = u10 * n10 + u11 * n11 + u12 * n12 + 0.3f;
            const float det = a * c - b * b;
            const float det_inv = 1.0f / det;
            const float qa = c * det_inv, qb = -b * det_inv, qc = a * det_inv;

            // conic Q = Sigma2^-1: dL/dSigma2 = -Q G Q with G = [[g_qa, g_qb / 2], [g_qb / 2, g_qc]]
            const float hb = 0.5f * g_qb;
            const float t00 = qa * g_qa + qb * hb, t01 = qa * hb + qb * g_qc;
            const float t10 = qb * g_qa + qc * hb, t11 = qb * hb + qc * g_qc;
            const float dA = -(t00 * qa + t01 * qb);
            const float dB = -2.0f * (t00 * qb + t01 * qc);  // b sits in both off-diagonal entries
            const float dC = -(t10 * qb + t11 * qc);
            // a = n0' C n0 + 0.3, b = n0' C n1, c = n1' C n1 + 0.3 (C = s^2 K, the upper triangle of K read)
            gk00 += s2 * (dA * n00 * n00 + dB * n00 * n10 + dC * n10 * n10);
            gk01 += s2 * (2.0f * dA * n00 * n01 + dB * (n00 * n11 + n01 * n10) + 2.0f * dC * n10 * n11);
            gk02 += s2 * (2.0f * dA * n00 * n02 + dB * (n00 * n12 + n02 * n10) + 2.0f * dC * n10 * n12);
            gk11 += s2 * (dA * n01 * n01 + dB * n01 * n11 + dC * n11 * n11);
            gk12 += s2 * (2.0f * dA * n01 * n02 + dB * (n01 * n12 + n02 * n11) + 2.0f * dC * n11 * n12);
            gk22 += s2 * (dA * n02 * n02 + dB * n02 * n12 + dC * n12 * n12);
            const float dn00 = 2.0f * dA * u00 + dB * u10, dn01 = 2.0f * dA * u01 + dB * u11,
                        dn02 = 2.0f * dA * u02 + dB * u12;
            const float dn10 = 2.0f * dC * u10 + dB * u00, dn11 = 2.0f * dC * u11 + dB * u01,
                        dn12 = 2.0f * dC * u12 + dB * u02;
            const float dj00 = dn00 * vm[0] + dn01 * vm[4] + dn02 * vm[8];
            const float dj02 = dn00 * vm[2] + dn01 * vm[6] + dn02 * vm[10];
            const float dj11 = dn10 * vm[1] + dn11 * vm[5] + dn12 * vm[9];
            const float dj12 = dn10 * vm[2] + dn11 * vm[6] + dn12 * vm[10];
            // j00 = fx / tz, j02 = -fx r / tz with r = clamp(vx / tz): inside the clamp r follows vx and
            // tz, at the clamp it is a constant
            const float itz = 1.0f / tz, itz2 = itz * itz;
            const float dvx = in_x ? -dj02 * fx * itz2 : 0.0f;
            const float dvy = in_y ? -dj12 * fy * itz2 : 0.0f;
            float dvz = -(dj00 * fx + dj11 * fy) * itz2 +
                        dj02 * (fx * rx * itz2 + (in_x ? fx * vx * itz2 * itz : 0.0f)) +
                        dj12 * (fy * ry * itz2 + (in_y ? fy * vy * itz2 * itz : 0.0f));
            if constexpr (kExtra) {
                // the depth value d = max(C0 f(vz / s) + 0.5, 0): field 9 of the record is dL/dd
                const float g_d = gr[2].y;
                if (p.depth_mode >= 0 && g_d != 0.0f)
                    dvz = dvz + g_d * depth_value_dz(p.depth_mode, vz, s, near[v], far[v]) / s;
            }
            float dmx = vm[0] * dvx + vm[1] * dvy + vm[2] * dvz;
            float dmy = vm[4] * dvx + vm[5] * dvy + vm[6] * dvz;
            float dmz = vm[8] * dvx + vm[9] * dvy + vm[10] * dvz;
            // pixel mean: px = ((hx pw + 1) W - 1) / 2, pw = 1 / (hw + 1e-7)
            const float dndx = g_px * 0.5f * (float)p.W, dndy = g_py * 0.5f * (float)p.H;
            const float dhx = dndx * pw, dhy = dndy * pw;
            const float dhw = -(dndx * hx + dndy * hy) * pw * pw;
            dmx += pm[0] * dhx + pm[1] * dhy + pm[3] * dhw;
            dmy += pm[4] * dhx + pm[5] * dhy + pm[7] * dhw;
            dmz += pm[8] * dhx + pm[9] * dhy + pm[11] * dhw;

            if constexpr (kColor) {
                // colour: rgb_c = max(sum_k B_k(n) sh[c][k] + 0.5, 0), n = d / |d|, d = mean s - campos
                const float* cp = campos + 3 * v;
                const float ddx = mx - cp[0], ddy = my - cp[1], ddz = mz - cp[2];
                float rgb[3];
                sh_to_rgb(my_sh, p.M, p.deg, ddx, ddy, ddz, rgb);
                float tc[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) tc[ch] = rgb[ch] > 0.0f ? g_rgb[ch] : 0.0f;  // the clamp at 0
                const float len = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);
                const float x = ddx / len, y = ddy / len, z = ddz / len;
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                float dnx = 0.f, dny = 0.f, dnz = 0.f;
                // one basis function: value B and its gradient (bx, by, bz) in the unit direction
                auto term = [&](int k, float B, float bx, float by, float bz) {
                    const float ak = tc[0] * my_sh[k] + tc[1] * my_sh[p.M + k] + tc[2] * my_sh[2 * p.M + k];
                    dnx += bx * ak;
                    dny += by * ak;
                    dnz += bz * ak;
                    my_dsh[k] += tc[0] * B;
                    my_dsh[p.M + k] += tc[1] * B;
                    my_dsh[2 * p.M + k] += tc[2] * B;
                };
                term(0, kSH_C0, 0.f, 0.f, 0.f);
                if (nb > 1) {
                    term(1, -kSH_C1 * y, 0.f, -kSH_C1, 0.f);
                    term(2, kSH_C1 * z, 0.f, 0.f, kSH_C1);
                    term(3, -kSH_C1 * x, -kSH_C1, 0.f, 0.f);
                }
                if (nb > 4) {
                    term(4, kSH_C2[0] * xy, kSH_C2[0] * y, kSH_C2[0] * x, 0.f);
                    term(5, kSH_C2[1] * yz, 0.f, kSH_C2[1] * z, kSH_C2[1] * y);
                    term(6, kSH_C2[2] * (2.0f * zz - xx - yy), kSH_C2[2] * -2.0f * x, kSH_C2[2] * -2.0f * y,
                         kSH_C2[2] * 4.0f * z);
                    term(7, kSH_C2[3] * xz, kSH_C2[3] * z, 0.f, kSH_C2[3] * x);
                    term(8, kSH_C2[4] * (xx - yy), kSH_C2[4] * 2.0f * x, kSH_C2[4] * -2.0f * y, 0.f);
                }
                if (nb > 9) {
                    term(9, kSH_C3[0] * y * (3.0f * xx - yy), kSH_C3[0] * 6.0f * xy, kSH_C3[0] * (3.0f * xx - 3.0f * yy), 0.f);
                    term(10, kSH_C3[1] * xy * z, kSH_C3[1] * yz, kSH_C3[1] * xz, kSH_C3[1] * xy);
                    term(11, kSH_C3[2] * y * (4.0f * zz - xx - yy), kSH_C3[2] * -2.0f * xy,
                         kSH_C3[2] * (4.0f * zz - xx - 3.0f * yy), kSH_C3[2] * 8.0f * yz);
                    term(12, kSH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy), kSH_C3[3] * -6.0f * xz,
                         kSH_C3[3] * -6.0f * yz, kSH_C3[3] * (6.0f * zz - 3.0f * xx - 3.0f * yy));
                    term(13, kSH_C3[4] * x * (4.0f * zz - xx - yy), kSH_C3[4] * (4.0f * zz - 3.0f * xx - yy),
                         kSH_C3[4] * -2.0f * xy, kSH_C3[4] * 8.0f * xz);
                    term(14, kSH_C3[5] * z * (xx - yy), kSH_C3[5] * 2.0f * xz, kSH_C3[5] * -2.0f * yz,
                         kSH_C3[5] * (xx - yy));
                    term(15, kSH_C3[6] * x * (xx - 3.0f * yy), kSH_C3[6] * (3.0f * xx - 3.0f * yy), kSH_C3[6] * -6.0f * xy,
                         0.f);
                }
                if (nb > 16) {
                    const float s7 = 7.0f * zz - 1.0f, t7 = 7.0f * zz - 3.0f;
                    term(16, kSH_C4[0] * xy * (xx - yy), kSH_C4[0] * y * (3.0f * xx - yy), kSH_C4[0] * x * (xx - 3.0f * yy),
                         0.f);
                    term(17, kSH_C4[1] * yz * (3.0f * xx - yy), kSH_C4[1] * 6.0f * xy * z,
                         kSH_C4[1] * z * (3.0f * xx - 3.0f * yy), kSH_C4[1] * y * (3.0f * xx - yy));
                    term(18, kSH_C4[2] * xy * s7, kSH_C4[2] * y * s7, kSH_C4[2] * x * s7, kSH_C4[2] * 14.0f * xy * z);
                    term(19, kSH_C4[3] * yz * t7, 0.f, kSH_C4[3] * z * t7, kSH_C4[3] * y * (21.0f * zz - 3.0f));
                    term(20, kSH_C4[4] * (zz * (35.0f * zz - 30.0f) + 3.0f), 0.f, 0.f,
                         kSH_C4[4] * z * (140.0f * zz - 60.0f));
                    term(21, kSH_C4[5] * xz * t7, kSH_C4[5] * z * t7, 0.f, kSH_C4[5] * x * (21.0f * zz - 3.0f));
                    term(22, kSH_C4[6] * (xx - yy) * s7, kSH_C4[6] * 2.0f * x * s7, kSH_C4[6] * -2.0f * y * s7,
                         kSH_C4[6] * 14.0f * z * (xx - yy));
                    term(23, kSH_C4[7] * xz * (xx - 3.0f * yy), kSH_C4[7] * z * (3.0f * xx - 3.0f * yy),
                         kSH_C4[7] * -6.0f * xy * z, kSH_C4[7] * x * (xx - 3.0f * yy));
                    term(24, kSH_C4[8] * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy)),
                         kSH_C4[8] * x * (4.0f * xx - 12.0f * yy), kSH_C4[8] * y * (4.0f * yy - 12.0f * xx), 0.f);
                }
                // through n = d / |d|: dL/dd = (dn - n (n . dn)) / |d|
                const float ndot = x * dnx + y * dny + z * dnz;
                dmx += (dnx - x * ndot) / len;
                dmy += (dny - y * ndot) / len;
                dmz += (dnz - z * ndot) / len;
            }
            // scale-invariant rendering: mean s (cov s^2 is in gk above)
            gm0 += s * dmx;
            gm1 += s * dmy;
            gm2 += s * dmz;
        }
        if (grad_means) {
            grad_means[3 * sg] = gm0;
            grad_means[3 * sg + 1] = gm1;
            grad_means[3 * sg + 2] = gm2;
        }
        if (grad_cov) {
            float* o = grad_cov + 9 * sg;
            o[0] = gk00;
            o[1] = gk01;
            o[2] = gk02;
            o[3] = 0.0f;
            o[4] = gk11;
            o[5] = gk12;
            o[6] = 0.0f;
            o[7] = 0.0f;
            o[8] = gk22;
        }
        if (grad_opacity) grad_opacity[sg] = go;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (grad_shs) {
        float* dst = grad_shs + sh_off;
        if constexpr (kColor) {
            const float* src = s_dsh + (size_t)wid * kWave * nf;
            for (int i = lane; i < sh_total; i += kWave) dst[i] = src[i];
        } else {
            for (int i = lane; i < sh_total; i += kWave) dst[i] = 0.0f;
        }
    }
}

}  // namespace raster
}  // namespace tsplat

using namespace tsplat;
using namespace tsplat::raster;

extern "C" size_t tsplat_raster_workspace_bytes(int32_t G, int32_t V, int32_t H, int32_t W,
                                                int32_t capacity) {
    const int T = ceil_div(W, kTile) * ceil_div(H, kTile);
    size_t total = 0;
    carve(nullptr, G, V, T, capacity, &total);
    return total;
}

extern "C" size_t tsplat_raster_num_rendered_offset(int32_t G, int32_t V, int32_t H, int32_t W) {
    const int T = ceil_div(W, kTile) * ceil_div(H, kTile);
    const Workspace w = carve((void*)(uintptr_t)0x100000, G, V, T, 1, nullptr);  // layout only
    return (size_t)((char*)(w.offsets + (size_t)V * T) - (char*)(uintptr_t)0x100000);
}

// The launch sequence of both entry points. kColor / kExtra pick the preprocess and render
// instantiations: <true, false> is tsplat_raster_fwd; tsplat_raster_depth_fwd takes <true, true>
// with a colour output and <false, true> without one.
template <bool kColor, bool kExtra>
static int raster_launch(Params p, const float* means, const float* cov, const float* shs,
                         const float* opacity, const float* viewmat, const float* projmat,
                         const float* campos, const float* tanfov, const float* bg,
                         const float* scene_scale, const float* near, const float* far,
                         float* out_color, float* out_depth, float* out_alpha, int32_t* out_radii,
                         Workspace ws, int32_t* status, hipStream_t stream) {
    TSPLAT_PROF_BEGIN(prof::kRasterAll, stream);
    {
        // counts + cursor: 2 V T uint32, padded by carve()'s 256-byte alignment to whole uint4s
        const size_t n4 = ceil_div((size_t)2 * p.V * p.T, (size_t)4);
        const int blocks = (int)std::min<size_t>(ceil_div(n4, (size_t)256), 1024);
        hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, stream, (uint4*)ws.counts, n4);
        TSPLAT_CHECK_LAUNCH();
    }
    const int scenes = p.V / p.vps;
    dim3 pre_grid(ceil_div(p.G, kPreThreads), p.V);
    TSPLAT_PROF_BEGIN(prof::kRasterPreprocess, stream);
    hipLaunchKernelGGL((preprocess_kernel<kColor, kExtra>), dim3(ceil_div(p.G, kPreThreads), scenes),
                       dim3(kPreThreads), p.T * sizeof(uint32_t),
                       stream, p, means, cov, shs, opacity, viewmat, projmat, campos, tanfov,
                       scene_scale, near, far, out_radii, ws);
    TSPLAT_PROF_END(prof::kRasterPreprocess, stream);
    TSPLAT_CHECK_LAUNCH();
    TSPLAT_PROF_BEGIN(prof::kRasterScatter, stream);
    hipLaunchKernelGGL(scatter_kernel, pre_grid, dim3(kPreThreads), 3 * p.T * sizeof(uint32_t),
                       stream, p, (const int32_t*)out_radii, ws, status);
    TSPLAT_PROF_END(prof::kRasterScatter, stream);
    TSPLAT_CHECK_LAUNCH();
    TSPLAT_PROF_BEGIN(prof::kRasterRender, stream);
    hipLaunchKernelGGL((render_kernel<kColor, kExtra>), dim3(p.T, p.V), dim3(kTileThreads), 0, stream, p,
                       bg, out_color, out_depth, out_alpha, ws);
    TSPLAT_PROF_END(prof::kRasterRender, stream);
    TSPLAT_PROF_END(prof::kRasterAll, stream);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

// Descriptor checks and launch parameters of every rasterizer entry point, forward and backward
// (sh_vec4 is the forward's own, set by raster_run). False: the descriptor is rejected.
static bool raster_params(const tsplat_raster_desc* d, int depth_mode, Params* out) {
    if (d->num_gaussians <= 0 || d->num_views <= 0 || d->views_per_scene <= 0 ||
        d->num_views % d->views_per_scene != 0 || d->height <= 0 || d->width <= 0 ||
        d->sh_coeffs <= 0 || d->sh_degree < 0 || d->sh_degree > 4 ||
        (d->sh_degree + 1) * (d->sh_degree + 1) > d->sh_coeffs || d->capacity <= 0)
        return false;
    Params p;
    p.G = d->num_gaussians;
    p.V = d->num_views;
    p.vps = d->views_per_scene;
    p.H = d->height;
    p.W = d->width;
    p.M = d->sh_coeffs;
    p.deg = d->sh_degree;
    p.tiles_x = ceil_div(p.W, kTile);
    p.tiles_y = ceil_div(p.H, kTile);
    p.T = p.tiles_x * p.tiles_y;
    p.capacity = d->capacity;
    p.depth_mode = depth_mode;
    p.sh_vec4 = 0;
    {
        const char* e = getenv("TSPLAT_RASTER_DIAG");
        p.diag = e ? atoi(e) : 0;
        const char* s = getenv("TSPLAT_RASTER_SORT");
        p.count_sort = !(s && !strcmp(s, "bitonic"));
        // rotation per view: about T / 3 tiles, rounded to whole rows
        p.view_rot = (p.tiles_y + 1) / 3 * p.tiles_x;
    }
    if (3 * p.M > kMaxShFloats || p.vps > 32) return false;
    // scatter keeps 3 T uint32 of per-tile counters in LDS: up to gfx950's 160 KB per workgroup
    // (13,653 16x16 tiles, about 1860 x 1860 px)
    if ((size_t)p.T * 3 * sizeof(uint32_t) > kMaxLdsBytes) return false;
    *out = p;
    return true;
}

// Argument checks and launch parameters shared by tsplat_raster_fwd (depth_mode = -1, no extra
// outputs) and tsplat_raster_depth_fwd. Every check comes before the first launch: a rejected call
// queues nothing.
static int raster_run(const tsplat_raster_desc* d, const float* means, const float* cov,
                      const float* shs, const float* opacity, const float* viewmat,
                      const float* projmat, const float* campos, const float* tanfov,
                      const float* bg, const float* scene_scale, const float* near, const float* far,
                      int depth_mode, bool extra, float* out_color, float* out_depth,
                      float* out_alpha, int32_t* out_radii, void* workspace, int32_t* status,
                      void* stream_) {
    if (!d || !means || !cov || !shs || !opacity || !viewmat || !projmat || !campos || !tanfov ||
        !bg || !scene_scale || !out_radii || !workspace || !status)
        return TSPLAT_EINVAL;
    if (!out_color && !out_depth && !out_alpha) return TSPLAT_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    Params p;
    if (!raster_params(d, depth_mode, &p)) return TSPLAT_EINVAL;
    // scatter keeps 3 T uint32 of per-tile counters in LDS: above 64 KB the kernel's dynamic-LDS limit is raised
    const size_t scatter_lds = (size_t)p.T * 3 * sizeof(uint32_t);
    if (scatter_lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&scatter_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)scatter_lds) != hipSuccess)
        return TSPLAT_EINVAL;
    Workspace ws = carve(workspace, p.G, p.V, p.T, p.capacity, nullptr);
    // a wave's SH block starts at 3 M (scene G + 64 k) floats: 16-byte aligned when the base is
    // and 3 M G is a multiple of 4 (or there is one scene)
    const int scenes = p.V / p.vps;
    p.sh_vec4 = ((uintptr_t)shs % 16 == 0) && (scenes == 1 || ((size_t)3 * p.M * p.G) % 4 == 0);
#define TSPLAT_RASTER_ARGS                                                                          \
    p, means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale, near, far,     \
        out_color, out_depth, out_alpha, out_radii, ws, status, stream
    if (!extra) return raster_launch<true, false>(TSPLAT_RASTER_ARGS);
    if (out_color) return raster_launch<true, true>(TSPLAT_RASTER_ARGS);
    return raster_launch<false, true>(TSPLAT_RASTER_ARGS);
#undef TSPLAT_RASTER_ARGS
}

extern "C" int tsplat_raster_fwd(const tsplat_raster_desc* d, const float* means, const float* cov,
                                 const float* shs, const float* opacity, const float* viewmat,
                                 const float* projmat, const float* campos, const float* tanfov,
                                 const float* bg, const float* scene_scale, float* out_color,
                                 int32_t* out_radii, void* workspace, int32_t* status,
                                 void* stream_) {
    if (!out_color) return TSPLAT_EINVAL;
    return raster_run(d, means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale,
                      nullptr, nullptr, -1, false, out_color, nullptr, nullptr, out_radii, workspace,
                      status, stream_);
}

extern "C" int tsplat_raster_depth_fwd(const tsplat_raster_desc* d, const float* means,
                                       const float* cov, const float* shs, const float* opacity,
                                       const float* viewmat, const float* projmat,
                                       const float* campos, const float* tanfov, const float* bg,
                                       const float* scene_scale, const float* near, const float* far,
                                       int32_t depth_mode, float* out_color, float* out_depth,
                                       float* out_alpha, int32_t* out_radii, void* workspace,
                                       int32_t* status, void* stream_) {
    if (depth_mode < 0 || depth_mode > 3) return TSPLAT_EINVAL;
    if (out_depth && (!near || !far)) return TSPLAT_EINVAL;
    return raster_run(d, means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale,
                      near, far, out_depth ? depth_mode : -1, true, out_color, out_depth, out_alpha,
                      out_radii, workspace, status, stream_);
}

extern "C" size_t tsplat_raster_bwd_workspace_bytes(int32_t G, int32_t V) {
    if (G <= 0 || V <= 0) return 0;
    return align_up((size_t)G * V * kGradRecFloats * sizeof(float), 256);
}

// The launch sequence of both backward entry points: zero fill of the gradient records,
// render_bwd_kernel, preprocess_bwd_kernel, in the <kColor, kExtra> instantiations. <true, false> is
// tsplat_raster_bwd's, and tsplat_raster_depth_bwd's with a colour gradient alone; <true, true> adds a
// depth and / or alpha gradient to the colour's; <false, true> runs without a colour gradient.
template <bool kColor, bool kExtra>
static int raster_bwd_launch(Params p, const float* means, const float* cov, const float* shs,
                             const float* opacity, const float* viewmat, const float* projmat,
                             const float* campos, const float* tanfov, const float* scene_scale,
                             const float* near, const float* far, const float* out_color,
                             const float* grad_color, const float* out_depth, const float* grad_depth,
                             const float* out_alpha, const float* grad_alpha, const int32_t* radii,
                             Workspace ws, float* grec, float* grad_means, float* grad_cov,
                             float* grad_shs, float* grad_opacity, hipStream_t stream) {
    TSPLAT_PROF_BEGIN(prof::kRasterBwdAll, stream);
    {
        const size_t n4 = (size_t)p.G * p.V * kGradRecFloats / 4;
        const int blocks = (int)std::min<size_t>(ceil_div(n4, (size_t)256), 4096);
        hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, stream, (uint4*)grec, n4);
        TSPLAT_CHECK_LAUNCH();
    }
    TSPLAT_PROF_BEGIN(prof::kRasterBwdRender, stream);
    hipLaunchKernelGGL((render_bwd_kernel<kColor, kExtra>), dim3(p.T, p.V), dim3(kTileThreads), 0, stream,
                       p, out_color, grad_color, grec, ws, out_depth, grad_depth, out_alpha, grad_alpha);
    TSPLAT_PROF_END(prof::kRasterBwdRender, stream);
    TSPLAT_CHECK_LAUNCH();
    const int scenes = p.V / p.vps;
    TSPLAT_PROF_BEGIN(prof::kRasterBwdPreprocess, stream);
    hipLaunchKernelGGL((preprocess_bwd_kernel<kColor, kExtra>), dim3(ceil_div(p.G, kPreBwdThreads), scenes),
                       dim3(kPreBwdThreads), 0, stream, p, means, cov, shs, opacity, viewmat, projmat,
                       campos, tanfov, scene_scale, radii, (const float*)grec, grad_means, grad_cov,
                       grad_shs, grad_opacity, near, far);
    TSPLAT_PROF_END(prof::kRasterBwdPreprocess, stream);
    TSPLAT_PROF_END(prof::kRasterBwdAll, stream);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

// Argument checks shared by tsplat_raster_bwd (no depth or alpha gradient, depth_mode = 0) and
// tsplat_raster_depth_bwd. Every check comes before the first launch.
static int raster_bwd_run(const tsplat_raster_desc* d, const float* means, const float* cov,
                          const float* shs, const float* opacity, const float* viewmat,
                          const float* projmat, const float* campos, const float* tanfov,
                          const float* bg, const float* scene_scale, const float* near,
                          const float* far, int depth_mode, const float* out_color,
                          const float* out_depth, const float* out_alpha, const float* grad_color,
                          const float* grad_depth, const float* grad_alpha, const int32_t* radii,
                          void* fwd_workspace, void* bwd_workspace, float* grad_means,
                          float* grad_cov, float* grad_shs, float* grad_opacity, void* stream_) {
    if (!d || !means || !cov || !shs || !opacity || !viewmat || !projmat || !campos || !tanfov ||
        !bg || !scene_scale || !radii || !fwd_workspace || !bwd_workspace)
        return TSPLAT_EINVAL;
    if (!grad_color && !grad_depth && !grad_alpha) return TSPLAT_EINVAL;
    if ((grad_color && !out_color) || (grad_depth && !out_depth) || (grad_alpha && !out_alpha))
        return TSPLAT_EINVAL;
    if (grad_depth && (!near || !far)) return TSPLAT_EINVAL;
    if (depth_mode < 0 || depth_mode > 3) return TSPLAT_EINVAL;
    if (!grad_means && !grad_cov && !grad_shs && !grad_opacity) return TSPLAT_EINVAL;
    Params p;
    if (!raster_params(d, grad_depth ? depth_mode : -1, &p)) return TSPLAT_EINVAL;
    p.diag = 0;  // the forward's timing diagnostics have no backward
    hipStream_t stream = (hipStream_t)stream_;
    Workspace ws = carve(fwd_workspace, p.G, p.V, p.T, p.capacity, nullptr);
    float* grec = (float*)bwd_workspace;
#define TSPLAT_RASTER_BWD_ARGS                                                                      \
    p, means, cov, shs, opacity, viewmat, projmat, campos, tanfov, scene_scale, near, far,          \
        out_color, grad_color, out_depth, grad_depth, out_alpha, grad_alpha, radii, ws, grec,       \
        grad_means, grad_cov, grad_shs, grad_opacity, stream
    if (!grad_depth && !grad_alpha) return raster_bwd_launch<true, false>(TSPLAT_RASTER_BWD_ARGS);
    if (grad_color) return raster_bwd_launch<true, true>(TSPLAT_RASTER_BWD_ARGS);
    return raster_bwd_launch<false, true>(TSPLAT_RASTER_BWD_ARGS);
#undef TSPLAT_RASTER_BWD_ARGS
}

extern "C" int tsplat_raster_bwd(const tsplat_raster_desc* d, const float* means, const float* cov,
                                 const float* shs, const float* opacity, const float* viewmat,
                                 const float* projmat, const float* campos, const float* tanfov,
                                 const float* bg, const float* scene_scale, const float* out_color,
                                 const float* grad_color, const int32_t* radii, void* fwd_workspace,
                                 void* bwd_workspace, float* grad_means, float* grad_cov,
                                 float* grad_shs, float* grad_opacity, void* stream_) {
    if (!out_color || !grad_color) return TSPLAT_EINVAL;
    return raster_bwd_run(d, means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale,
                          nullptr, nullptr, 0, out_color, nullptr, nullptr, grad_color, nullptr, nullptr,
                          radii, fwd_workspace, bwd_workspace, grad_means, grad_cov, grad_shs,
                          grad_opacity, stream_);
}

extern "C" int tsplat_raster_depth_bwd(const tsplat_raster_desc* d, const float* means,
                                       const float* cov, const float* shs, const float* opacity,
                                       const float* viewmat, const float* projmat,
                                       const float* campos, const float* tanfov, const float* bg,
                                       const float* scene_scale, const float* near, const float* far,
                                       int32_t depth_mode, const float* out_color,
                                       const float* out_depth, const float* out_alpha,
                                       const float* grad_color, const float* grad_depth,
                                       const float* grad_alpha, const int32_t* radii,
                                       void* fwd_workspace, void* bwd_workspace, float* grad_means,
                                       float* grad_cov, float* grad_shs, float* grad_opacity,
                                       void* stream_) {
    return raster_bwd_run(d, means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale,
                          near, far, depth_mode, out_color, out_depth, out_alpha, grad_color, grad_depth,
                          grad_alpha, radii, fwd_workspace, bwd_workspace, grad_means, grad_cov,
                          grad_shs, grad_opacity, stream_);
}

// ---------------------------------------------------------------------------------------------
// Per-view camera constants of render_cuda (reference src/model/decoder/cuda_splatting.py:56-96,
// get_fov projection.py:233-247, get_projection_matrix cuda_splatting.py:26-53) in one launch,
// one thread per view: scale invariance (t, near, far scaled by 1/near), fov from K^-1 applied
// to the image-edge midpoints, tan(fov / 2), the projection matrix, view = inverse(c2w)^T,
// full = view @ proj^T. Replaces ~40 tiny PyTorch launches per decoder call.
namespace tsplat {
namespace raster {

template <int D>
__device__ void gj_inverse(const float* a_in, float* out) {
    float a[D][2 * D];
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            a[r][c] = a_in[r * D + c];
            a[r][D + c] = r == c ? 1.0f : 0.0f;
        }
    for (int col = 0; col < D; ++col) {
        int piv = col;
        for (int r = col + 1; r < D; ++r)
            if (fabsf(a[r][col]) > fabsf(a[piv][col])) piv = r;
        if (piv != col)
            for (int c = 0; c < 2 * D; ++c) {
                const float t = a[col][c];
                a[col][c] = a[piv][c];
                a[piv][c] = t;
            }
        const float inv = 1.0f / a[col][col];
        for (int c = 0; c < 2 * D; ++c) a[col][c] *= inv;
        for (int r = 0; r < D; ++r) {
            if (r == col) continue;
            const float f = a[r][col];
            for (int c = 0; c < 2 * D; ++c) a[r][c] -= f * a[col][c];
        }
    }
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) out[r * D + c] = a[r][D + c];
}

__global__ void cameras_kernel(const float* __restrict__ ext, const float* __restrict__ intr,
                               const float* __restrict__ near_in, const float* __restrict__ far_in,
                               const float* __restrict__ bg_in, int bg_per_view, int scale_invariant, int V,
                               float* __restrict__ viewmat, float* __restrict__ projmat, float* __restrict__ campos,
                               float* __restrict__ tanfov, float* __restrict__ bg_out, float* __restrict__ scale_out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    float e[16];
    for (int i = 0; i < 16; ++i) e[i] = ext[v * 16 + i];
    float nr = near_in[v], fr = far_in[v], s = 1.0f;
    if (scale_invariant) {
        s = 1.0f / nr;
        e[3] *= s;
        e[7] *= s;
        e[11] *= s;
        nr *= s;
        fr *= s;
    }
    float ki[9];
    gj_inverse<3>(intr + v * 9, ki);
    auto dir = [&](float x, float y, float d[3]) {
        float n2 = 0.f;
        for (int r = 0; r < 3; ++r) {
            d[r] = ki[3 * r] * x + ki[3 * r + 1] * y + ki[3 * r + 2];
            n2 += d[r] * d[r];
        }
        const float n = sqrtf(n2);
        for (int r = 0; r < 3; ++r) d[r] /= n;
    };
    float l[3], r_[3], t[3], b[3];
    dir(0.f, 0.5f, l);
    dir(1.f, 0.5f, r_);
    dir(0.5f, 0.f, t);
    dir(0.5f, 1.f, b);
    const float fov_x = acosf(l[0] * r_[0] + l[1] * r_[1] + l[2] * r_[2]);
    const float fov_y = acosf(t[0] * b[0] + t[1] * b[1] + t[2] * b[2]);
    const float tx = tanf(0.5f * fov_x), ty = tanf(0.5f * fov_y);
    // projection P (row-major), as get_projection_matrix builds it
    const float top = ty * nr, bottom = -top, right = tx * nr, left = -right;
    float P[16] = {0.f};
    P[0] = 2 * nr / (right - left);
    P[5] = 2 * nr / (top - bottom);
    P[2] = (right + left) / (right - left);
    P[6] = (top + bottom) / (top - bottom);
    P[14] = 1.0f;
    P[10] = fr / (fr - nr);
    P[11] = -(fr * nr) / (fr - nr);
    float w2c[16];
    gj_inverse<4>(e, w2c);
    // view_matrix = w2c^T; full = view_matrix @ P^T -> full[i][j] = sum_k w2c[k][i] P[j][k]
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            viewmat[v * 16 + i * 4 + j] = w2c[j * 4 + i];
            float acc = 0.f;
            for (int k = 0; k < 4; ++k) acc += w2c[k * 4 + i] * P[j * 4 + k];
            projmat[v * 16 + i * 4 + j] = acc;
        }
    campos[v * 3 + 0] = e[3];
    campos[v * 3 + 1] = e[7];
    campos[v * 3 + 2] = e[11];
    tanfov[v * 2 + 0] = tx;
    tanfov[v * 2 + 1] = ty;
    for (int c = 0; c < 3; ++c) bg_out[v * 3 + c] = bg_in[(bg_per_view ? v * 3 : 0) + c];
    scale_out[v * 2 + 0] = s;
    scale_out[v * 2 + 1] = s * s;
}

}  // namespace raster
}  // namespace tsplat

extern "C" int tsplat_raster_cameras(const float* extrinsics, const float* intrinsics, const float* near,
                                     const float* far, const float* bg, int32_t bg_per_view, int32_t scale_invariant,
                                     int32_t num_views, float* viewmat, float* projmat, float* campos, float* tanfov,
                                     float* bg_out, float* scale, void* stream_) {
    if (!extrinsics || !intrinsics || !near || !far || !bg || !viewmat || !projmat || !campos || !tanfov ||
        !bg_out || !scale || num_views <= 0)
        return TSPLAT_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(tsplat::raster::cameras_kernel, dim3((num_views + 63) / 64), dim3(64), 0, stream, extrinsics,
                       intrinsics, near, far, bg, bg_per_view, scale_invariant, num_views, viewmat, projmat, campos,
                       tanfov, bg_out, scale);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}
