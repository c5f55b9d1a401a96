// Gaussian-splat rasterizer for gfx950 (MI355X): the forward, and the backward of its colour, depth and
// alpha renders in the Gaussians (tsplat_raster_bwd, tsplat_raster_depth_bwd: render_bwd_kernel and
// preprocess_bwd_kernel). Forward and backward run the same steps, each defined once: the sorts in
// raster_sort.h; projection and EWA covariance, SH basis, depth value, tile prologue, chunk walk and blend
// decision in raster_steps.h.
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

// The tile-list sorts, and the steps the forward kernels and their backward share, one definition each.
// Sections of this translation unit (contraction stays off in them), not headers for anyone else.
#include "raster_sort.h"
#include "raster_steps.h"

__device__ __forceinline__ void get_rect(float px, float py, int r, int tx, int ty, int& x0,
                                         int& y0, int& x1, int& y1) {
    // (int) truncation and clamps exactly as the reference getRect (auxiliary.h)
    x0 = min(tx, max(0, (int)((px - (float)r) / (float)kTile)));
    y0 = min(ty, max(0, (int)((py - (float)r) / (float)kTile)));
    x1 = min(tx, max(0, (int)((px + (float)r + (float)(kTile - 1)) / (float)kTile)));
    y1 = min(ty, max(0, (int)((py + (float)r + (float)(kTile - 1)) / (float)kTile)));
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
            const ViewPoint q = view_point(m0, m1, m2, s, vm);
            const float vz = q.vz;
            bool ok = vz > 0.2f;
            float px = 0.f, py = 0.f, conic_a = 0.f, conic_b = 0.f, conic_c = 0.f;
            float cov_a = 0.f, cov_c = 0.f;
            int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
            if (ok) {
                const Projection pr = project(q, k00, k01, k02, k11, k12, k22, s2, vm, pm, tanfov[2 * v],
                                              tanfov[2 * v + 1], p.W, p.H);
                const float ndc_x = pr.hx * pr.pw, ndc_y = pr.hy * pr.pw;
                const float a = pr.a, c = pr.c, det = pr.det;
                cov_a = a;
                cov_c = c;
                ok = det != 0.0f;
                if (ok) {
                    const Conic co = conic_of(pr);
                    conic_a = co.a;
                    conic_b = co.b;
                    conic_c = co.c;
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
                    if (p.depth_mode >= 0) d = depth_value(p.depth_mode, vz, s, near[v], far[v]).d;
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
        const ViewPoint q = view_point(m0, m1, m2, s, vm);  // pass 1's, bit for bit: q.vz is the sort key
        float rgb[3] = {0.5f, 0.5f, 0.5f};
        const float* cp = campos + 3 * v;
        if (!no_sh) sh_to_rgb(my_sh, p.M, p.deg, sh_dir(q.mx - cp[0], q.my - cp[1], q.mz - cp[2]), rgb);
        ws.rec[4 * ((size_t)v * p.G + g) + 2] = make_float4(rgb[0], rgb[1], rgb[2], q.vz);
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
    using L = RecLayout<kColor, kExtra, false>;  // 9, 10 or 7 fields
    __shared__ uint64_t skeys[kSortCap];
    __shared__ uint32_t s_cnt[kBuckets];
    __shared__ uint32_t s_red[4];
    // per-wave compacted records of the current 64-entry chunk (waves progress independently),
    // field-major: one ds_read_b128 of a field gives 4 consecutive entries = 2 packed pairs
    __shared__ __attribute__((aligned(16))) float s_rec[kTileThreads / kWave][L::kRecFields][kWave];

    const int v = blockIdx.y;
    const uint64_t t_begin = p.diag == 5 ? __builtin_amdgcn_s_memtime() : 0;
    int d_entries = 0, d_chunks = 0;  // diag 5 only
    TileList tl;
    if (!tile_prologue(p, ws, v, {skeys, s_cnt, s_red}, tl)) return;

    const WavePixel wp = wave_pixel(p, tl.tile);
    bool done = !wp.inside;
    float T = 1.0f;
    float C0 = 0.f, C1 = 0.f, C2 = 0.f;
    float D = 0.f;  // kExtra: sum of d w
    float (*w_rec)[kWave] = s_rec[wp.wid];

    // C += rgb w and D += d w with the entry's weight w = alpha T of blend_step()
    auto blend = [&](auto, float x, float y, float ca, float cb, float cc, float o, float r, float g, float bl,
                     float d) {
        const BlendStep b = blend_step(x, y, ca, cb, cc, o, wp.pfx, wp.pfy, T, done);
        if constexpr (kColor) {
            C0 = fmaf(r, b.w, C0);
            C1 = fmaf(g, b.w, C1);
            C2 = fmaf(bl, b.w, C2);
        }
        if constexpr (kExtra) D = fmaf(d, b.w, D);
    };
    walk_tile<L>(p, ws, v, tl, skeys, wp, w_rec, done, [&](int m) {
        d_entries += m;
        ++d_chunks;
        // groups of 4 entries: one ds_read_b128 per field
        const int m4 = m & ~3;
        for (int i = 0; i < m4; i += 4) {
            float4 q[L::kDataFields];
            load_quad<L>(w_rec, i, q);
            quad_each<L>(q, blend);
        }
        for (int i = m4; i < m; ++i)
            blend(0, w_rec[0][i], w_rec[1][i], w_rec[2][i], w_rec[3][i], w_rec[4][i], w_rec[5][i], w_rec[L::iR][i],
                  w_rec[L::iG][i], w_rec[L::iB][i], w_rec[L::iD][i]);
    });
    if (p.diag == 5) {  // per-wave cost instead of colours: cycles since the start, entries, chunks
        C0 = (float)(__builtin_amdgcn_s_memtime() - t_begin);
        C1 = (float)d_entries;
        C2 = (float)d_chunks;
        T = 0.0f;
    }
    if (wp.inside) {
        const size_t hw = (size_t)p.H * p.W;
        const size_t pix = (size_t)wp.pyi * p.W + wp.pxi;
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
// forward's workspace by the forward's tile_prologue() (same total order on (depth bits, id)), and each
// wave walks it through the forward's chunk_walk() and blend_step() (one definition each, under this
// file's contraction-off rule, so T, alpha and every branch are the forward's bit for bit; early exit
// included). Walk direction: FRONT TO BACK. With g the
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
    using L = RecLayout<kColor, kExtra, true>;  // 10, 11 or 8 fields, the id last
    constexpr int kSums = L::kDataFields;       // 9, 10 or 7: one sum per data field
    constexpr int kDepthSum = kSums - 1;        // kExtra: the local index of sum w gd
    static_assert(kSums <= kAccStride && kGradFields + 1 <= kGradRecFloats, "sums fit their slots");
    __shared__ uint64_t skeys[kSortCap];
    __shared__ uint32_t s_cnt[kBuckets];
    __shared__ uint32_t s_red[4];
    __shared__ __attribute__((aligned(16))) float s_rec[kTileThreads / kWave][L::kRecFields][kWave];
    __shared__ __attribute__((aligned(16))) float s_acc[kTileThreads / kWave][kWave][kAccStride];

    const int v = blockIdx.y;
    TileList tl;
    if (!tile_prologue(p, ws, v, {skeys, s_cnt, s_red}, tl)) return;  // never: p.diag is 0 in the backward

    const WavePixel wp = wave_pixel(p, tl.tile);
    const int lane = wp.lane, pxi = wp.pxi, pyi = wp.pyi;
    bool done = !wp.inside;
    float T = 1.0f;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    float gd = 0.f;  // kExtra
    float S = 0.f;  // out . g minus the entries walked so far
    if (wp.inside) {
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
    float (*w_rec)[kWave] = s_rec[wp.wid];
    float (*w_acc)[kAccStride] = s_acc[wp.wid];
    const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0;
    const int my_e = (b0 ? 2 : 0) + (b1 ? 1 : 0);  // the quad entry whose sums this lane ends up with

    // one entry at this lane's pixel: the forward's decisions (blend_step), then its contributions
    float va[4][kSums];
    auto entry = [&](auto e, float x, float y, float ca, float cb, float cc, float o, float r, float g, float bl,
                     float d) {
        float (&val)[kSums] = va[decltype(e)::value];
        const BlendStep b = blend_step(x, y, ca, cb, cc, o, wp.pfx, wp.pfy, T, done);
        const float dx = b.dx, dy = b.dy, alpha = b.alpha, w = b.w;
        float cg = 0.0f;
        if constexpr (kColor) cg = r * g0 + g * g1 + bl * g2;
        if constexpr (kExtra) cg = cg + d * gd;  // alpha's term: the constant in S
        S = fmaf(-w, cg, S);
        const float dalpha = b.acc ? b.T_in * cg - S * __builtin_amdgcn_rcpf(1.0f - alpha) : 0.0f;
        const bool pass = b.acc && !(b.oe > 0.99f);  // the 0.99 cap passes nothing to conic, mean, opacity
        const float gp = pass ? dalpha * alpha : 0.0f;  // dL/d power (natural log domain)
        constexpr float kLn2 = 0.69314718055994531f;
        const float gl = gp * kLn2;  // the stored conic carries log2(e)
        val[0] = gl * fmaf(2.0f * ca, dx, cb * dy);
        val[1] = gl * fmaf(2.0f * cc, dy, cb * dx);
        val[2] = gp * (-0.5f * dx * dx);
        val[3] = gp * (-dx * dy);
        val[4] = gp * (-0.5f * dy * dy);
        val[5] = pass ? dalpha * b.ex : 0.0f;
        if constexpr (kColor) {
            val[6] = w * g0;
            val[7] = w * g1;
            val[8] = w * g2;
        }
        if constexpr (kExtra) val[kDepthSum] = w * gd;
    };

    walk_tile<L>(p, ws, v, tl, skeys, wp, w_rec, done, [&](int m) {
        const int m4 = (m + 3) & ~3;  // the walk padded the last quad
        for (int i = 0; i < m4; i += 4) {
            float4 q[L::kDataFields];
            load_quad<L>(w_rec, i, q);
            quad_each<L>(q, entry);
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
        const int f = lane & 15;
        for (int j = 0; j < m; j += 4) {
            const int e = j + (lane >> 4);
            if (e < m && f < kSums) {
                const float val = w_acc[e][f];
                const uint32_t id = __float_as_uint(w_rec[L::kIdField][e]);
                // the record's field: the local sum's own index, but for the depth sum without colour
                const int rf = (!kColor && f == kDepthSum) ? kGradFields : f;
                if (val != 0.0f) atomicAdd(grec + (vbase + id) * kGradRecFloats + rf, val);
            }
        }
    });
}

// --- B2: gradient records -> gradients of the Gaussians ----------------------------------------
// One thread per Gaussian for all views of its scene (blockIdx.y = scene), the mirror of
// preprocess_kernel: the forward geometry of each view is recomputed by the forward's view_point(),
// project(), conic_of() and sh_basis(), the view's gradient record is chained through them, and the contributions of the
// views are summed in registers (SH: in the thread's LDS slot) and written once. No atomics. Views
// with radii == 0 are skipped. The SH block of a wave's 64 Gaussians is staged to LDS and its
// gradient written back by coalesced loops, as the forward reads it. 128 threads per workgroup:
// two [threads][75] float LDS arrays (coefficients and their gradients), 76,800 bytes.
constexpr int kPreBwdThreads = 128;

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
            // forward geometry: the forward's own steps
            const ViewPoint q = view_point(m0, m1, m2, s, vm);
            const Projection pr = project(q, k00, k01, k02, k11, k12, k22, s2, vm, pm, tanfov[2 * v],
                                          tanfov[2 * v + 1], p.W, p.H);
            const Conic co = conic_of(pr);
            const float mx = q.mx, my = q.my, mz = q.mz, vx = q.vx, vy = q.vy, vz = q.vz, tz = q.vz;
            const float hx = pr.hx, hy = pr.hy, pw = pr.pw, fx = pr.fx, fy = pr.fy, rx = pr.rx, ry = pr.ry;
            const bool in_x = pr.in_x, in_y = pr.in_y;
            const float n00 = pr.n00, n01 = pr.n01, n02 = pr.n02, n10 = pr.n10, n11 = pr.n11, n12 = pr.n12;
            const float u00 = pr.u00, u01 = pr.u01, u02 = pr.u02, u10 = pr.u10, u11 = pr.u11, u12 = pr.u12;
            const float qa = co.a, qb = co.b, qc = co.c;

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
                    dvz = dvz + g_d * depth_value(p.depth_mode, vz, s, near[v], far[v]).dz / s;
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
                const ShDir n = sh_dir(mx - cp[0], my - cp[1], mz - cp[2]);
                float rgb[3];
                sh_to_rgb(my_sh, p.M, p.deg, n, rgb);
                float tc[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) tc[ch] = rgb[ch] > 0.0f ? g_rgb[ch] : 0.0f;  // the clamp at 0
                float dnx = 0.f, dny = 0.f, dnz = 0.f;
                // one basis function: value B and its gradient (bx, by, bz) in the unit direction
                sh_basis(p.deg, n.x, n.y, n.z, [&](auto k_, float B, float bx, float by, float bz) {
                    constexpr int k = decltype(k_)::value;
                    const float ak = tc[0] * my_sh[k] + tc[1] * my_sh[p.M + k] + tc[2] * my_sh[2 * p.M + k];
                    dnx += bx * ak;
                    dny += by * ak;
                    dnz += bz * ak;
                    my_dsh[k] += tc[0] * B;
                    my_dsh[p.M + k] += tc[1] * B;
                    my_dsh[2 * p.M + k] += tc[2] * B;
                });
                // through n = d / |d|: dL/dd = (dn - n (n . dn)) / |d|
                const float ndot = n.x * dnx + n.y * dny + n.z * dnz;
                dmx += (dnx - n.x * ndot) / n.len;
                dmy += (dny - n.y * ndot) / n.len;
                dmz += (dnz - n.z * ndot) / n.len;
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

// The Gaussians and cameras every entry point reads, forward and backward. near / far: the depth entry
// points' planes, NULL elsewhere (each entry point checks them where it needs them).
struct Scene {
    const float *means, *cov, *shs, *opacity, *viewmat, *projmat, *campos, *tanfov, *bg, *scene_scale, *near, *far;
};
static bool scene_ok(const Scene& s) {
    return s.means && s.cov && s.shs && s.opacity && s.viewmat && s.projmat && s.campos && s.tanfov && s.bg &&
           s.scene_scale;
}

// The launch sequence of both entry points. kColor / kExtra pick the preprocess and render
// instantiations: <true, false> is tsplat_raster_fwd; tsplat_raster_depth_fwd takes <true, true>
// with a colour output and <false, true> without one.
template <bool kColor, bool kExtra>
static int raster_launch(Params p, const Scene& s, float* out_color, float* out_depth, float* out_alpha,
                         int32_t* out_radii, Workspace ws, int32_t* status, hipStream_t stream) {
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
                       stream, p, s.means, s.cov, s.shs, s.opacity, s.viewmat, s.projmat, s.campos, s.tanfov,
                       s.scene_scale, s.near, s.far, out_radii, ws);
    TSPLAT_PROF_END(prof::kRasterPreprocess, stream);
    TSPLAT_CHECK_LAUNCH();
    TSPLAT_PROF_BEGIN(prof::kRasterScatter, stream);
    hipLaunchKernelGGL(scatter_kernel, pre_grid, dim3(kPreThreads), 3 * p.T * sizeof(uint32_t),
                       stream, p, (const int32_t*)out_radii, ws, status);
    TSPLAT_PROF_END(prof::kRasterScatter, stream);
    TSPLAT_CHECK_LAUNCH();
    TSPLAT_PROF_BEGIN(prof::kRasterRender, stream);
    hipLaunchKernelGGL((render_kernel<kColor, kExtra>), dim3(p.T, p.V), dim3(kTileThreads), 0, stream, p,
                       s.bg, out_color, out_depth, out_alpha, ws);
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
static int raster_run(const tsplat_raster_desc* d, const Scene& s, int depth_mode, bool extra, float* out_color,
                      float* out_depth, float* out_alpha, int32_t* out_radii, void* workspace, int32_t* status,
                      void* stream_) {
    if (!d || !scene_ok(s) || !out_radii || !workspace || !status) return TSPLAT_EINVAL;
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
    p.sh_vec4 = ((uintptr_t)s.shs % 16 == 0) && (scenes == 1 || ((size_t)3 * p.M * p.G) % 4 == 0);
    const auto launch = !extra ? raster_launch<true, false>
                               : out_color ? raster_launch<true, true> : raster_launch<false, true>;
    return launch(p, s, out_color, out_depth, out_alpha, out_radii, ws, status, stream);
}

extern "C" int tsplat_raster_fwd(const tsplat_raster_desc* d, const float* means, const float* cov,
                                 const float* shs, const float* opacity, const float* viewmat,
                                 const float* projmat, const float* campos, const float* tanfov,
                                 const float* bg, const float* scene_scale, float* out_color,
                                 int32_t* out_radii, void* workspace, int32_t* status,
                                 void* stream_) {
    if (!out_color) return TSPLAT_EINVAL;
    const Scene s{means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale, nullptr, nullptr};
    return raster_run(d, s, -1, false, out_color, nullptr, nullptr, out_radii, workspace, status, stream_);
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
    const Scene s{means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale, near, far};
    return raster_run(d, s, out_depth ? depth_mode : -1, true, out_color, out_depth, out_alpha, out_radii,
                      workspace, status, stream_);
}

extern "C" size_t tsplat_raster_bwd_workspace_bytes(int32_t G, int32_t V) {
    if (G <= 0 || V <= 0) return 0;
    return align_up((size_t)G * V * kGradRecFloats * sizeof(float), 256);
}

// What a backward call adds to the Scene: the saved outputs and the gradients at them (NULL: not part of
// the loss), and the four gradient outputs (NULL: not asked for).
struct BwdIo {
    const float *out_color, *out_depth, *out_alpha, *grad_color, *grad_depth, *grad_alpha;
    float *grad_means, *grad_cov, *grad_shs, *grad_opacity;
};

// The launch sequence of both backward entry points: zero fill of the gradient records,
// render_bwd_kernel, preprocess_bwd_kernel, in the <kColor, kExtra> instantiations. <true, false> is
// tsplat_raster_bwd's, and tsplat_raster_depth_bwd's with a colour gradient alone; <true, true> adds a
// depth and / or alpha gradient to the colour's; <false, true> runs without a colour gradient.
template <bool kColor, bool kExtra>
static int raster_bwd_launch(Params p, const Scene& s, const BwdIo& io, const int32_t* radii, Workspace ws,
                             float* grec, hipStream_t stream) {
    TSPLAT_PROF_BEGIN(prof::kRasterBwdAll, stream);
    {
        const size_t n4 = (size_t)p.G * p.V * kGradRecFloats / 4;
        const int blocks = (int)std::min<size_t>(ceil_div(n4, (size_t)256), 4096);
        hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, stream, (uint4*)grec, n4);
        TSPLAT_CHECK_LAUNCH();
    }
    TSPLAT_PROF_BEGIN(prof::kRasterBwdRender, stream);
    hipLaunchKernelGGL((render_bwd_kernel<kColor, kExtra>), dim3(p.T, p.V), dim3(kTileThreads), 0, stream,
                       p, io.out_color, io.grad_color, grec, ws, io.out_depth, io.grad_depth, io.out_alpha,
                       io.grad_alpha);
    TSPLAT_PROF_END(prof::kRasterBwdRender, stream);
    TSPLAT_CHECK_LAUNCH();
    const int scenes = p.V / p.vps;
    TSPLAT_PROF_BEGIN(prof::kRasterBwdPreprocess, stream);
    hipLaunchKernelGGL((preprocess_bwd_kernel<kColor, kExtra>), dim3(ceil_div(p.G, kPreBwdThreads), scenes),
                       dim3(kPreBwdThreads), 0, stream, p, s.means, s.cov, s.shs, s.opacity, s.viewmat, s.projmat,
                       s.campos, s.tanfov, s.scene_scale, radii, (const float*)grec, io.grad_means, io.grad_cov,
                       io.grad_shs, io.grad_opacity, s.near, s.far);
    TSPLAT_PROF_END(prof::kRasterBwdPreprocess, stream);
    TSPLAT_PROF_END(prof::kRasterBwdAll, stream);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

// Argument checks shared by tsplat_raster_bwd (no depth or alpha gradient, depth_mode = 0) and
// tsplat_raster_depth_bwd. Every check comes before the first launch.
static int raster_bwd_run(const tsplat_raster_desc* d, const Scene& s, int depth_mode, const BwdIo& io,
                          const int32_t* radii, void* fwd_workspace, void* bwd_workspace, void* stream_) {
    if (!d || !scene_ok(s) || !radii || !fwd_workspace || !bwd_workspace) return TSPLAT_EINVAL;
    if (!io.grad_color && !io.grad_depth && !io.grad_alpha) return TSPLAT_EINVAL;
    if ((io.grad_color && !io.out_color) || (io.grad_depth && !io.out_depth) || (io.grad_alpha && !io.out_alpha))
        return TSPLAT_EINVAL;
    if (io.grad_depth && (!s.near || !s.far)) return TSPLAT_EINVAL;
    if (depth_mode < 0 || depth_mode > 3) return TSPLAT_EINVAL;
    if (!io.grad_means && !io.grad_cov && !io.grad_shs && !io.grad_opacity) return TSPLAT_EINVAL;
    Params p;
    if (!raster_params(d, io.grad_depth ? depth_mode : -1, &p)) return TSPLAT_EINVAL;
    p.diag = 0;  // the forward's timing diagnostics have no backward
    hipStream_t stream = (hipStream_t)stream_;
    Workspace ws = carve(fwd_workspace, p.G, p.V, p.T, p.capacity, nullptr);
    const auto launch = !io.grad_depth && !io.grad_alpha ? raster_bwd_launch<true, false>
                        : io.grad_color                  ? raster_bwd_launch<true, true>
                                                         : raster_bwd_launch<false, true>;
    return launch(p, s, io, radii, ws, (float*)bwd_workspace, stream);
}

extern "C" int tsplat_raster_bwd(const tsplat_raster_desc* d, const float* means, const float* cov,
                                 const float* shs, const float* opacity, const float* viewmat,
                                 const float* projmat, const float* campos, const float* tanfov,
                                 const float* bg, const float* scene_scale, const float* out_color,
                                 const float* grad_color, const int32_t* radii, void* fwd_workspace,
                                 void* bwd_workspace, float* grad_means, float* grad_cov,
                                 float* grad_shs, float* grad_opacity, void* stream_) {
    if (!out_color || !grad_color) return TSPLAT_EINVAL;
    const Scene s{means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale, nullptr, nullptr};
    const BwdIo io{out_color, nullptr, nullptr, grad_color, nullptr, nullptr,
                   grad_means, grad_cov, grad_shs, grad_opacity};
    return raster_bwd_run(d, s, 0, io, radii, fwd_workspace, bwd_workspace, stream_);
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
    const Scene s{means, cov, shs, opacity, viewmat, projmat, campos, tanfov, bg, scene_scale, near, far};
    const BwdIo io{out_color, out_depth, out_alpha, grad_color, grad_depth, grad_alpha,
                   grad_means, grad_cov, grad_shs, grad_opacity};
    return raster_bwd_run(d, s, depth_mode, io, radii, fwd_workspace, bwd_workspace, stream_);
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
