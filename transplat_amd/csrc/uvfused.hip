// Fine cross correlation without the [HW, HW] table in memory (tsplat_uv_cross_fused_fwd).
//
//   out[n][p][d] = (1/C) sum_pt softmax(logits[n][p][d])_pt sum_corner b_corner <key[n][p], value[n^1][corner]>
//
// The table route computes G[n] = key[n] value[n^1]^T with a library GEMM ([HW, HW] fp32 per map,
// 64 MB at 64 x 64) and gathers 16 scalars of it per (pixel, depth). Here one workgroup owns kQ = 32
// consecutive query pixels of one map and walks the other view's map in bands of kBand = 512
// consecutive pixels (8 image rows at W = 64): per band it computes its 32 x 512 slice of G into
// LDS with split-bf16 MFMAs (key_hi val_hi + key_hi val_lo + key_lo val_hi, fp32 accumulation: the
// products of the K = 3C library GEMM) and every (pixel, depth) pair adds the corners of its
// samples that lie in the band. A first pass marks, per pair and per workgroup, the bands any corner
// falls in (the same corner walk as the gather, so the two cannot disagree); bands nobody samples
// are skipped by a workgroup-uniform test. With every band touched this is the dense product, in
// which a workgroup reads the whole packed map (2 MB at 64 x 64) from L2.
//
// Operands: the key rows are split to (hi, lo) once per workgroup into LDS in A-fragment order.
// value comes pre-split from tsplat_uv_cross_pack_fwd as the B-fragment image
//   packed[map][tile of 32 pixels][k-step 0..7][hi, lo][lane 0..63] x 16 B,
// lane l holding channels 16 ks + 8 (l >> 5) .. + 7 of pixel 32 tile + (l & 31), so a wave's fragment
// load is one contiguous KB; pixels past HW in the last tile are zero.
//
// No atomics and no cross-workgroup state: a pair accumulates its bands in ascending order in its
// own LDS slot, so the result is the same bit for bit from launch to launch.
#include "common.h"
#include "mfma.h"
#include "corr_geo.h"
#include "prof.h"

namespace tsplat {
namespace corr {

constexpr int kQ = 32;                  // query pixels per workgroup: one MFMA M tile
constexpr int kBand = 512;              // value pixels per band
constexpr int kBandShift = 9;
constexpr int kBandTiles = kBand / 32;  // 32-pixel MFMA N tiles per band
constexpr int kGStride = kBand + 8;     // floats per G row: rows 4 apart (the two lane halves of an
                                        // accumulator register) start 32 banks apart
constexpr int kFThreads = 512;
constexpr int kFWaves = kFThreads / 64;
constexpr int kTileU4 = 8 * 2 * 64;     // uint4 per packed 32-pixel tile (16 KB)
constexpr size_t kFusedLds = (size_t)kQ * kGStride * 4 + (size_t)kTileU4 * 16 + kFWaves * 4;

__device__ float4 g_zero32[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

#ifndef TSPLAT_UVX_DIAG
#define TSPLAT_UVX_DIAG 0  // diagnostic builds only: bands touched per workgroup (tools/uv_cross_bands.py)
#endif
#if TSPLAT_UVX_DIAG
__device__ int* g_uvx_bands = nullptr;
#endif

// (hi, lo) bf16 halves of 8 floats, hi = bf16(x), lo = bf16(x - hi), as two 16-B fragments
// (the split rule of mfma.h as 4-wide vector converts; not split_pair: other device code)
__device__ __forceinline__ void split8(floatx4 a, floatx4 b, uint4& hi, uint4& lo) {
    const bf16x4 ah = __builtin_convertvector(a, bf16x4), bh = __builtin_convertvector(b, bf16x4);
    const bf16x4 al = __builtin_convertvector(a - __builtin_convertvector(ah, floatx4), bf16x4);
    const bf16x4 bl = __builtin_convertvector(b - __builtin_convertvector(bh, floatx4), bf16x4);
    const uint2 h0 = __builtin_bit_cast(uint2, ah), h1 = __builtin_bit_cast(uint2, bh);
    const uint2 l0 = __builtin_bit_cast(uint2, al), l1 = __builtin_bit_cast(uint2, bl);
    hi = make_uint4(h0.x, h0.y, h1.x, h1.y);
    lo = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

// value [maps, HW, 128] fp32 (rows ldv floats apart) -> the packed B-fragment image (see the head of
// the file). One thread per (padded pixel, 8-channel unit): 16 consecutive threads read one 512-B
// feature row.
__global__ void __launch_bounds__(256)
uv_cross_pack_kernel(const float* __restrict__ value, int ldv, uint4* __restrict__ packed, int maps, int hw, int tiles) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)maps * tiles * 32 * 16) return;
    const int u = (int)(t & 15);
    const size_t pp = t >> 4;  // padded pixel index over all maps
    const int map = (int)(pp / ((size_t)tiles * 32));
    const int pix = (int)(pp - (size_t)map * tiles * 32);
    const float4* src = pix < hw ? reinterpret_cast<const float4*>(value + ((size_t)map * hw + pix) * ldv + 8 * u)
                                 : g_zero32;
    const float4 a = src[0], b = src[1];
    uint4 hi, lo;
    split8((floatx4){a.x, a.y, a.z, a.w}, (floatx4){b.x, b.y, b.z, b.w}, hi, lo);
    const int tile = pix >> 5, lane = (pix & 31) + 32 * (u & 1), ks = u >> 1;
    uint4* dst = packed + ((size_t)map * tiles + tile) * kTileU4 + (size_t)(ks * 2) * 64 + lane;
    dst[0] = hi;
    dst[64] = lo;
}

// The PMAX sample points of one (pixel p, depth) pair: position in the other view's pixel grid and
// softmax weight (points pt >= P: weight 0 at (-2, -2), which has no corner).
template <int PMAX>
struct PairPoints {
    float x[PMAX], y[PMAX], w[PMAX];
};

// the pair's logits and offsets as read from memory
template <int PMAX>
struct PairRaw {
    float lv[PMAX], ov[2 * PMAX];
};

// P == PMAX == 4 reads the offsets and logits as vector loads; rows of other lengths point by point
template <int PMAX>
__device__ __forceinline__ void load_pair(int P, const float* __restrict__ off, const float* __restrict__ lg,
                                          PairRaw<PMAX>& r) {
    if (PMAX == 4 && P == 4) {
        const float4 l4 = *reinterpret_cast<const float4*>(lg);
        const float4 o0 = reinterpret_cast<const float4*>(off)[0], o1 = reinterpret_cast<const float4*>(off)[1];
        r.lv[0] = l4.x; r.lv[1] = l4.y; r.lv[2] = l4.z; r.lv[3] = l4.w;
        r.ov[0] = o0.x; r.ov[1] = o0.y; r.ov[2] = o0.z; r.ov[3] = o0.w;
        r.ov[4] = o1.x; r.ov[5] = o1.y; r.ov[6] = o1.z; r.ov[7] = o1.w;
    } else {
#pragma unroll
        for (int pt = 0; pt < PMAX; ++pt) {
            r.lv[pt] = pt < P ? lg[pt] : -INFINITY;
            r.ov[2 * pt] = pt < P ? off[2 * pt] : 0.f;
            r.ov[2 * pt + 1] = pt < P ? off[2 * pt + 1] : 0.f;
        }
    }
}

// No fma contraction, as in the table kernel's helpers.
template <int PMAX>
__device__ __forceinline__ void sample_points(const Geo& g, int P, const float* __restrict__ c, int p, float dsp,
                                              const PairRaw<PMAX>& r, PairPoints<PMAX>& s) {
#pragma clang fp contract(off)
    float ray[3];
    pixel_ray(c, (float)(p % g.W), (float)(p / g.W), ray);
    float rx, ry;
    sample_ref(c, g, ray, dsp, rx, ry);
    point_softmax(P, r.lv, s.w);
    const float fw = (float)g.W, fh = (float)g.H;
#pragma unroll
    for (int pt = 0; pt < PMAX; ++pt) {
        s.x[pt] = pt < P ? (rx + r.ov[2 * pt] / fw) * fw - 0.5f : -2.0f;
        s.y[pt] = pt < P ? (ry + r.ov[2 * pt + 1] / fh) * fh - 0.5f : -2.0f;
    }
}

// f(k, inside, pixel index, w x bilinear weight) for the 4 corners k of the sample at (xim, yim);
// inside: the corner counts (the cell of corr_cell.h; a sample that is not taken has the corner
// (-1, -1) and no corner inside). Branch-free, so the gather's 4 LDS reads of a point are in flight
// together; the marking pass and the gather both walk the stored points through this.
template <typename F>
__device__ __forceinline__ void point_corners(const Geo& g, float xim, float yim, float w, F&& f) {
    Cell cl;
    cell_at(xim, yim, g.H, g.W, cl);
    float cw[4];
    cell_weights(cl.ly, cl.lx, cw);
#pragma unroll
    for (int k = 0; k < 4; ++k) f(k, (cl.in >> k) & 1u, (cl.y0 + (k >> 1)) * g.W + (cl.x0 + (k & 1)), w * cw[k]);
}

// PMAX = 4 or 8 points: a thread keeps the sample points of 32 / PMAX pairs in registers from the
// marking pass to the last band (offsets and logits, 50 MB per launch at 64 x 64, are read once),
// so one pass over the bands serves 512 / PMAX depth candidates per query.
template <int PMAX>
__global__ void __launch_bounds__(kFThreads)
uv_cross_fused_kernel(Geo g, int P, const uint4* __restrict__ vpack, const float* __restrict__ key,
                      const float* __restrict__ cams, const float* __restrict__ disp,
                      const float* __restrict__ offsets, int ld_off, const float* __restrict__ logits, int ld_lg,
                      float* __restrict__ out) {
    constexpr int NPAIR = 32 / PMAX;                   // pairs per thread
    constexpr int kDChunk = NPAIR * kFThreads / kQ;    // depth candidates per pass over the bands
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sG = reinterpret_cast<float*>(smem);                              // [kQ][kGStride]
    uint4* sA = reinterpret_cast<uint4*>(smem + (size_t)kQ * kGStride * 4);  // [ks][hi, lo][lane]
    uint32_t* sWave = reinterpret_cast<uint32_t*>(sA + kTileU4);             // [kFWaves]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y, q0 = blockIdx.x * kQ;
    const int HW = g.H * g.W;
    const int tiles = ceil_div(HW, 32), bands = ceil_div(HW, kBand);
    const float* c = cam_ptr(cams, g, n);
    const float* dsp = disp + (size_t)((n & 1) * g.B + (n >> 1)) * g.D;
#if TSPLAT_UVX_DIAG
    const long long t_begin = wall_clock64();
    long long t_marks = 0, t_fill = 0, t_gather = 0;
    int n_bands = 0;
#endif

    {   // the workgroup's key rows -> (hi, lo) A fragments: thread = (row r, 8-channel unit u)
        const int r = tid & 31, u = tid >> 5;
        const float4* src = q0 + r < HW ? reinterpret_cast<const float4*>(key + ((size_t)n * HW + q0 + r) * kC + 8 * u)
                                        : g_zero32;
        const float4 a = src[0], b = src[1];
        uint4 hi, lo;
        split8((floatx4){a.x, a.y, a.z, a.w}, (floatx4){b.x, b.y, b.z, b.w}, hi, lo);
        uint4* dst = sA + ((u >> 1) * 2) * 64 + r + 32 * (u & 1);
        dst[0] = hi;
        dst[64] = lo;
    }

    for (int d0 = 0; d0 < g.D; d0 += kDChunk) {
        const int dn = min(kDChunk, g.D - d0), pairs = kQ * dn;
#if TSPLAT_UVX_DIAG
        const long long t_chunk = d0 ? wall_clock64() : t_begin;
#endif
        // thread's pair j: i = tid + 512 j = (query q0 + i / dn, depth d0 + i % dn)
        PairPoints<PMAX> pts[NPAIR];
        uint32_t bits[NPAIR];
        float acc[NPAIR];
        // ---- marks: bit (band & 31) of every band a corner of the pair falls in
        uint32_t mine = 0;
        {
            // every load of the thread's pairs before the first use: one trip to memory, not NPAIR
            PairRaw<PMAX> raw[NPAIR];
            float dv[NPAIR];
#pragma unroll
            for (int j = 0; j < NPAIR; ++j) {
                const int i = tid + kFThreads * j, q = i / dn, p = q0 + q;
                const bool ok = i < pairs && p < HW;
                // pairs past the block read pair 0 of the map (always there) and are dropped below;
                // a query's rows of offsets / logits lie ld_off / ld_lg floats apart
                const size_t row = (size_t)n * HW + (ok ? p : 0), dd = ok ? d0 + (i - q * dn) : 0;
                load_pair<PMAX>(P, offsets + row * ld_off + dd * P * 2, logits + row * ld_lg + dd * P, raw[j]);
                dv[j] = dsp[ok ? d0 + (i - q * dn) : 0];
            }
#pragma unroll
            for (int j = 0; j < NPAIR; ++j) {
                const int i = tid + kFThreads * j, q = i / dn, p = q0 + q;
                const bool ok = i < pairs && p < HW;
                sample_points<PMAX>(g, P, c, ok ? p : 0, dv[j], raw[j], pts[j]);
                bits[j] = 0;
                acc[j] = 0.f;
#pragma unroll
                for (int pt = 0; pt < PMAX; ++pt) {
                    if (!ok) pts[j].x[pt] = pts[j].y[pt] = -2.0f, pts[j].w[pt] = 0.f;
                    point_corners(g, pts[j].x[pt], pts[j].y[pt], pts[j].w[pt], [&](int, bool inside, int idx, float) {
                        bits[j] |= inside ? 1u << ((idx >> kBandShift) & 31) : 0u;
                    });
                }
                mine |= bits[j];
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) mine |= (uint32_t)__shfl_xor((int)mine, m);
        if (lane == 0) sWave[wave] = mine;
        __syncthreads();
        uint32_t touched = 0;
#pragma unroll
        for (int w = 0; w < kFWaves; ++w) touched |= sWave[w];
#if TSPLAT_UVX_DIAG
        t_marks += wall_clock64() - t_chunk;
#endif

        for (int band = 0; band < bands; ++band) {
            if (!((touched >> (band & 31)) & 1)) continue;  // workgroup-uniform
#if TSPLAT_UVX_DIAG
            const long long t0 = wall_clock64();
            ++n_bands;
#endif
            // ---- G[0:32][band] = key value_other^T: wave w takes the band's tiles w, w + 8
            const int tb = min(kBandTiles, tiles - band * kBandTiles);
#pragma unroll 1
            for (int s = 0; s < kBandTiles / kFWaves; ++s) {
                const int t = wave + kFWaves * s;
                if (t < tb) {
                    const uint4* vb = vpack + ((size_t)(n ^ 1) * tiles + band * kBandTiles + t) * kTileU4 + lane;
                    uint4 bf[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) bf[k] = vb[k * 64];
                    floatx16 a16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) {
                        const bf16x8 ah = __builtin_bit_cast(bf16x8, sA[(ks * 2) * 64 + lane]);
                        const bf16x8 al = __builtin_bit_cast(bf16x8, sA[(ks * 2 + 1) * 64 + lane]);
                        const bf16x8 bh = __builtin_bit_cast(bf16x8, bf[2 * ks]);
                        const bf16x8 bl = __builtin_bit_cast(bf16x8, bf[2 * ks + 1]);
                        a16 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, a16, 0, 0, 0);
                        a16 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, a16, 0, 0, 0);
                        a16 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, a16, 0, 0, 0);
                    }
                    // accumulator register i of lane l: query row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31
                    float* gcol = sG + (4 * (lane >> 5)) * kGStride + t * 32 + (lane & 31);
#pragma unroll
                    for (int i = 0; i < 16; ++i) gcol[((i & 3) + 8 * (i >> 2)) * kGStride] = a16[i];
                }
            }
            __syncthreads();
#if TSPLAT_UVX_DIAG
            const long long t1 = wall_clock64();
            t_fill += t1 - t0;
#endif
            // ---- gather: the pairs that marked this band add their corners inside it
#pragma unroll
            for (int j = 0; j < NPAIR; ++j) {
                if (!((bits[j] >> (band & 31)) & 1)) continue;
                const float* grow = sG + min((tid + kFThreads * j) / dn, kQ - 1) * kGStride;
#pragma unroll
                for (int pt = 0; pt < PMAX; ++pt) {
                    // the corner walk is redone per band from the 3 stored floats: hoisted out of the band
                    // loop, its 8 derived values per point would not fit the register file
                    float x = pts[j].x[pt], y = pts[j].y[pt];
                    asm volatile("" : "+v"(x), "+v"(y));
                    // a corner outside the band (or the map) reads some column of the row and drops the value
                    point_corners(g, x, y, pts[j].w[pt], [&](int, bool inside, int idx, float w) {
                        const float v = grow[idx & (kBand - 1)];
                        // & not &&: no short-circuit branch for the compiler to sink the LDS read into
                        acc[j] += w * (inside & ((idx >> kBandShift) == band) ? v : 0.f);
                    });
                }
            }
            __syncthreads();
#if TSPLAT_UVX_DIAG
            t_gather += wall_clock64() - t1;
#endif
        }
#pragma unroll
        for (int j = 0; j < NPAIR; ++j) {
            const int i = tid + kFThreads * j, q = i / dn, p = q0 + q;
            if (i < pairs && p < HW) out[((size_t)n * HW + p) * g.D + d0 + (i - q * dn)] = acc[j] / (float)kC;
        }
        __syncthreads();  // sWave is rewritten by the next depth chunk
    }
#if TSPLAT_UVX_DIAG
    // per workgroup: bands computed, then 10-ns ticks in the marking pass, the fills, the gathers, in all
    if (tid == 0 && g_uvx_bands) {
        int* o = g_uvx_bands + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8;
        o[0] = n_bands; o[1] = (int)t_marks; o[2] = (int)t_fill; o[3] = (int)t_gather;
        o[4] = (int)(wall_clock64() - t_begin);
    }
#endif
}

}  // namespace corr
}  // namespace tsplat

using namespace tsplat;

extern "C" size_t tsplat_uv_cross_pack_bytes(int32_t batch, int32_t height, int32_t width) {
    if (batch <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)2 * batch * ceil_div((size_t)height * width, (size_t)32) * corr::kTileU4 * 16;
}

extern "C" int tsplat_uv_cross_pack_ld_fwd(const float* value, int32_t ld_value, void* packed, int32_t batch,
                                           int32_t height, int32_t width, int32_t channels, void* stream_) {
    using namespace tsplat::corr;
    if (!value || !packed || channels != kC || batch <= 0 || height <= 1 || width <= 1 || ld_value < kC ||
        ld_value % 4 || (size_t)height * width > (size_t)1 << 24 || (uintptr_t)value % 16 || (uintptr_t)packed % 16)
        return TSPLAT_EINVAL;
    const int hw = height * width, tiles = ceil_div(hw, 32), maps = 2 * batch;
    const size_t work = (size_t)maps * tiles * 32 * 16;
    hipLaunchKernelGGL(uv_cross_pack_kernel, dim3((unsigned)ceil_div(work, (size_t)256)), dim3(256), 0,
                       (hipStream_t)stream_, value, ld_value, (uint4*)packed, maps, hw, tiles);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

extern "C" int tsplat_uv_cross_pack_fwd(const float* value, void* packed, int32_t batch, int32_t height,
                                        int32_t width, int32_t channels, void* stream_) {
    return tsplat_uv_cross_pack_ld_fwd(value, tsplat::corr::kC, packed, batch, height, width, channels, stream_);
}

extern "C" int tsplat_uv_cross_fused_ld_fwd(const void* packed, const float* key, const float* cams,
                                            const float* disp, const float* offsets, int32_t ld_offsets,
                                            const float* logits, int32_t ld_logits, float* out, int32_t batch,
                                            int32_t height, int32_t width, int32_t channels, int32_t depths,
                                            int32_t points, void* stream_) {
    using namespace tsplat::corr;
    if (!packed || !key || !cams || !disp || !offsets || !logits || !out || channels != kC || batch <= 0 ||
        height <= 1 || width <= 1 || depths <= 0 || points <= 0 || points > kMaxPoints ||
        (size_t)height * width > (size_t)1 << 24 || 2 * batch > 65535 ||
        (size_t)2 * batch * height * width * depths * points > (size_t)1 << 40 ||
        (uintptr_t)packed % 16 || (uintptr_t)key % 16 || (uintptr_t)offsets % 16 || (uintptr_t)logits % 16)
        return TSPLAT_EINVAL;
    // rows hold at least the depths x points entries; the 4-point kernel reads them as float4
    if ((int64_t)ld_offsets < (int64_t)depths * points * 2 || (int64_t)ld_logits < (int64_t)depths * points ||
        (points == 4 && (ld_offsets % 4 || ld_logits % 4)))
        return TSPLAT_EINVAL;
    Geo g{batch, height, width, depths};
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(ceil_div(height * width, kQ), 2 * batch);
    // 81 KB of LDS per workgroup: above 64 KB the kernel's dynamic-LDS limit is raised
    static_assert(kFusedLds <= 160 * 1024, "LDS of the fused cross correlation exceeds gfx950's 160 KB");
    const void* fn = points <= 4 ? reinterpret_cast<const void*>(&uv_cross_fused_kernel<4>)
                                 : reinterpret_cast<const void*>(&uv_cross_fused_kernel<8>);
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFusedLds) != hipSuccess)
        return TSPLAT_EHIP;
    TSPLAT_PROF_BEGIN(prof::kUvCross, stream);
    if (points <= 4)
        hipLaunchKernelGGL(uv_cross_fused_kernel<4>, grid, dim3(kFThreads), kFusedLds, stream, g, points,
                           (const uint4*)packed, key, cams, disp, offsets, ld_offsets, logits, ld_logits, out);
    else
        hipLaunchKernelGGL(uv_cross_fused_kernel<8>, grid, dim3(kFThreads), kFusedLds, stream, g, points,
                           (const uint4*)packed, key, cams, disp, offsets, ld_offsets, logits, ld_logits, out);
    TSPLAT_PROF_END(prof::kUvCross, stream);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}

extern "C" int tsplat_uv_cross_fused_fwd(const void* packed, const float* key, const float* cams, const float* disp,
                                         const float* offsets, const float* logits, float* out, int32_t batch,
                                         int32_t height, int32_t width, int32_t channels, int32_t depths,
                                         int32_t points, void* stream_) {
    if (depths <= 0 || depths > (1 << 24) || points <= 0 || points > tsplat::corr::kMaxPoints) return TSPLAT_EINVAL;
    // contiguous rows; with 4 points depths * 4 and depths * 8 floats keep every row 16-byte aligned
    return tsplat_uv_cross_fused_ld_fwd(packed, key, cams, disp, offsets, depths * points * 2, logits,
                                        depths * points, out, batch, height, width, channels, depths, points, stream_);
}

#if TSPLAT_UVX_DIAG
// diagnostic builds: buf [workgroups][8] int32 receives, per workgroup, the bands it computed and its
// phase clocks (see the end of the kernel); nullptr turns the recording off
extern "C" int tsplat_uv_cross_fused_diag(int* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(tsplat::corr::g_uvx_bands), &buf, sizeof(buf)) == hipSuccess ? TSPLAT_OK
                                                                                                    : TSPLAT_EHIP;
}
#endif
