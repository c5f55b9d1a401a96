// The tile-list sorts of the rasterizer's render kernels, forward and backward: the LDS counting sort, the
// register bitonic network and the global-memory bitonic network, all ascending on (depth bits << 32 | id).
//
// Included by raster.hip only, inside namespace tsplat::raster, after its `#pragma clang fp contract(off)`
// and its constants (kTileThreads, kSortCap): this is a section of that translation unit, not a library.
#pragma once

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
