// Exact quantiles of an fp32 array without a sort and without a host round trip: radix selection
// on the order-preserving 32-bit key, 4 passes of 8-bit digits from the top. Replaces the two
// torch.quantile calls (full sorts of 2-16 M values) and the boolean-mask indexing of the
// reference's depth_map closure (src/model/model_wrapper.py:736-738).
//
// A request (q, positive_only) needs the order statistics k = floor(q (m - 1)) and min(k + 1, m - 1)
// of its population, so R requests are 2R selectors, each with its own key prefix and remaining
// rank. Selectors whose (prefix, population) agree share one histogram slot (pass 0 has at most
// two slots: all values, positive values). Per pass: every workgroup histograms the elements that
// match a slot's prefix into LDS and flushes one integer atomic per non-empty bin; a single small
// workgroup then prefix-sums the bins and picks each selector's bucket. Integer atomics only: the
// result is bit-identical from run to run.
#include "common.h"

namespace tsplat {
namespace quantile {

constexpr int kMaxReq = 4;
constexpr int kSel = 2 * kMaxReq;
constexpr int kBins = 256;
constexpr int kPasses = 4;
constexpr int kThreads = 256;
constexpr uint32_t kKeyZero = 0x80000000u;  // key of +0.0: a value is positive iff its key is above

struct State {
    uint32_t prefix[kSel];  // the digits chosen so far (pass p: the top 8 p bits of the key)
    uint32_t rank[kSel];    // rank of the wanted element among the keys that share the prefix
    int32_t slot[kSel];     // histogram slot of the selector
    int32_t slot_sel[kSel]; // a selector of each slot (its prefix and population)
    int32_t num_slots;
    int32_t num_requests;
    int32_t positive[kMaxReq];
    uint32_t count[kMaxReq];  // m, the population size
    double q[kMaxReq];
    double frac[kMaxReq];
};

struct Requests {
    double q[kMaxReq];
    int32_t positive[kMaxReq];
    int32_t n;
};

__host__ __device__ inline size_t hist_bytes() { return (size_t)kPasses * kSel * kBins * sizeof(uint32_t); }

__device__ inline uint32_t key_of(float x) {
    const uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : kKeyZero);
}

__device__ inline float value_of(uint32_t key) {
    return __uint_as_float(key ^ ((key >> 31) ? kKeyZero : 0xFFFFFFFFu));
}

// slots: selectors with equal (prefix, population) share one
__device__ inline void assign_slots(State* st) {
    const int ns = 2 * st->num_requests;
    int slots = 0;
    for (int s = 0; s < ns; ++s) {
        int found = -1;
        for (int u = 0; u < s; ++u)
            if (st->prefix[u] == st->prefix[s] && st->positive[u >> 1] == st->positive[s >> 1]) {
                found = st->slot[u];
                break;
            }
        if (found < 0) {
            found = slots;
            st->slot_sel[slots++] = s;
        }
        st->slot[s] = found;
    }
    st->num_slots = slots;
}

__global__ void init_kernel(Requests rq, uint32_t* __restrict__ hist, State* __restrict__ st) {
    for (int i = threadIdx.x; i < kPasses * kSel * kBins; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x == 0) {
        st->num_requests = rq.n;
        for (int r = 0; r < kMaxReq; ++r) {
            st->q[r] = rq.q[r];
            st->positive[r] = r < rq.n ? rq.positive[r] : 0;
            st->count[r] = 0u;
            st->frac[r] = 0.0;
        }
        for (int s = 0; s < kSel; ++s) {
            st->prefix[s] = 0u;
            st->rank[s] = 0u;
        }
        assign_slots(st);
    }
}

__global__ void __launch_bounds__(kThreads)
hist_kernel(const float* __restrict__ x, int64_t n, int pass, const State* __restrict__ st,
            uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[kSel * kBins];
    __shared__ uint32_t s_prefix[kSel];
    __shared__ int32_t s_positive[kSel];
    const int num_slots = st->num_slots;
    for (int i = threadIdx.x; i < num_slots * kBins; i += kThreads) bins[i] = 0u;
    if (threadIdx.x < num_slots) {
        const int sel = st->slot_sel[threadIdx.x];
        s_prefix[threadIdx.x] = st->prefix[sel];
        s_positive[threadIdx.x] = st->positive[sel >> 1];
    }
    __syncthreads();
    const int digit_shift = 24 - 8 * pass;
    auto add = [&](float v) {
        const uint32_t key = key_of(v);
        const uint32_t digit = (key >> digit_shift) & 255u;
        const uint32_t head = pass == 0 ? 0u : key >> (digit_shift + 8);
        for (int s = 0; s < num_slots; ++s) {
            if (head != s_prefix[s]) continue;
            if (s_positive[s] && key <= kKeyZero) continue;
            atomicAdd(&bins[s * kBins + digit], 1u);
        }
    };
    // scalar head up to 16-byte alignment, float4 body, scalar tail
    int64_t head = (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 4;
    if (((uintptr_t)x & 3) != 0 || head > n) head = n;
    const int64_t nvec = (n - head) / 4;
    const float4* xv = reinterpret_cast<const float4*>(x + head);
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    // the four values of a load mostly share a digit (neighbouring depths, and every element in pass
    // 0 matches): equal digits go out as one LDS atomic
    for (int64_t i = tid; i < nvec; i += stride) {
        const float4 v = xv[i];
        const uint32_t key[4] = {key_of(v.x), key_of(v.y), key_of(v.z), key_of(v.w)};
        for (int s = 0; s < num_slots; ++s) {
            uint32_t digit[4];
            bool live[4];
            for (int j = 0; j < 4; ++j) {
                const uint32_t head_j = pass == 0 ? 0u : key[j] >> (digit_shift + 8);
                digit[j] = (key[j] >> digit_shift) & 255u;
                live[j] = head_j == s_prefix[s] && !(s_positive[s] && key[j] <= kKeyZero);
            }
            for (int j = 0; j < 4; ++j) {
                if (!live[j]) continue;
                uint32_t c = 1u;
                for (int k = j + 1; k < 4; ++k)
                    if (live[k] && digit[k] == digit[j]) {
                        ++c;
                        live[k] = false;
                    }
                atomicAdd(&bins[s * kBins + digit[j]], c);
            }
        }
    }
    const int64_t tail0 = head + nvec * 4;
    for (int64_t i = tid; i < head + (n - tail0); i += stride) add(x[i < head ? i : tail0 + (i - head)]);
    __syncthreads();
    uint32_t* out = hist + (size_t)pass * kSel * kBins;
    for (int i = threadIdx.x; i < num_slots * kBins; i += kThreads) {
        const uint32_t c = bins[i];
        if (c) atomicAdd(&out[i], c);
    }
}

// One workgroup of one thread per bin: the histograms of all slots are prefix-summed in LDS, then the
// thread whose bin holds a selector's rank extends that selector's prefix (a serial walk of the bins
// by one thread per selector is up to 255 global loads, each waiting for the compare before it).
__global__ void __launch_bounds__(kBins)
pick_kernel(int pass, const uint32_t* __restrict__ hist, State* st, double* __restrict__ out) {
    __shared__ uint32_t scan[kSel][kBins];  // inclusive prefix sums per slot (unused slots are zero)
    __shared__ uint32_t s_rank[kSel];
    __shared__ int32_t s_slot[kSel];
    const int s = threadIdx.x;  // bin in the scan, selector / request index elsewhere
    const int ns = 2 * st->num_requests;
    const uint32_t* hp = hist + (size_t)pass * kSel * kBins;
    for (int u = 0; u < kSel; ++u) scan[u][s] = hp[u * kBins + s];
    __syncthreads();
    for (int off = 1; off < kBins; off <<= 1) {
        uint32_t add[kSel];
        for (int u = 0; u < kSel; ++u) add[u] = s >= off ? scan[u][s - off] : 0u;
        __syncthreads();
        for (int u = 0; u < kSel; ++u) scan[u][s] += add[u];
        __syncthreads();
    }
    if (pass == 0) {
        if (s < ns && (s & 1) == 0) {  // population size, position and the two ranks of request s / 2
            const int r = s >> 1;
            const uint32_t m = scan[st->slot[s]][kBins - 1];
            st->count[r] = m;
            if (m > 0u) {
                const double pos = st->q[r] * (double)(m - 1u);
                uint32_t k = (uint32_t)floor(pos);
                if (k > m - 1u) k = m - 1u;
                st->frac[r] = pos - (double)k;
                st->rank[s] = k;
                st->rank[s + 1] = k + 1u < m ? k + 1u : m - 1u;
            }
        }
        __syncthreads();
    }
    if (s < kSel) {
        s_rank[s] = st->rank[s];
        s_slot[s] = s < ns && st->count[s >> 1] > 0u ? st->slot[s] : -1;
    }
    __syncthreads();
    for (int u = 0; u < ns; ++u) {
        if (s_slot[u] < 0) continue;
        const uint32_t incl = scan[s_slot[u]][s], excl = s ? scan[s_slot[u]][s - 1] : 0u;
        if (s_rank[u] >= excl && s_rank[u] < incl) {  // one bin per selector
            st->prefix[u] = (st->prefix[u] << 8) | (uint32_t)s;
            st->rank[u] = s_rank[u] - excl;
        }
    }
    __syncthreads();
    if (pass < kPasses - 1) {
        if (s == 0) assign_slots(st);
        return;
    }
    if (s < st->num_requests) {
        double res = __longlong_as_double(0x7ff8000000000000LL);  // empty population: NaN
        if (st->count[s] > 0u) {
            const double lo = (double)value_of(st->prefix[2 * s]);
            const double hi = (double)value_of(st->prefix[2 * s + 1]);
            res = lo + (hi - lo) * st->frac[s];
        }
        out[s] = res;
    }
}

}  // namespace quantile
}  // namespace tsplat

extern "C" size_t tsplat_quantile_workspace_bytes(int32_t num_requests) {
    using namespace tsplat::quantile;
    if (num_requests < 1 || num_requests > kMaxReq) return 0;
    return hist_bytes() + tsplat::align_up(sizeof(State), 256);
}

extern "C" int tsplat_quantile_f32(const float* x, int64_t n, const double* q, const int32_t* positive_only,
                                   int32_t num_requests, double* out, void* workspace, void* stream_) {
    using namespace tsplat::quantile;
    if (!x || !q || !positive_only || !out || !workspace || n <= 0 || n > (int64_t)0x7fffffff || num_requests < 1 ||
        num_requests > kMaxReq)
        return TSPLAT_EINVAL;
    Requests rq = {};
    rq.n = num_requests;
    for (int r = 0; r < num_requests; ++r) {
        if (!(q[r] >= 0.0 && q[r] <= 1.0)) return TSPLAT_EINVAL;
        rq.q[r] = q[r];
        rq.positive[r] = positive_only[r] != 0;
    }
    hipStream_t stream = (hipStream_t)stream_;
    uint32_t* hist = reinterpret_cast<uint32_t*>(workspace);
    State* st = reinterpret_cast<State*>(reinterpret_cast<char*>(workspace) + hist_bytes());
    const int64_t want = (n + (int64_t)kThreads * 16 - 1) / ((int64_t)kThreads * 16);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, 2048));
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(kThreads), 0, stream, rq, hist, st);
    TSPLAT_CHECK_LAUNCH();
    for (int pass = 0; pass < kPasses; ++pass) {
        hipLaunchKernelGGL(hist_kernel, dim3(blocks), dim3(kThreads), 0, stream, x, n, pass, st, hist);
        TSPLAT_CHECK_LAUNCH();
        hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(kBins), 0, stream, pass, hist, st, out);
        TSPLAT_CHECK_LAUNCH();
    }
    return TSPLAT_OK;
}
