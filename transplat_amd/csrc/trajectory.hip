// Camera trajectory between two poses: interpolate_extrinsics of the reference
// (src/visualization/camera_trajectory/interpolation.py:204-252) as one launch, one thread per
// (pair, time step). The reference goes through torch.linalg.lstsq, boolean-mask indexing and
// scipy's Euler conversions on numpy (several host round trips); here every intermediate is a
// float64 register value and only the 16 outputs are rounded to fp32 (the reference rounds the
// interpolated parameters, the pivot frame and the pivot point to fp32 before converting back).
#include "common.h"

namespace tsplat {
namespace trajectory {

struct V3 {
    double x, y, z;
};

__device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 col(const double* m, int c) { return {m[c], m[4 + c], m[8 + c]}; }  // of a row-major 4x4

// columns (y x z, y, z): generate_coordinate_frame
struct Frame {
    V3 c0, c1, c2;
};
__device__ inline Frame coordinate_frame(V3 y, V3 z) { return {cross(y, z), y, z}; }

__device__ inline bool parallel(V3 a, V3 b, double eps) { return fabs(fabs(dot(a, b)) - 1.0) < eps; }

// 3x3 solve / inverse by the adjugate (rows r0, r1, r2)
__device__ inline void inverse3(const double m[9], double inv[9]) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    const double id = 1.0 / det;
    inv[0] = c00 * id;
    inv[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    inv[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    inv[3] = c01 * id;
    inv[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    inv[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    inv[6] = c02 * id;
    inv[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    inv[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// extrinsics_to_pivot_parameters: (translation in the frame (axis x look, axis, look), first and
// third intrinsic YXZ Euler angle of frame^-1 R)
__device__ inline void pivot_parameters(const double* e, const Frame& f, const double finv[9], V3 pivot, double p[5]) {
    const V3 look = col(e, 2), origin = col(e, 3);
    const Frame tf = coordinate_frame(f.c1, look);
    const V3 delta = sub(pivot, origin);
    p[0] = dot(tf.c0, delta);
    p[1] = dot(tf.c1, delta);
    p[2] = dot(tf.c2, delta);
    double m[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            m[3 * r + c] = finv[3 * r] * e[c] + finv[3 * r + 1] * e[4 + c] + finv[3 * r + 2] * e[8 + c];
    // M = Ry(a) Rx(b) Rz(g): M02 = sa cb, M22 = ca cb, M10 = cb sg, M11 = cb cg, M12 = -sb
    if (hypot(m[2], m[8]) < 1e-7) {  // gimbal lock: the third angle is set to zero
        p[3] = atan2(-m[6], m[0]);
        p[4] = 0.0;
    } else {
        p[3] = atan2(m[2], m[8]);
        p[4] = atan2(m[3], m[4]);
    }
}

__device__ inline double mod_tau(double a, double tau) {  // torch's remainder for a positive divisor
    double r = fmod(a, tau);
    if (r != 0.0 && r < 0.0) r += tau;
    return r;
}

// interpolate_circular: the nearest of a - tau, a, a + tau to b, ties resolved as the reference does
__device__ inline double lerp_circular(double a, double b, double t) {
    const double tau = 2.0 * 3.141592653589793;
    a = mod_tau(a, tau);
    b = mod_tau(b, tau);
    const double d = fabs(b - a);
    const double a_left = a - tau, d_left = fabs(b - a_left);
    const double a_right = a + tau, d_right = fabs(b - a_right);
    const bool use_d = d < d_left && d < d_right;
    const bool use_left = d_left < d_right && !use_d;
    const double a0 = use_d ? a : (use_left ? a_left : a_right);
    return a0 + (b - a0) * t;
}

__global__ void interpolate_kernel(const float* __restrict__ initial, const float* __restrict__ final_,
                                   const float* __restrict__ ts, double eps, int P, int T,
                                   float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * T) return;
    const int p = idx / T, ti = idx % T;
    double a[16], b[16];
    for (int i = 0; i < 16; ++i) {
        a[i] = (double)initial[(size_t)p * 16 + i];
        b[i] = (double)final_[(size_t)p * 16 + i];
    }
    const double t = (double)ts[ti];
    const V3 la = col(a, 2), lb = col(b, 2), oa = col(a, 3), ob = col(b, 3);

    // pivot point: midpoint of the origins for parallel looks, else the least-squares intersection
    // of the two look rays, (sum_i n_i n_i^T - I) p = sum_i (n_i n_i^T - I) o_i
    V3 pivot = {0.5 * (oa.x + ob.x), 0.5 * (oa.y + ob.y), 0.5 * (oa.z + ob.z)};
    if (!parallel(la, lb, eps)) {
        const double da[3] = {la.x, la.y, la.z}, db[3] = {lb.x, lb.y, lb.z};
        const double pa[3] = {oa.x, oa.y, oa.z}, pb[3] = {ob.x, ob.y, ob.z};
        double lhs[9], rhs[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double id = i == j ? 1.0 : 0.0;
                const double na = da[i] * da[j] - id, nb = db[i] * db[j] - id;
                lhs[3 * i + j] = na + nb;
                rhs[i] += na * pa[j] + nb * pb[j];
            }
        double inv[9];
        inverse3(lhs, inv);
        pivot = {inv[0] * rhs[0] + inv[1] * rhs[1] + inv[2] * rhs[2],
                 inv[3] * rhs[0] + inv[4] * rhs[1] + inv[5] * rhs[2],
                 inv[6] * rhs[0] + inv[7] * rhs[1] + inv[8] * rhs[2]};
    }

    // generate_rotation_coordinate_frame: Y normal to the plane of the two looks
    V3 bb = lb;
    if (parallel(la, bb, eps)) bb = {0.0, 0.0, 1.0};
    if (parallel(la, bb, eps)) bb = {0.0, 1.0, 0.0};
    V3 n = cross(la, bb);
    const double nn = sqrt(dot(n, n));
    n = {n.x / nn, n.y / nn, n.z / nn};
    const Frame f = coordinate_frame(n, la);
    const double fm[9] = {f.c0.x, f.c1.x, f.c2.x, f.c0.y, f.c1.y, f.c2.y, f.c0.z, f.c1.z, f.c2.z};
    double finv[9];
    inverse3(fm, finv);

    double pi[5], pf[5], q[5];
    pivot_parameters(a, f, finv, pivot, pi);
    pivot_parameters(b, f, finv, pivot, pf);
    for (int i = 0; i < 3; ++i) q[i] = pi[i] + (pf[i] - pi[i]) * t;
    q[3] = lerp_circular(pi[3], pf[3], t);
    q[4] = lerp_circular(pi[4], pf[4], t);

    // pivot_parameters_to_extrinsics: R = frame Ry(q3) Rz(q4)
    const double ca = cos(q[3]), sa = sin(q[3]), cg = cos(q[4]), sg = sin(q[4]);
    const double e[9] = {ca * cg, -ca * sg, sa, sg, cg, 0.0, -sa * cg, sa * sg, ca};
    double r[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            r[3 * i + j] = fm[3 * i] * e[j] + fm[3 * i + 1] * e[3 + j] + fm[3 * i + 2] * e[6 + j];
    const V3 look = {r[2], r[5], r[8]};
    const Frame tf = coordinate_frame(f.c1, look);
    const V3 origin = {pivot.x - (tf.c0.x * q[0] + tf.c1.x * q[1] + tf.c2.x * q[2]),
                       pivot.y - (tf.c0.y * q[0] + tf.c1.y * q[1] + tf.c2.y * q[2]),
                       pivot.z - (tf.c0.z * q[0] + tf.c1.z * q[1] + tf.c2.z * q[2])};
    float* o = out + (size_t)idx * 16;
    o[0] = (float)r[0], o[1] = (float)r[1], o[2] = (float)r[2], o[3] = (float)origin.x;
    o[4] = (float)r[3], o[5] = (float)r[4], o[6] = (float)r[5], o[7] = (float)origin.y;
    o[8] = (float)r[6], o[9] = (float)r[7], o[10] = (float)r[8], o[11] = (float)origin.z;
    o[12] = 0.f, o[13] = 0.f, o[14] = 0.f, o[15] = 1.f;
}

}  // namespace trajectory
}  // namespace tsplat

extern "C" int tsplat_trajectory_extrinsics(const float* initial, const float* final_, const float* t, double eps,
                                            int32_t num_pairs, int32_t num_steps, float* out, void* stream_) {
    if (!initial || !final_ || !t || !out || num_pairs <= 0 || num_steps <= 0 ||
        (int64_t)num_pairs * num_steps > (int64_t)1 << 24)
        return TSPLAT_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    const int n = num_pairs * num_steps;
    hipLaunchKernelGGL(tsplat::trajectory::interpolate_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, initial,
                       final_, t, eps, num_pairs, num_steps, out);
    TSPLAT_CHECK_LAUNCH();
    return TSPLAT_OK;
}
