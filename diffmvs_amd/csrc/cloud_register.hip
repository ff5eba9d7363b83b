// Registration and cropping of point clouds (diffmvs_amd/cloud_register.py): what has to happen before cloud_eval's scores mean anything
// when the two clouds do not already share a frame (a COLMAP reconstruction, Tanks&Temples, ETH3D).
//
// dmvs_cloud_nn_index_f32: the walk of dmvs_cloud_nn_dist_f32 (cloud_walk.h, described in cloud_eval.hip) instantiated with INDEX = true:
// one more register holds the position of the best target so far.  The query may be moved by a similarity first: q' = fp32(sR q + t),
// products and sums in fp64, ONE rounding -- so that the host can restate q' exactly and the moved cloud never has to exist in memory.
//
// dmvs_cloud_pair_moments_f64: everything one point-to-point ICP step needs from the pairs (i, index[i]), in ONE pass over the source:
// the count, sum p, sum t, sum p t^T, sum |p|^2, sum |t|^2, sum |q' - target|^2 with p = q' - center_p, t = target - center_q in fp64.
// Streaming: 12 bytes of source, 4 of index, (1 of mask) and one 12-byte gather per point; the source is sorted by grid key, so the lanes of
// a wave gather neighbouring targets.  The reduction is the project's: every term is rint(value * 2^k) as a signed 64-bit integer, added
// in two's complement through unsigned long long -- lanes, wave shuffles, LDS, then ONE integer atomicAdd per counter per workgroup --
// so all 20 outputs are bitwise independent of the grid shape, `blocks` and the order of the points.
// Why the centres: the fixed point has to hold N * max|term| below 2^62.  Uncentred DTU coordinates (10^3) with 10^7 points would leave
// 2^62 / (10^7 * 3 * 10^6) ~ 2^17 per unit for the quadratic sums while the quantities that matter -- the covariance about the centroids --
// are differences of those sums; centred on the box the coordinates are bounded by the half-extent B, the scale is the largest power of two
// below 2^62 / (N * 3 B^2), one term is rounded by at most 0.5 / scale and a sum of n terms by n * 0.5 / scale: for N = 10^7, B = 500
// that is scale 2^19, at most 10 units on sums of order N B^2 / 3 ~ 10^12 (1e-11 relative; fp64 itself carries 1e-16 * sqrt(N)).  The
// linear sums take their own, finer scale (2^62 / (N B): 2^29).  A pair whose p or t leaves the bound is NOT summed but counted in out[19],
// which the caller treats as an error: nothing overflows silently.
//
// dmvs_cloud_crop_prism_f32: the crop volume of a Tanks&Temples scene (SelectionPolygonVolume): an interval along one axis and a polygon in
// the plane of the other two, even-odd rule.  One lane per point, the polygon staged once per workgroup in LDS (at most
// DMVS_CLOUD_MAX_POLYGON vertices: 4 KiB); every lane walks all edges, so LDS reads are broadcasts.  All fp64 in a fixed operation order.
#include "cloud_walk.h"

namespace {

#define CLOUD_NMOM DMVS_CLOUD_MOMENTS
struct CloudMomentArgs {
    double cp[3], cq[3];       // the centres
    double bound, s1, s2;      // coordinate bound, scale of the linear sums, scale of the quadratic sums
    float max_corr;
};

__device__ __forceinline__ unsigned long long cloud_fix(double v) { return (unsigned long long)(long long)rint(v); }

__global__ void __launch_bounds__(DMVS_BLOCK)
cloud_pair_moments_kernel(const float* __restrict__ source, long N, CloudTransform T, const float* __restrict__ target, long M,
                          const int32_t* __restrict__ index, const uint8_t* __restrict__ valid, CloudMomentArgs a,
                          unsigned long long* __restrict__ out) {
#pragma clang fp contract(off)
    CloudSums<CLOUD_NMOM> sums = {};
    unsigned long long* const acc = sums.v;
    const long stride = (long)gridDim.x * DMVS_BLOCK;
    for (long i = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x; i < N; i += stride) {
        const long j = index[i];
        if (j < 0 || (valid && !valid[i])) continue;
        if (j >= M) {                                       // not an index into this target: never dereferenced
            ++acc[19];
            continue;
        }
        float qx = source[3 * i], qy = source[3 * i + 1], qz = source[3 * i + 2];
        cloud_move(T, qx, qy, qz);
        const float* t = target + 3 * j;
        const float tx = t[0], ty = t[1], tz = t[2];
        const float ex = qx - tx, ey = qy - ty, ez = qz - tz;
        const float d = sqrtf((ex * ex + ey * ey) + ez * ez);                // the distance of the search, bit for bit
        if (!(d <= a.max_corr)) continue;
        const double p0 = (double)qx - a.cp[0], p1 = (double)qy - a.cp[1], p2 = (double)qz - a.cp[2];
        const double t0 = (double)tx - a.cq[0], t1 = (double)ty - a.cq[1], t2 = (double)tz - a.cq[2];
        const double big = fmax(fmax(fmax(fabs(p0), fabs(p1)), fabs(p2)), fmax(fmax(fabs(t0), fabs(t1)), fabs(t2)));
        if (!(big <= a.bound)) {                            // (NaN as well) beyond what the fixed point was sized for
            ++acc[19];
            continue;
        }
        const double r0 = (double)qx - (double)tx, r1 = (double)qy - (double)ty, r2 = (double)qz - (double)tz;
        acc[0] += 1ull;
        acc[1] += cloud_fix(p0 * a.s1), acc[2] += cloud_fix(p1 * a.s1), acc[3] += cloud_fix(p2 * a.s1);
        acc[4] += cloud_fix(t0 * a.s1), acc[5] += cloud_fix(t1 * a.s1), acc[6] += cloud_fix(t2 * a.s1);
        acc[7] += cloud_fix(p0 * t0 * a.s2), acc[8] += cloud_fix(p0 * t1 * a.s2), acc[9] += cloud_fix(p0 * t2 * a.s2);
        acc[10] += cloud_fix(p1 * t0 * a.s2), acc[11] += cloud_fix(p1 * t1 * a.s2), acc[12] += cloud_fix(p1 * t2 * a.s2);
        acc[13] += cloud_fix(p2 * t0 * a.s2), acc[14] += cloud_fix(p2 * t1 * a.s2), acc[15] += cloud_fix(p2 * t2 * a.s2);
        acc[16] += cloud_fix(((p0 * p0 + p1 * p1) + p2 * p2) * a.s2);
        acc[17] += cloud_fix(((t0 * t0 + t1 * t1) + t2 * t2) * a.s2);
        acc[18] += cloud_fix(((r0 * r0 + r1 * r1) + r2 * r2) * a.s2);
    }
    cloud_block_sum(sums, CLOUD_NMOM, out);
}

struct CloudPrism {
    double lo, hi;             // the interval along w, both ends included
    int u, v, w, K;            // coordinate indices and the number of vertices
};

__global__ void __launch_bounds__(DMVS_BLOCK)
cloud_crop_prism_kernel(const float* __restrict__ points, long N, CloudTransform T, const double* __restrict__ polygon, CloudPrism P,
                        uint8_t* __restrict__ inside) {
#pragma clang fp contract(off)
    __shared__ double pu[DMVS_CLOUD_MAX_POLYGON], pv[DMVS_CLOUD_MAX_POLYGON];
    for (int k = threadIdx.x; k < P.K; k += DMVS_BLOCK) pu[k] = polygon[2 * k], pv[k] = polygon[2 * k + 1];
    __syncthreads();
    const long i = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (i >= N) return;
    float c[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    cloud_move(T, c[0], c[1], c[2]);
    const double u = (double)(P.u == 0 ? c[0] : (P.u == 1 ? c[1] : c[2]));
    const double v = (double)(P.v == 0 ? c[0] : (P.v == 1 ? c[1] : c[2]));
    const double w = (double)(P.w == 0 ? c[0] : (P.w == 1 ? c[1] : c[2]));
    bool in = false;
    for (int k = 0, j = P.K - 1; k < P.K; j = k++) {
        const double ui = pu[k], vi = pv[k], uj = pu[j], vj = pv[j];
        if ((vi > v) != (vj > v)) {                         // (so vj != vi: the division is defined)
            const double cross = (uj - ui) * (v - vi) / (vj - vi) + ui;
            if (u < cross) in = !in;
        }
    }
    inside[i] = (uint8_t)((in && w >= P.lo && w <= P.hi) ? 1 : 0);
}

}  // namespace

extern "C" int dmvs_cloud_nn_index_f32(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys,
                                       const int64_t* cell_start, int64_t C, const double* origin, double h, const int32_t* dims,
                                       float max_dist, const double* transform, float* dist, int32_t* index, int32_t* work, void* stream) {
    return cloud_nn_launch<true>(query, Q, target, M, cell_keys, cell_start, C, origin, h, dims, max_dist, transform, dist, index, work, stream);
}

extern "C" int dmvs_cloud_pair_moments_f64(const float* source, int64_t N, const double* transform, const float* target, int64_t M,
                                           const int32_t* index, const uint8_t* valid, float max_corr, const double* center_p,
                                           const double* center_q, double bound, double scale_linear, double scale_quadratic, int32_t blocks,
                                           int64_t* out, void* stream) {
    if (N < 0 || M < 0 || M > 2147483647L || !out || blocks < 0 || !center_p || !center_q) return DMVS_EINVAL;
    if (N > 0 && (!source || !index)) return DMVS_EINVAL;
    if (N > 0 && M > 0 && !target) return DMVS_EINVAL;
    if (!(max_corr > 0.0f) || !isfinite(max_corr) || !(bound > 0.0) || !isfinite(bound)) return DMVS_EINVAL;
    if (!cloud_pow2(scale_linear) || !cloud_pow2(scale_quadratic)) return DMVS_EINVAL;
    CloudMomentArgs a;
    for (int k = 0; k < 3; ++k) {
        a.cp[k] = center_p[k], a.cq[k] = center_q[k];
        if (!isfinite(a.cp[k]) || !isfinite(a.cq[k])) return DMVS_EINVAL;
    }
    // no sum can reach 2^62: |p_k|, |t_k| <= bound, so |p|^2, |t|^2, |p_a t_b| <= 3 bound^2, and a counted pair is at most max_corr apart
    const double mc = (double)max_corr * 1.001;
    if (!cloud_sum_fits(N, bound, scale_linear) || !cloud_sum_fits(N, fmax(3.0 * bound * bound, mc * mc), scale_quadratic)) return DMVS_EINVAL;
    CloudTransform T;
    if (cloud_transform_arg(transform, T) != 0) return DMVS_EINVAL;
    a.bound = bound, a.s1 = scale_linear, a.s2 = scale_quadratic, a.max_corr = max_corr;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(out);
    const hipError_t err = hipMemsetAsync(acc, 0, (size_t)CLOUD_NMOM * sizeof(unsigned long long), s);
    if (err != hipSuccess) return (int)err;
    if (N == 0) return 0;
    dim3 grid(cloud_sum_blocks(N, blocks)), block(DMVS_BLOCK);
    hipLaunchKernelGGL(cloud_pair_moments_kernel, grid, block, 0, s, source, (long)N, T, target, (long)M, index, valid, a, acc);
    return dmvs_launch_status();
}

extern "C" int dmvs_cloud_crop_prism_f32(const float* points, int64_t N, const double* transform, const double* polygon, int32_t K,
                                         int32_t axis, double axis_min, double axis_max, uint8_t* inside, void* stream) {
    if (N < 0 || K < 3 || K > DMVS_CLOUD_MAX_POLYGON || !polygon || axis < 0 || axis > 2) return DMVS_EINVAL;
    if (N > 0 && (!points || !inside)) return DMVS_EINVAL;
    if (!(axis_min <= axis_max)) return DMVS_EINVAL;       // (NaN as well; infinite ends are allowed: no limit on that side)
    if (dmvs_ceil_div(N, DMVS_BLOCK) > (1u << 30) || N > (1L << 38)) return DMVS_EINVAL;
    CloudTransform T;
    if (cloud_transform_arg(transform, T) != 0) return DMVS_EINVAL;
    if (N == 0) return 0;
    CloudPrism P;
    P.lo = axis_min, P.hi = axis_max, P.K = K, P.w = axis;
    P.u = axis == 0 ? 1 : 0, P.v = axis == 2 ? 1 : 2;      // (u, v, w) = (1,2,0) for X, (0,2,1) for Y, (0,1,2) for Z
    dim3 grid(dmvs_ceil_div(N, DMVS_BLOCK)), block(DMVS_BLOCK);
    hipLaunchKernelGGL(cloud_crop_prism_kernel, grid, block, 0, (hipStream_t)stream, points, (long)N, T, polygon, P, inside);
    return dmvs_launch_status();
}
