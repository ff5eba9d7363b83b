// View selection of the COLMAP import (reference colmap_input.py:374-390 calc_score): the score of an image pair is the sum,
// over the 3-D points both images list, of a Gaussian of the triangulation angle at the point.  The reference loops over image
// pairs and tests list membership in Python (O(N^2 L^2)); here every point adds one term to every pair of the images that see it.
// One lane per (point, image pair) term: the pairs of all points are flattened by a prefix sum (pair_offsets), so a track of
// length 300 is 44850 lanes, not one lane walking them.  Terms are rounded to u64 fixed point (f * 2^40) and summed with integer
// atomics into the upper triangle (a positive term at least 1 unit): integer adds are associative, so the matrix does not depend on launch order or shape.
// A second pass converts to fp64 and mirrors.
#include <math.h>
#include "dmvs_common.h"

namespace {

constexpr double kFixedScale = 1099511627776.0;            // 2^40
constexpr double kFixedInv = 1.0 / 1099511627776.0;

__device__ __forceinline__ long tri_index(int a, int b) { return (long)b * (b - 1) / 2 + a; }      // a < b

// term of one point for the pair (ci, cj), in the reference's operation order (no contraction: numpy does not fuse)
__device__ __forceinline__ double angle_term(double px, double py, double pz, const double* __restrict__ ci, const double* __restrict__ cj,
                                             double theta0, double sigma1, double sigma2) {
#pragma clang fp contract(off)
    const double ax = ci[0] - px, ay = ci[1] - py, az = ci[2] - pz;
    const double bx = cj[0] - px, by = cj[1] - py, bz = cj[2] - pz;
    const double na = sqrt(ax * ax + ay * ay + az * az), nb = sqrt(bx * bx + by * by + bz * bz);
    if (na == 0.0 || nb == 0.0) return 0.0;                 // deviation 2: a point at a camera centre contributes nothing
    double c = (ax * bx + ay * by + az * bz) / na / nb;
    c = fmin(1.0, fmax(-1.0, c));                           // deviation 1: the reference's arccos gives NaN past +-1
    const double theta = (180.0 / M_PI) * acos(c);
    const double s = theta <= theta0 ? sigma1 : sigma2;
    const double d = theta - theta0;
    return exp(-d * d / (2.0 * (s * s)));
}

__global__ void __launch_bounds__(DMVS_BLOCK)
view_select_terms_kernel(const double* __restrict__ xyz, const int64_t* __restrict__ offsets, const int32_t* __restrict__ images,
                         const int32_t* __restrict__ mult, const int64_t* __restrict__ pair_offsets, long P, long terms,
                         const double* __restrict__ centres, int N, double theta0, double sigma1, double sigma2,
                         unsigned long long* __restrict__ acc) {
    const long stride = (long)gridDim.x * DMVS_BLOCK;
    for (long g = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x; g < terms; g += stride) {
        long lo = 0, hi = P - 1;                            // the point: last p with pair_offsets[p] <= g
        while (lo < hi) {
            const long mid = (lo + hi + 1) >> 1;
            if (pair_offsets[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const long p = lo;
        const long t = g - pair_offsets[p];
        // pairs of a point in column order: (k, l), k < l, at t = l (l - 1) / 2 + k
        long l = (long)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
        while (l * (l - 1) / 2 > t) --l;
        while ((l + 1) * l / 2 <= t) ++l;
        const long k = t - l * (l - 1) / 2;
        const long e0 = offsets[p];
        if (e0 < 0 || e0 + l >= offsets[p + 1]) continue;   // pair_offsets inconsistent with offsets: nothing is written
        const int a = images[e0 + k], b = images[e0 + l], m = mult[e0 + k];
        if (a < 0 || a >= b || b >= N || m <= 0) continue;  // image lists must be ascending and unique within a point
        const double f = angle_term(xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2], centres + 3 * a, centres + 3 * b, theta0, sigma1, sigma2);
        if (!(f > 0.0)) continue;
        // a positive term stays positive (at least 2^-40): a pair the reference scores above zero never ties with an unrelated pair
        const double r = rint(f * kFixedScale);
        const unsigned long long q = r < 1.0 ? 1ull : (unsigned long long)r;
        atomicAdd(acc + tri_index(a, b), q * (unsigned long long)m);
    }
}

__global__ void __launch_bounds__(DMVS_BLOCK)
view_select_finish_kernel(const unsigned long long* __restrict__ acc, double* __restrict__ score, int N) {
    const long e = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (e >= (long)N * N) return;
    const int i = (int)(e / N), j = (int)(e - (long)i * N);
    score[e] = i == j ? 0.0 : (double)acc[i < j ? tri_index(i, j) : tri_index(j, i)] * kFixedInv;
}

}  // namespace

extern "C" int dmvs_view_select_scores_f64(const double* xyz, const int64_t* offsets, const int32_t* images, const int32_t* mult,
                                           const int64_t* pair_offsets, int64_t P, int64_t terms, const double* centres, int32_t N,
                                           double theta0, double sigma1, double sigma2, uint64_t* workspace, double* score, void* stream) {
    if (!centres || !score || N < 1 || N > DMVS_VIEW_SELECT_MAX_IMAGES || P < 0 || terms < 0) return DMVS_EINVAL;
    if (!(sigma1 > 0.0) || !(sigma2 > 0.0) || !isfinite(theta0) || !isfinite(sigma1) || !isfinite(sigma2)) return DMVS_EINVAL;
    const long tri = (long)N * (N - 1) / 2;
    if (terms > 0 && (P < 1 || !xyz || !offsets || !images || !mult || !pair_offsets)) return DMVS_EINVAL;
    if (tri > 0 && !workspace) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(workspace);
    if (tri > 0) {
        const hipError_t e = hipMemsetAsync(acc, 0, (size_t)tri * sizeof(unsigned long long), s);
        if (e != hipSuccess) return (int)e;
    }
    if (terms > 0) {
        const long blocks = (terms + DMVS_BLOCK - 1) / DMVS_BLOCK;      // a grid-stride loop past 2^20 workgroups
        dim3 grid((unsigned)(blocks < (1L << 20) ? blocks : (1L << 20))), block(DMVS_BLOCK);
        hipLaunchKernelGGL(view_select_terms_kernel, grid, block, 0, s, xyz, offsets, images, mult, pair_offsets, (long)P, (long)terms, centres,
                           (int)N, theta0, sigma1, sigma2, acc);
        if (int rc = dmvs_launch_status()) return rc;
    }
    dim3 grid(dmvs_ceil_div((long)N * N, DMVS_BLOCK)), block(DMVS_BLOCK);
    hipLaunchKernelGGL(view_select_finish_kernel, grid, block, 0, s, acc, score, (int)N);
    return dmvs_launch_status();
}
