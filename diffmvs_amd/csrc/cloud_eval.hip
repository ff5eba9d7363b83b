// Point-cloud scoring (diffmvs_amd/cloud_eval.py): the two searches of the DTU / Tanks&Temples / ETH3D scorers and their reduction.
//
// dmvs_cloud_nn_dist_f32: min(|q - nearest target|, max_dist) per query, one lane per query.  The targets arrive sorted into a uniform
// grid of cell side h; key = (z << (bx + by)) | (y << bx) | x with power-of-two strides, so that cells adjacent in x are adjacent in
// key order and a key decodes by shifts.  `keys` lists the occupied cells ascending, `start` their first point.
// The walk is outward in rings: ring r is the slab pair z = cz -+ r.  Inside a slab the occupied rows (y) are walked outward from the
// query's row, inside a row the occupied cells (x) outward from the query's cell; every "next occupied row / cell" is one binary
// search in `keys` (the idiom of view_select.hip), so empty space costs a search, not a visit per cell.
// A slab, row or cell is left out -- and with it everything behind it in that direction -- when the squared gap between the query and
// its extent is at least best^2 (1 + 1e-5), best starting at max_dist.  After ring r every unseen point is farther than r h (in z
// alone), so a lane stops when its best distance is <= r h, at the latest at r h >= max_dist.  The gaps are computed in fp64 from the
// same fp64 cell coordinates floor((p - origin) / h) the Python layer sorted the targets by; the margin 1e-5 is far above the 4 * 2^-24
// relative rounding of an fp32 squared distance, so a pruned point can never beat the best one: the result is the minimum over ALL
// targets of the fp32 squared distance, whatever h is.
// Worst case: a query farther than max_dist from a surface that fills the search box visits up to (2R + 1)^2 rows, R = ceil(max_dist / h),
// two searches each.  The caller caps R by raising h (cloud_eval.nn_distance resolves near queries on a fine grid and the rest on a
// coarse one); R above DMVS_CLOUD_MAX_RINGS is refused.
// Differences, squares and the square root are fp32, without contraction (three roundings for the differences, three products, two sums,
// one root: at most 3.5 * 2^-24 relative).  Latency-bound divergent gather: the lever is locality (queries sorted by the same key, so
// neighbouring lanes search and read the same cells) and waves in flight, not LDS.
//
// dmvs_cloud_stats_f32: counts and the fixed-point sum of the distances.  Lanes accumulate u64 counters, waves reduce with shuffles, the
// workgroup through LDS, then ONE integer atomicAdd per counter per workgroup: integer sums are associative, so every metric is bitwise
// independent of launch order and grid shape (the rule of view_select.hip and the GroupNorm statistics).
#include "cloud_walk.h"      // the walk, shared with dmvs_cloud_nn_index_f32 (cloud_register.hip)

namespace {

#define CLOUD_MAX_T DMVS_CLOUD_MAX_THRESHOLDS
#define CLOUD_NCOUNT (3 + CLOUD_MAX_T)
struct CloudThresholds { float t[CLOUD_MAX_T]; };

__global__ void __launch_bounds__(DMVS_BLOCK)
cloud_stats_kernel(const float* __restrict__ dist, const uint8_t* __restrict__ valid, long N, float max_dist, CloudThresholds thr, int T, double scale,
                   unsigned long long* __restrict__ out) {
    CloudSums<CLOUD_NCOUNT> acc = {};
    unsigned long long &n_valid = acc.v[0], &n_in = acc.v[1], &sum = acc.v[2], *const below = acc.v + 3;
    const long stride = (long)gridDim.x * DMVS_BLOCK;
    for (long i = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x; i < N; i += stride) {
        if (valid && !valid[i]) continue;
        const float d = dist[i];
        ++n_valid;
        if (d < max_dist) {
            ++n_in;
            sum += (unsigned long long)rint((double)d * scale);
        }
#pragma unroll
        for (int t = 0; t < CLOUD_MAX_T; ++t) below[t] += d < thr.t[t] ? 1ull : 0ull;      // unused slots hold -inf
    }
    cloud_block_sum(acc, 3 + T, out);
}

}  // namespace

extern "C" int dmvs_cloud_nn_dist_f32(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys,
                                      const int64_t* cell_start, int64_t C, const double* origin, double h, const int32_t* dims,
                                      float max_dist, float* dist, int32_t* work, void* stream) {
    return cloud_nn_launch<false>(query, Q, target, M, cell_keys, cell_start, C, origin, h, dims, max_dist, nullptr, dist, nullptr, work, stream);
}

extern "C" int dmvs_cloud_stats_f32(const float* dist, const uint8_t* valid, int64_t N, float max_dist, const float* thresholds, int32_t T,
                                    double scale, int32_t blocks, uint64_t* out, void* stream) {
    if (N < 0 || T < 0 || T > CLOUD_MAX_T || !out || blocks < 0 || (N > 0 && !dist) || (T > 0 && !thresholds)) return DMVS_EINVAL;
    if (!(max_dist > 0.0f) || !isfinite(max_dist) || !cloud_pow2(scale) || !cloud_sum_fits(N, (double)max_dist, scale)) return DMVS_EINVAL;
    CloudThresholds thr;
    for (int t = 0; t < CLOUD_MAX_T; ++t) {
        thr.t[t] = t < T ? thresholds[t] : -INFINITY;
        if (t < T && !(thresholds[t] == thresholds[t])) return DMVS_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(out);
    const hipError_t err = hipMemsetAsync(acc, 0, (size_t)(3 + T) * sizeof(unsigned long long), s);
    if (err != hipSuccess) return (int)err;
    if (N == 0) return 0;
    dim3 grid(cloud_sum_blocks(N, blocks)), block(DMVS_BLOCK);
    hipLaunchKernelGGL(cloud_stats_kernel, grid, block, 0, s, dist, valid, (long)N, max_dist, thr, (int)T, scale, acc);
    return dmvs_launch_status();
}
