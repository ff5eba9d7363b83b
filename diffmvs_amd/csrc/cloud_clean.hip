// Point-cloud cleaning (diffmvs_amd/cloud_clean.py): the k-nearest search both outlier filters stand on.
//
// dmvs_cloud_knn_f32: the walk of dmvs_cloud_nn_dist_f32 (cloud_walk.h, described in cloud_eval.hip) with a collector that keeps the k
// smallest squared distances instead of the single smallest.  One lane per query; the prune bound of the walk is the k-th best so far
// (max_dist^2 until the list is full), under the same kPruneMargin rule, so a pruned target can never enter the list: the list is the k
// smallest of ALL candidates' fp32 squared distances, a multiset that does not depend on the walk order, hence not on the cell size.
//
// The list lives in registers.  A per-lane array indexed by a run-time value goes to scratch on gfx950 and would turn every tested target
// into memory traffic, so the capacity KB is a template bound (8, 16, 32; run-time k <= KB) and every access is a fully unrolled loop with
// constant indices.  The list is kept ascending in the LAST k slots; the KB - k slots in front of them hold -inf, which nothing displaces.
// That puts the k-th best -- the bound -- always in slot KB - 1: no select over the slots is needed to read it, whatever k is.
// A tested target is first compared against the bound (one compare; most fail it, and the whole wave skips the insertion when all do);
// an accepted one is inserted by KB compare / select steps that carry the larger value upward, the last carry (the old k-th best) dropped.
//
// The statistical filter needs the MEAN distance to the k nearest: the roots are taken in fp64 and summed in ascending order, one
// rounding to fp32 at the end, so that a host restatement reproduces it bit for bit.
#include "cloud_walk.h"

namespace {

template <int KB>
struct CloudKBest {
    float d[KB];                // [KB - k, KB): the k smallest candidates so far, ascending, padded with max_dist^2;  [0, KB - k): -inf
    int self;                   // the target that is the query itself (-1: none)
    __device__ __forceinline__ float bound() const { return d[KB - 1]; }
    __device__ __forceinline__ void take(float d2, long p) {
        if (!(d2 < d[KB - 1]) || p == (long)self) return;
        float v = d2;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const bool below = v < d[j];
            const float up = below ? d[j] : v;
            d[j] = below ? v : d[j];
            v = up;
        }
    }
};

template <int KB>
__global__ void __launch_bounds__(DMVS_BLOCK)
cloud_knn_kernel(const float* __restrict__ query, long Q, const float* __restrict__ target, CloudGrid g, float max_dist,
                 const int32_t* __restrict__ self_index, int k, float* __restrict__ d2_out, float* __restrict__ kth, float* __restrict__ mean,
                 int32_t* __restrict__ found, int32_t* __restrict__ work) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (i >= Q) return;
    CloudQuery q;
    q.qx = query[3 * i], q.qy = query[3 * i + 1], q.qz = query[3 * i + 2];
    const float md2 = max_dist * max_dist;
    CloudKBest<KB> col;
    col.self = self_index ? self_index[i] : -1;
#pragma unroll
    for (int j = 0; j < KB; ++j) col.d[j] = j < KB - k ? -INFINITY : md2;
    const int rings = cloud_walk(q, col, g, target);

    int n = 0;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        if (j < KB - k) continue;
        const float v = col.d[j];
        if (v < md2) {
            ++n;
            sum += sqrt((double)v);
        }
        if (d2_out) d2_out[i * k + (j - (KB - k))] = v;
    }
    found[i] = n;
    kth[i] = n == k ? sqrtf(col.d[KB - 1]) : max_dist;
    mean[i] = n > 0 ? (float)(sum / (double)n) : max_dist;
    if (work) {
        work[2 * i] = rings;
        work[2 * i + 1] = q.points;
    }
}

template <int KB>
void cloud_knn_launch(dim3 grid, hipStream_t s, const float* query, long Q, const float* target, const CloudGrid& g, float max_dist,
                      const int32_t* self_index, int k, float* d2_out, float* kth, float* mean, int32_t* found, int32_t* work) {
    hipLaunchKernelGGL(cloud_knn_kernel<KB>, grid, dim3(DMVS_BLOCK), 0, s, query, Q, target, g, max_dist, self_index, k, d2_out, kth, mean, found, work);
}

}  // namespace

extern "C" int dmvs_cloud_knn_f32(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys,
                                  const int64_t* cell_start, int64_t C, const double* origin, double h, const int32_t* dims,
                                  float max_dist, const int32_t* self_index, int32_t k, float* d2_out, float* kth, float* mean,
                                  int32_t* found, int32_t* work, void* stream) {
    if (k < 1 || k > DMVS_CLOUD_MAX_K) return DMVS_EINVAL;
    if (Q > 0 && (!query || !kth || !mean || !found)) return DMVS_EINVAL;
    if (M > 2147483647L) return DMVS_EINVAL;               // self_index is 32 bits
    CloudGrid g;
    const int rc = cloud_grid_args(Q, M, target, cell_keys, cell_start, C, origin, h, dims, max_dist, g);
    if (rc != 0) return rc;
    if (Q == 0) return 0;
    const dim3 grid(dmvs_ceil_div(Q, DMVS_BLOCK));
    hipStream_t s = (hipStream_t)stream;
    if (k <= 8) cloud_knn_launch<8>(grid, s, query, (long)Q, target, g, max_dist, self_index, k, d2_out, kth, mean, found, work);
    else if (k <= 16) cloud_knn_launch<16>(grid, s, query, (long)Q, target, g, max_dist, self_index, k, d2_out, kth, mean, found, work);
    else cloud_knn_launch<32>(grid, s, query, (long)Q, target, g, max_dist, self_index, k, d2_out, kth, mean, found, work);
    return dmvs_launch_status();
}
