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
#include <math.h>
#include "dmvs_common.h"

namespace {

struct CloudGrid {
    const int64_t* keys;       // [C] occupied cells, ascending
    const int64_t* start;      // [C + 1] first target of each cell
    long C;
    double ox, oy, oz, h;
    int nx, ny, nz, bx, by;
};

// first index in [lo, hi) whose key is >= k (hi if none)
__device__ __forceinline__ long cloud_lower_bound(const int64_t* __restrict__ keys, long lo, long hi, int64_t k) {
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// gap, in cells, between a query at offset t (cells, relative to its own cell's lower face) and the cell at integer offset d
__device__ __forceinline__ double cloud_gap(int d, double t) { return fmax(0.0, fmax((double)d - t, t - (double)(d + 1))); }

constexpr float kPruneMargin = 1.00001f;

struct CloudQuery {
    float qx, qy, qz;
    double tx, ty, tz;          // position inside the (clamped) own cell, in cells
    int cx, cy, cz;
    float best2;
    int points;                 // targets tested (the optional work output)
};

__device__ __forceinline__ void cloud_scan_cell(CloudQuery& q, const CloudGrid& g, const float* __restrict__ target, long c) {
#pragma clang fp contract(off)
    const long p0 = g.start[c], p1 = g.start[c + 1];
    for (long p = p0; p < p1; ++p) {
        const float dx = q.qx - target[3 * p], dy = q.qy - target[3 * p + 1], dz = q.qz - target[3 * p + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        q.best2 = d2 < q.best2 ? d2 : q.best2;
    }
    q.points += (int)(p1 - p0);
}

// one occupied row (y, z): its cells outward from the query's x; g2yz = squared gap of the row (length units)
__device__ __forceinline__ void cloud_visit_row(CloudQuery& q, const CloudGrid& g, const float* __restrict__ target, int y, int z, float g2yz) {
    const int64_t row = ((int64_t)z << g.by) | y, base = row << g.bx;
    const long cm = cloud_lower_bound(g.keys, 0, g.C, base | q.cx);
    for (long c = cm; c < g.C; ++c) {                      // x >= cx
        const int64_t k = g.keys[c];
        if ((k >> g.bx) != row) break;
        const float gx = (float)(cloud_gap((int)(k - base) - q.cx, q.tx) * g.h);
        if (gx * gx + g2yz >= q.best2 * kPruneMargin) break;
        cloud_scan_cell(q, g, target, c);
    }
    for (long c = cm - 1; c >= 0; --c) {                   // x < cx
        const int64_t k = g.keys[c];
        if ((k >> g.bx) != row) break;
        const float gx = (float)(cloud_gap((int)(k - base) - q.cx, q.tx) * g.h);
        if (gx * gx + g2yz >= q.best2 * kPruneMargin) break;
        cloud_scan_cell(q, g, target, c);
    }
}

// one slab z: its occupied rows outward from the query's y
__device__ __forceinline__ void cloud_visit_slab(CloudQuery& q, const CloudGrid& g, const float* __restrict__ target, int z, float g2z) {
    const int sh = g.bx + g.by;
    const int64_t ymask = ((int64_t)1 << g.by) - 1;
    for (int y = q.cy; y < g.ny;) {                        // rows >= cy: the first occupied row at or after y
        const long c = cloud_lower_bound(g.keys, 0, g.C, (((int64_t)z << g.by) | y) << g.bx);
        if (c >= g.C) break;
        const int64_t k = g.keys[c];
        if ((k >> sh) != z) break;
        const int yo = (int)((k >> g.bx) & ymask);
        const float gy = (float)(cloud_gap(yo - q.cy, q.ty) * g.h);
        const float g2 = gy * gy + g2z;
        if (g2 >= q.best2 * kPruneMargin) break;
        cloud_visit_row(q, g, target, yo, z, g2);
        y = yo + 1;
    }
    for (int y = q.cy - 1; y >= 0;) {                      // rows < cy: the last occupied row at or before y
        const long c = cloud_lower_bound(g.keys, 0, g.C, (((int64_t)z << g.by) | (y + 1)) << g.bx) - 1;
        if (c < 0) break;
        const int64_t k = g.keys[c];
        if ((k >> sh) != z) break;
        const int yo = (int)((k >> g.bx) & ymask);
        const float gy = (float)(cloud_gap(yo - q.cy, q.ty) * g.h);
        const float g2 = gy * gy + g2z;
        if (g2 >= q.best2 * kPruneMargin) break;
        cloud_visit_row(q, g, target, yo, z, g2);
        y = yo - 1;
    }
}

__device__ __forceinline__ int cloud_clamp_cell(double u, int n) {
    const double f = floor(u);
    return f < 0.0 ? 0 : (f > (double)(n - 1) ? n - 1 : (int)f);      // (u is finite: checked by the caller)
}

__global__ void __launch_bounds__(DMVS_BLOCK)
cloud_nn_dist_kernel(const float* __restrict__ query, long Q, const float* __restrict__ target, CloudGrid g, float max_dist,
                     float* __restrict__ dist, int32_t* __restrict__ work) {
    const long i = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (i >= Q) return;
    CloudQuery q;
    q.qx = query[3 * i], q.qy = query[3 * i + 1], q.qz = query[3 * i + 2];
    const double ux = ((double)q.qx - g.ox) / g.h, uy = ((double)q.qy - g.oy) / g.h, uz = ((double)q.qz - g.oz) / g.h;
    int rings = 0;
    q.points = 0;
    q.best2 = max_dist * max_dist;
    if (g.C > 0 && isfinite(ux) && isfinite(uy) && isfinite(uz)) {
        q.cx = cloud_clamp_cell(ux, g.nx), q.cy = cloud_clamp_cell(uy, g.ny), q.cz = cloud_clamp_cell(uz, g.nz);
        q.tx = ux - q.cx, q.ty = uy - q.cy, q.tz = uz - q.cz;
        bool up = true, down = true;
        for (int r = 0; up || down; ++r) {
            rings = r + 1;
            if (up) {
                const int z = q.cz + r;
                const float gz = (float)(cloud_gap(r, q.tz) * g.h);
                if (z >= g.nz || gz * gz >= q.best2 * kPruneMargin) up = false;
                else cloud_visit_slab(q, g, target, z, gz * gz);
            }
            if (r == 0) continue;
            if (down) {
                const int z = q.cz - r;
                const float gz = (float)(cloud_gap(-r, q.tz) * g.h);
                if (z < 0 || gz * gz >= q.best2 * kPruneMargin) down = false;
                else cloud_visit_slab(q, g, target, z, gz * gz);
            }
        }
    }
    const float d = sqrtf(q.best2);
    dist[i] = q.best2 < max_dist * max_dist ? fminf(d, max_dist) : max_dist;
    if (work) {
        work[2 * i] = rings;
        work[2 * i + 1] = q.points;
    }
}

#define CLOUD_MAX_T DMVS_CLOUD_MAX_THRESHOLDS
#define CLOUD_NCOUNT (3 + CLOUD_MAX_T)
struct CloudThresholds { float t[CLOUD_MAX_T]; };

__global__ void __launch_bounds__(DMVS_BLOCK)
cloud_stats_kernel(const float* __restrict__ dist, const uint8_t* __restrict__ valid, long N, float max_dist, CloudThresholds thr, int T, double scale,
                   unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[DMVS_BLOCK / 64][CLOUD_NCOUNT];
    unsigned long long n_valid = 0, n_in = 0, sum = 0, below[CLOUD_MAX_T];
#pragma unroll
    for (int t = 0; t < CLOUD_MAX_T; ++t) below[t] = 0;
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
    for (int off = 32; off > 0; off >>= 1) {
        n_valid += __shfl_down(n_valid, off);
        n_in += __shfl_down(n_in, off);
        sum += __shfl_down(sum, off);
#pragma unroll
        for (int t = 0; t < CLOUD_MAX_T; ++t) below[t] += __shfl_down(below[t], off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = n_valid, part[wave][1] = n_in, part[wave][2] = sum;
#pragma unroll
        for (int t = 0; t < CLOUD_MAX_T; ++t) part[wave][3 + t] = below[t];
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 + T) {
        unsigned long long v = 0;
        for (int w = 0; w < DMVS_BLOCK / 64; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(out + threadIdx.x, v);
    }
}

int cloud_bits(long n) {
    int b = 0;
    while ((1L << b) < n) ++b;
    return b;
}

}  // namespace

extern "C" int dmvs_cloud_nn_dist_f32(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys,
                                      const int64_t* cell_start, int64_t C, const double* origin, double h, const int32_t* dims,
                                      float max_dist, float* dist, int32_t* work, void* stream) {
    if (Q < 0 || M < 0 || C < 0 || C > M || !origin || !dims) return DMVS_EINVAL;
    if (!(h > 0.0) || !isfinite(h) || !(max_dist > 0.0f) || !isfinite(max_dist)) return DMVS_EINVAL;
    if (!isfinite(origin[0]) || !isfinite(origin[1]) || !isfinite(origin[2])) return DMVS_EINVAL;
    if (Q > 0 && (!query || !dist)) return DMVS_EINVAL;
    if (M > 0 && (!target || !cell_keys || !cell_start || C < 1)) return DMVS_EINVAL;
    if (M == 0 && C != 0) return DMVS_EINVAL;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return DMVS_EINVAL;
    if (ceil((double)max_dist / h) > (double)DMVS_CLOUD_MAX_RINGS) return DMVS_EINVAL;
    CloudGrid g;
    g.bx = cloud_bits(dims[0]), g.by = cloud_bits(dims[1]);
    if (g.bx + g.by + cloud_bits(dims[2]) > DMVS_CLOUD_MAX_KEY_BITS) return DMVS_EINVAL;      // the grid exceeds the key range
    if (Q == 0) return 0;
    g.keys = cell_keys, g.start = cell_start, g.C = (long)C;
    g.ox = origin[0], g.oy = origin[1], g.oz = origin[2], g.h = h;
    g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
    if (dmvs_ceil_div(Q, DMVS_BLOCK) > (1u << 30) || Q > (1L << 38)) return DMVS_EINVAL;
    dim3 grid(dmvs_ceil_div(Q, DMVS_BLOCK)), block(DMVS_BLOCK);
    hipLaunchKernelGGL(cloud_nn_dist_kernel, grid, block, 0, (hipStream_t)stream, query, (long)Q, target, g, max_dist, dist, work);
    return dmvs_launch_status();
}

extern "C" int dmvs_cloud_stats_f32(const float* dist, const uint8_t* valid, int64_t N, float max_dist, const float* thresholds, int32_t T,
                                    double scale, int32_t blocks, uint64_t* out, void* stream) {
    if (N < 0 || T < 0 || T > CLOUD_MAX_T || !out || blocks < 0 || (N > 0 && !dist) || (T > 0 && !thresholds)) return DMVS_EINVAL;
    if (!(max_dist > 0.0f) || !isfinite(max_dist) || !(scale > 0.0) || !isfinite(scale)) return DMVS_EINVAL;
    int e = 0;
    if (frexp(scale, &e) != 0.5) return DMVS_EINVAL;                                       // not a power of two
    if (!((double)max_dist * scale * (double)(N > 0 ? N : 1) < 4611686018427387904.0)) return DMVS_EINVAL;      // 2^62: the sum cannot overflow
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
    long nb = (N + DMVS_BLOCK - 1) / DMVS_BLOCK;
    const long cap = blocks > 0 ? blocks : 4096;          // a grid-stride loop: a few thousand workgroups keep the atomics few
    if (nb > cap) nb = cap;
    dim3 grid((unsigned)nb), block(DMVS_BLOCK);
    hipLaunchKernelGGL(cloud_stats_kernel, grid, block, 0, s, dist, valid, (long)N, max_dist, thr, (int)T, scale, acc);
    return dmvs_launch_status();
}
