// The grid walk of the point-cloud kernels, shared by dmvs_cloud_nn_dist_f32 (cloud_eval.hip) and dmvs_cloud_nn_index_f32
// (cloud_register.hip); the walk itself is described at the top of cloud_eval.hip.  INDEX = true also tracks WHICH target is the
// nearest (one more register and a select per target tested); with INDEX = false that member is never read and the walk compiles
// to what it was before the index search existed.  The walk is written once over a collector, so dmvs_cloud_knn_f32 (cloud_clean.hip)
// runs the same code with a k-best list in place of the single best.  Also here: what the fixed-point reductions of both files share (cloud_block_sum
// and the host-side shaping of its launches).
#pragma once
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

// an optional similarity applied to a point before anything else: p' = fp32(((m0 x + m1 y) + m2 z) + m3) per row, products and sums
// in fp64 in exactly this order without contraction, ONE rounding to fp32 (include/dmvs.h)
struct CloudTransform {
    double m[12];              // row-major 3x4 [sR | t]
    int on;                    // 0: identity (the point is taken as it is)
};

__device__ __forceinline__ void cloud_move(const CloudTransform& T, float& x, float& y, float& z) {
#pragma clang fp contract(off)
    if (!T.on) return;
    const double dx = x, dy = y, dz = z;
    x = (float)(((T.m[0] * dx + T.m[1] * dy) + T.m[2] * dz) + T.m[3]);
    y = (float)(((T.m[4] * dx + T.m[5] * dy) + T.m[6] * dz) + T.m[7]);
    z = (float)(((T.m[8] * dx + T.m[9] * dy) + T.m[10] * dz) + T.m[11]);
}

// the fp32 squared distance of the searches: three differences, three products, two sums, no contraction
__device__ __forceinline__ float cloud_dist2(float qx, float qy, float qz, const float* __restrict__ t) {
#pragma clang fp contract(off)
    const float dx = qx - t[0], dy = qy - t[1], dz = qz - t[2];
    return (dx * dx + dy * dy) + dz * dz;
}

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
    int points;                 // targets tested (the optional work output)
};

// What a search keeps of the targets it tests is its COLLECTOR: bound() is the squared distance a target has to beat (the walk prunes
// against it), take(d2, p) is handed every tested target p with its squared distance.  CloudNearest is the collector of the two nearest
// searches; CloudKBest (cloud_clean.hip) keeps the k smallest.
template <bool INDEX>
struct CloudNearest {
    float best2;
    int best_i;                 // INDEX: the target that gave best2 (-1: none yet)
    __device__ __forceinline__ float bound() const { return best2; }
    __device__ __forceinline__ void take(float d2, long p) {
        if (INDEX) best_i = d2 < best2 ? (int)p : best_i;      // (strict: the first of exactly equidistant targets in walk order stays)
        best2 = d2 < best2 ? d2 : best2;
    }
};

template <class COL>
__device__ __forceinline__ void cloud_scan_cell(CloudQuery& q, COL& col, const CloudGrid& g, const float* __restrict__ target, long c) {
#pragma clang fp contract(off)
    const long p0 = g.start[c], p1 = g.start[c + 1];
    for (long p = p0; p < p1; ++p) {
        const float dx = q.qx - target[3 * p], dy = q.qy - target[3 * p + 1], dz = q.qz - target[3 * p + 2];
        col.take((dx * dx + dy * dy) + dz * dz, p);
    }
    q.points += (int)(p1 - p0);
}

// one occupied row (y, z): its cells outward from the query's x; g2yz = squared gap of the row (length units)
template <class COL>
__device__ __forceinline__ void cloud_visit_row(CloudQuery& q, COL& col, const CloudGrid& g, const float* __restrict__ target, int y, int z, float g2yz) {
    const int64_t row = ((int64_t)z << g.by) | y, base = row << g.bx;
    const long cm = cloud_lower_bound(g.keys, 0, g.C, base | q.cx);
    for (long c = cm; c < g.C; ++c) {                      // x >= cx
        const int64_t k = g.keys[c];
        if ((k >> g.bx) != row) break;
        const float gx = (float)(cloud_gap((int)(k - base) - q.cx, q.tx) * g.h);
        if (gx * gx + g2yz >= col.bound() * kPruneMargin) break;
        cloud_scan_cell(q, col, g, target, c);
    }
    for (long c = cm - 1; c >= 0; --c) {                   // x < cx
        const int64_t k = g.keys[c];
        if ((k >> g.bx) != row) break;
        const float gx = (float)(cloud_gap((int)(k - base) - q.cx, q.tx) * g.h);
        if (gx * gx + g2yz >= col.bound() * kPruneMargin) break;
        cloud_scan_cell(q, col, g, target, c);
    }
}

// one slab z: its occupied rows outward from the query's y
template <class COL>
__device__ __forceinline__ void cloud_visit_slab(CloudQuery& q, COL& col, const CloudGrid& g, const float* __restrict__ target, int z, float g2z) {
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
        if (g2 >= col.bound() * kPruneMargin) break;
        cloud_visit_row(q, col, g, target, yo, z, g2);
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
        if (g2 >= col.bound() * kPruneMargin) break;
        cloud_visit_row(q, col, g, target, yo, z, g2);
        y = yo - 1;
    }
}

__device__ __forceinline__ int cloud_clamp_cell(double u, int n) {
    const double f = floor(u);
    return f < 0.0 ? 0 : (f > (double)(n - 1) ? n - 1 : (int)f);      // (u is finite: checked by the caller)
}

// the walk of one query (q.qx, q.qy, q.qz set by the caller) into `col`: rings of slabs outward in z until no unseen slab can beat the
// collector's bound.  -> rings walked (0: an empty grid or a non-finite query, nothing tested); q.points counts the targets tested
template <class COL>
__device__ __forceinline__ int cloud_walk(CloudQuery& q, COL& col, const CloudGrid& g, const float* __restrict__ target) {
    const double ux = ((double)q.qx - g.ox) / g.h, uy = ((double)q.qy - g.oy) / g.h, uz = ((double)q.qz - g.oz) / g.h;
    int rings = 0;
    q.points = 0;
    if (g.C > 0 && isfinite(ux) && isfinite(uy) && isfinite(uz)) {
        q.cx = cloud_clamp_cell(ux, g.nx), q.cy = cloud_clamp_cell(uy, g.ny), q.cz = cloud_clamp_cell(uz, g.nz);
        q.tx = ux - q.cx, q.ty = uy - q.cy, q.tz = uz - q.cz;
        bool up = true, down = true;
        for (int r = 0; up || down; ++r) {
            rings = r + 1;
            if (up) {
                const int z = q.cz + r;
                const float gz = (float)(cloud_gap(r, q.tz) * g.h);
                if (z >= g.nz || gz * gz >= col.bound() * kPruneMargin) up = false;
                else cloud_visit_slab(q, col, g, target, z, gz * gz);
            }
            if (r == 0) continue;
            if (down) {
                const int z = q.cz - r;
                const float gz = (float)(cloud_gap(-r, q.tz) * g.h);
                if (z < 0 || gz * gz >= col.bound() * kPruneMargin) down = false;
                else cloud_visit_slab(q, col, g, target, z, gz * gz);
            }
        }
    }
    return rings;
}

// the search of one query: moves it (T), walks the grid, writes dist (may be NULL with INDEX) / index (INDEX only) / work (may be NULL)
template <bool INDEX>
__global__ void __launch_bounds__(DMVS_BLOCK)
cloud_nn_kernel(const float* __restrict__ query, long Q, const float* __restrict__ target, CloudGrid g, float max_dist, CloudTransform T,
                float* __restrict__ dist, int32_t* __restrict__ index, int32_t* __restrict__ work) {
    const long i = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (i >= Q) return;
    CloudQuery q;
    q.qx = query[3 * i], q.qy = query[3 * i + 1], q.qz = query[3 * i + 2];
    if (INDEX) cloud_move(T, q.qx, q.qy, q.qz);
    CloudNearest<INDEX> col;
    col.best_i = -1;
    col.best2 = max_dist * max_dist;
    const int rings = cloud_walk(q, col, g, target);
    const float d = col.best2 < max_dist * max_dist ? fminf(sqrtf(col.best2), max_dist) : max_dist;
    if (INDEX) {
        if (dist) dist[i] = d;
        index[i] = d < max_dist ? col.best_i : -1;      // -1 exactly where the distance is the clamp
    } else {
        dist[i] = d;
    }
    if (work) {
        work[2 * i] = rings;
        work[2 * i + 1] = q.points;
    }
}

// The project's fixed-point reduction (dmvs_cloud_stats_f32, dmvs_cloud_pair_moments_f64): every lane of a DMVS_BLOCK workgroup brings N
// u64 partial sums; waves reduce with shuffles, the workgroup through LDS, then ONE integer atomicAdd per counter per workgroup into
// out[0 .. live).  Integer sums are associative, so the totals are bitwise independent of launch order and grid shape.
template <int N> struct CloudSums { unsigned long long v[N]; };

template <int N>
__device__ __forceinline__ void cloud_block_sum(CloudSums<N> acc, int live, unsigned long long* out) {
    __shared__ unsigned long long part[DMVS_BLOCK / 64][N];
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc.v[k] += __shfl_down(acc.v[k], off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) part[wave][k] = acc.v[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < live) {
        unsigned long long v = 0;
        for (int w = 0; w < DMVS_BLOCK / 64; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(out + threadIdx.x, v);
    }
}

// The integer minimum of the z-buffer splat (cloud_render.hip): one no-return u32 atomic-min on the device; under the host emulation, whose
// header has integer atomicAdd only, a compare-exchange loop on the compiler builtin.  dmvs_peek_u32 is the plain load in front of it (the
// value may be stale; the caller only ever uses it as an upper bound of a value that never rises).
__device__ __forceinline__ void dmvs_atomic_min_u32(unsigned* p, unsigned v) {
#ifdef DMVS_HOST_EMULATION
    unsigned old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
#else
    atomicMin(p, v);
#endif
}
__device__ __forceinline__ unsigned dmvs_peek_u32(const unsigned* p) {
#ifdef DMVS_HOST_EMULATION
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return *p;
#endif
}

// The same pair on 64 bits, for the rasteriser's (depth bits << 32 | face) keys (mesh_render.hip).
__device__ __forceinline__ void dmvs_atomic_min_u64(unsigned long long* p, unsigned long long v) {
#ifdef DMVS_HOST_EMULATION
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
#else
    atomicMin(p, v);
#endif
}
__device__ __forceinline__ unsigned long long dmvs_peek_u64(const unsigned long long* p) {
#ifdef DMVS_HOST_EMULATION
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return *p;
#endif
}

// host side of such a launch: the scale is a positive finite power of two ...
inline bool cloud_pow2(double s) {
    int e = 0;
    return s > 0.0 && isfinite(s) && frexp(s, &e) == 0.5;
}

// ... no sum of N terms of at most `big` can reach 2^62 ...
inline bool cloud_sum_fits(int64_t N, double big, double scale) { return (double)(N > 0 ? N : 1) * big * scale < 4611686018427387904.0; }

// ... and the kernel is a grid-stride loop: a few thousand workgroups (or `blocks`) keep the atomics few
inline unsigned cloud_sum_blocks(int64_t N, int32_t blocks) {
    const long nb = (N + DMVS_BLOCK - 1) / DMVS_BLOCK, cap = blocks > 0 ? blocks : 4096;
    return (unsigned)(nb < cap ? nb : cap);
}

inline int cloud_bits(long n) {
    int b = 0;
    while ((1L << b) < n) ++b;
    return b;
}

// host-side validation and set-up of the grid operands the two searches share; 0 or DMVS_EINVAL
inline int cloud_grid_args(int64_t Q, int64_t M, const float* target, const int64_t* cell_keys, const int64_t* cell_start, int64_t C,
                           const double* origin, double h, const int32_t* dims, float max_dist, CloudGrid& g) {
    if (Q < 0 || M < 0 || C < 0 || C > M || !origin || !dims) return DMVS_EINVAL;
    if (!(h > 0.0) || !isfinite(h) || !(max_dist > 0.0f) || !isfinite(max_dist)) return DMVS_EINVAL;
    if (!isfinite(origin[0]) || !isfinite(origin[1]) || !isfinite(origin[2])) return DMVS_EINVAL;
    if (M > 0 && (!target || !cell_keys || !cell_start || C < 1)) return DMVS_EINVAL;
    if (M == 0 && C != 0) return DMVS_EINVAL;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return DMVS_EINVAL;
    if (ceil((double)max_dist / h) > (double)DMVS_CLOUD_MAX_RINGS) return DMVS_EINVAL;
    g.bx = cloud_bits(dims[0]), g.by = cloud_bits(dims[1]);
    if (g.bx + g.by + cloud_bits(dims[2]) > DMVS_CLOUD_MAX_KEY_BITS) return DMVS_EINVAL;      // the grid exceeds the key range
    if (dmvs_ceil_div(Q, DMVS_BLOCK) > (1u << 30) || Q > (1L << 38)) return DMVS_EINVAL;
    g.keys = cell_keys, g.start = cell_start, g.C = (long)C;
    g.ox = origin[0], g.oy = origin[1], g.oz = origin[2], g.h = h;
    g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
    return 0;
}

// a HOST 3x4 row-major [sR | t] (NULL = identity) -> the kernel argument; DMVS_EINVAL for a non-finite entry
inline int cloud_transform_arg(const double* transform, CloudTransform& T) {
    T.on = transform ? 1 : 0;
    for (int k = 0; k < 12; ++k) {
        T.m[k] = transform ? transform[k] : (k % 5 == 0 ? 1.0 : 0.0);
        if (!isfinite(T.m[k])) return DMVS_EINVAL;
    }
    return 0;
}

// the two searches: dist is required without INDEX (and may be NULL with it), index and a 32-bit M with INDEX only
template <bool INDEX>
inline int cloud_nn_launch(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys, const int64_t* cell_start,
                           int64_t C, const double* origin, double h, const int32_t* dims, float max_dist, const double* transform, float* dist,
                           int32_t* index, int32_t* work, void* stream) {
    if (Q > 0 && (!query || (INDEX ? !index : !dist))) return DMVS_EINVAL;
    if (INDEX && M > 2147483647L) return DMVS_EINVAL;      // the index is 32 bits
    CloudGrid g;
    const int rc = cloud_grid_args(Q, M, target, cell_keys, cell_start, C, origin, h, dims, max_dist, g);
    if (rc != 0) return rc;
    CloudTransform T;
    if (cloud_transform_arg(transform, T) != 0) return DMVS_EINVAL;
    if (Q == 0) return 0;
    dim3 grid(dmvs_ceil_div(Q, DMVS_BLOCK)), block(DMVS_BLOCK);
    hipLaunchKernelGGL(cloud_nn_kernel<INDEX>, grid, block, 0, (hipStream_t)stream, query, (long)Q, target, g, max_dist, T, dist, index, work);
    return dmvs_launch_status();
}

}  // namespace
