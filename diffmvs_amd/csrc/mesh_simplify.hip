// Simplifying an extracted mesh (diffmvs_amd/mesh_simplify.py): dmvs_mesh_cluster_verts_i64, dmvs_mesh_cluster_quadrics_i64,
// dmvs_mesh_cluster_place_f32 and dmvs_mesh_cluster_remap_i32.  The contract (the local coordinate, the quadric terms, the regularised
// solve by cofactors, the rotation of the remapped faces) is in include/dmvs.h.
//
// Sums.  A vertex adds 7 integers to its cluster and a face up to 30 to the clusters of its corners.  Surface-nets vertices and faces are
// numbered in cell order, so neighbouring lanes of a wave mostly add to the same cluster, and atomics on one address are served one after
// the other.  run_sum() finds the runs of neighbouring lanes with the same destination (a max-scan of the run heads), sums every run into
// its first lane with a segmented suffix sum (six shuffle steps whatever the run lengths) and only that lane issues the atomics: one lot
// per run and wave instead of one per lane.  A corner slot in which no lane of the wave has anything to add (the second and third corner
// of a face inside one cell) costs one reduction.  Integer adds either way: the sums are the same bits.  Compiled with
// -DDMVS_MESH_QUADRIC_PLAIN every lane issues its own atomics (tools/mesh_simplify_bench.py builds that variant beside the product and
// measures both).
//
// Placement and remap are one lane per cluster / per face, fp64 in the header's order.
#include "cloud_walk.h"      // CloudSums / cloud_block_sum, cloud_pow2, cloud_sum_fits, cloud_sum_blocks

namespace {

typedef unsigned long long u64;

struct Lattice {
    double o[3], cell;
};

struct SimplifyMesh {
    const float* verts;
    const int32_t* faces;
    const int32_t* cluster;
    long N, F, K;
};

// the position of a coordinate inside its lattice cell, relative to the cell's centre, in cells
__device__ __forceinline__ double local_coord(double p, double o, double cell) {
#pragma clang fp contract(off)
    const double t = (p - o) / cell;
    return isfinite(t) ? t - (floor(t) + 0.5) : 0.0;
}

__device__ __forceinline__ int cluster_of(const SimplifyMesh& m, int32_t v) {
    const int k = m.cluster[v];
    return k < 0 || (long)k >= m.K ? -1 : k;
}

// a face's corners and their clusters; false for a BAD face (an index outside [0, N) or a corner without a cluster)
__device__ __forceinline__ bool simplify_face(const SimplifyMesh& m, long f, int32_t x[3], int k[3]) {
    x[0] = m.faces[3 * f], x[1] = m.faces[3 * f + 1], x[2] = m.faces[3 * f + 2];
    if (x[0] < 0 || x[1] < 0 || x[2] < 0 || (long)x[0] >= m.N || (long)x[1] >= m.N || (long)x[2] >= m.N) return false;
    k[0] = cluster_of(m, x[0]), k[1] = cluster_of(m, x[1]), k[2] = cluster_of(m, x[2]);
    return k[0] >= 0 && k[1] >= 0 && k[2] >= 0;
}

// (p1 - p0) x (p2 - p0) in the order of dmvs_mesh_face_tally_i64
__device__ __forceinline__ void face_cross(const double p[3][3], double c[3]) {
#pragma clang fp contract(off)
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    c[0] = ay * bz - az * by, c[1] = az * bx - ax * bz, c[2] = ax * by - ay * bx;
}

// ------------------------------------------------------------------------------------------ runs of one destination inside a wave
// true in every lane when some lane of the wave has flag set (every lane of the wave calls)
__device__ __forceinline__ bool wave_any(bool flag) {
    int a = flag ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) a |= __shfl_xor(a, off);
    return a != 0;
}

// Every lane of the wave calls with its destination `key` (< 0: nothing to add, its terms are zero) and NT terms.  Neighbouring lanes
// with the same key form a run; on return the FIRST lane of every run holds the run's sums and gets true (for key >= 0), the others false.
template <int NT>
__device__ __forceinline__ bool run_sum(int key, u64 (&v)[NT]) {
    const int lane = threadIdx.x & 63;
    const int before = __shfl(key, lane > 0 ? lane - 1 : 0);
    const bool head = lane == 0 || before != key;
    int start = head ? lane : 0;                            // the first lane of this lane's run: the largest head at or before it
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl(start, lane >= off ? lane - off : lane);
        start = o > start ? o : start;
    }
    for (int off = 1; off < 64; off <<= 1) {                // after the step `off` a lane holds the sum of up to 2 off lanes of its run from itself on
        const int src = lane + off < 64 ? lane + off : lane;
        const int theirs = __shfl(start, src);             // (every lane shuffles: no short-circuit in front of it)
        const bool same = lane + off < 64 && theirs == start;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const u64 o = __shfl(v[k], src);
            v[k] += same ? o : 0ull;
        }
    }
    return head && key >= 0;
}

// ------------------------------------------------------------------------------------------ the vertex pass
template <bool COMBINE, bool RGB>
__global__ void __launch_bounds__(DMVS_BLOCK)
cluster_verts_kernel(SimplifyMesh m, const uint8_t* __restrict__ rgb, Lattice g, int* cnt, u64* pos_q, u64* rgb_sum) {
    constexpr int NT = RGB ? 7 : 4;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    // the trip count is the wave's, not the lane's: every lane of a wave reaches every shuffle
    for (long v0 = tid - (threadIdx.x & 63); v0 < m.N; v0 += stride) {
        const long v = v0 + (threadIdx.x & 63);
        int k = -1;
        u64 t[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) t[i] = 0ull;
        if (v < m.N && (k = cluster_of(m, (int32_t)v)) >= 0) {
            t[0] = 1ull;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                t[1 + i] = (u64)(long long)llrint(local_coord((double)m.verts[3 * v + i], g.o[i], g.cell) * 4294967296.0);
                if (RGB) t[4 + i] = (u64)rgb[3 * v + i];
            }
        }
        const bool send = COMBINE ? run_sum<NT>(k, t) : k >= 0;
        if (!send) continue;
        atomicAdd(cnt + k, (int)t[0]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (t[1 + i]) atomicAdd(pos_q + 3 * (long)k + i, t[1 + i]);
            if (RGB && t[4 + i]) atomicAdd(rgb_sum + 3 * (long)k + i, t[4 + i]);
        }
    }
}

// ------------------------------------------------------------------------------------------ the face pass
// the ten terms of one corner's plane: n the unit normal, w the weight, u the corner's local coordinate
__device__ __forceinline__ void quadric_terms(const double n[3], double w, const double u[3], double scale, u64 (&t)[10]) {
#pragma clang fp contract(off)
    const double d = -((n[0] * u[0] + n[1] * u[1]) + n[2] * u[2]);
    const double wx = w * n[0], wy = w * n[1], wz = w * n[2], wd = w * d;
    const double T[10] = {wx * n[0], wx * n[1], wx * n[2], wy * n[1], wy * n[2], wz * n[2], wd * n[0], wd * n[1], wd * n[2], wd * d};
#pragma unroll
    for (int k = 0; k < 10; ++k) t[k] = (u64)(long long)llrint(T[k] * scale);
}

template <bool COMBINE>
__global__ void __launch_bounds__(DMVS_BLOCK)
cluster_quadrics_kernel(SimplifyMesh m, Lattice g, double scale, double cap, u64* quad_q, u64* state) {
    CloudSums<2> counts;                                   // bad, flat
    counts.v[0] = counts.v[1] = 0ull;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    for (long f0 = tid - (threadIdx.x & 63); f0 < m.F; f0 += stride) {      // (the wave's trip count, as above)
        const long f = f0 + (threadIdx.x & 63);
        int dest[3] = {-1, -1, -1};                        // per corner slot: the cluster this lane adds to, -1 = nothing
        double n[3] = {0.0, 0.0, 0.0}, u[3][3], w = 0.0;
        if (f < m.F) {
            int32_t x[3];
            int k[3];
            if (!simplify_face(m, f, x, k)) {
                counts.v[0] += 1ull;
            } else {
#pragma clang fp contract(off)
                double p[3][3], c[3];
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 3; ++i) p[j][i] = (double)m.verts[3 * (long)x[j] + i];
                face_cross(p, c);
                const double l = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
                if (!(l > 0.0) || !isfinite(l)) {
                    counts.v[1] += 1ull;
                } else {
                    n[0] = c[0] / l, n[1] = c[1] / l, n[2] = c[2] / l;
                    w = fmin((0.5 * l) / (g.cell * g.cell), cap);
                    for (int j = 0; j < 3; ++j)
                        for (int i = 0; i < 3; ++i) u[j][i] = local_coord(p[j][i], g.o[i], g.cell);
                    dest[0] = k[0];
                    dest[1] = k[1] != k[0] ? k[1] : -1;
                    dest[2] = k[2] != k[0] && k[2] != k[1] ? k[2] : -1;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (COMBINE && !wave_any(dest[j] >= 0)) continue;      // (wave-uniform)
            u64 t[10];
            if (dest[j] >= 0) {
                quadric_terms(n, w, u[j], scale, t);
            } else {
#pragma unroll
                for (int k = 0; k < 10; ++k) t[k] = 0ull;
            }
            const bool send = COMBINE ? run_sum<10>(dest[j], t) : dest[j] >= 0;
            if (!send) continue;
            u64* q = quad_q + 10 * (long)dest[j];
#pragma unroll
            for (int k = 0; k < 10; ++k)
                if (t[k]) atomicAdd(q + k, t[k]);
        }
    }
    cloud_block_sum<2>(counts, 2, state);
}

// ------------------------------------------------------------------------------------------ placement
struct PlaceArgs {
    const int32_t* cnt;
    const int64_t* pos_q;
    const int64_t* rgb_sum;
    const int64_t* quad_q;
    const int64_t* cells;
    long K;
    double scale, reg;
    int mode;
};

__global__ void __launch_bounds__(DMVS_BLOCK)
cluster_place_kernel(PlaceArgs a, Lattice g, float* __restrict__ out_verts, uint8_t* __restrict__ out_rgb, u64* state) {
#pragma clang fp contract(off)
    CloudSums<1> fell;
    fell.v[0] = 0ull;
    const long k = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (k < a.K) {
        const long long n = a.cnt[k];
        double q[9], mean[3], x[3];
        for (int i = 0; i < 9; ++i) q[i] = (double)a.quad_q[10 * k + i] / a.scale;
        for (int i = 0; i < 3; ++i) mean[i] = n > 0 ? ((double)a.pos_q[3 * k + i] / 4294967296.0) / (double)n : 0.0;
        const double tr = (q[0] + q[3]) + q[5], lam = a.reg * tr;
        const double M00 = q[0] + lam, M01 = q[1], M02 = q[2], M11 = q[3] + lam, M12 = q[4], M22 = q[5] + lam;
        const double r0 = lam * mean[0] - q[6], r1 = lam * mean[1] - q[7], r2 = lam * mean[2] - q[8];
        const double c00 = M11 * M22 - M12 * M12, c01 = M02 * M12 - M01 * M22, c02 = M01 * M12 - M02 * M11;
        const double c11 = M00 * M22 - M02 * M02, c12 = M01 * M02 - M00 * M12, c22 = M00 * M11 - M01 * M01;
        const double det = (M00 * c00 + M01 * c01) + M02 * c02;
        x[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        x[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        x[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        const bool fin = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
        const bool good = tr > 0.0 && det > 0.0 && fin && fmax(fmax(fabs(x[0]), fabs(x[1])), fabs(x[2])) <= 1.0;
        if (a.mode == DMVS_SIMPLIFY_QUADRIC && tr > 0.0 && !good) fell.v[0] = 1ull;
        for (int i = 0; i < 3; ++i) {
            const double xi = a.mode == DMVS_SIMPLIFY_QUADRIC && good ? x[i] : mean[i];
            out_verts[3 * k + i] = (float)(g.o[i] + (((double)a.cells[3 * k + i] + 0.5) + xi) * g.cell);
            if (out_rgb) out_rgb[3 * k + i] = n > 0 ? (uint8_t)((2 * a.rgb_sum[3 * k + i] + n) / (2 * n)) : (uint8_t)0;
        }
    }
    cloud_block_sum<1>(fell, 1, state);
}

// ------------------------------------------------------------------------------------------ remap
__global__ void __launch_bounds__(DMVS_BLOCK)
cluster_remap_kernel(SimplifyMesh m, const float* __restrict__ new_verts, int32_t* __restrict__ out_faces, uint8_t* __restrict__ keep, u64* state) {
#pragma clang fp contract(off)
    CloudSums<3> counts;                                   // degenerate, flipped, bad
    counts.v[0] = counts.v[1] = counts.v[2] = 0ull;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    for (long f = tid; f < m.F; f += stride) {
        int32_t x[3];
        int k[3] = {-1, -1, -1};
        uint8_t kept = 0;
        if (m.N == 0 || m.K == 0 || !simplify_face(m, f, x, k)) {
            counts.v[2] += 1ull;
            k[0] = k[1] = k[2] = -1;
        } else if (k[0] == k[1] || k[0] == k[2] || k[1] == k[2]) {
            counts.v[0] += 1ull;
        } else {
            kept = 1;
            if (new_verts) {
                double p[3][3], pn[3][3], c[3], cn[3];
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 3; ++i) p[j][i] = (double)m.verts[3 * (long)x[j] + i], pn[j][i] = (double)new_verts[3 * (long)k[j] + i];
                face_cross(p, c);
                face_cross(pn, cn);
                if ((c[0] * cn[0] + c[1] * cn[1]) + c[2] * cn[2] < 0.0) counts.v[1] += 1ull;
            }
        }
        const int first = k[0] <= k[1] && k[0] <= k[2] ? 0 : (k[1] <= k[2] ? 1 : 2);      // (distinct where it matters)
        out_faces[3 * f] = k[first], out_faces[3 * f + 1] = k[(first + 1) % 3], out_faces[3 * f + 2] = k[(first + 2) % 3];
        keep[f] = kept;
    }
    cloud_block_sum<3>(counts, 3, state);
}

inline bool simplify_sizes_ok(int64_t N, int64_t F, int64_t K) {
    return N >= 0 && F >= 0 && K >= 0 && N <= 2147483647L && F <= 2147483647L && K <= 2147483647L;
}

// origin (HOST) and cell -> the kernel argument; false for a NULL or non-finite origin or a cell that is not positive and finite
inline bool simplify_lattice(const double* origin, double cell, Lattice& g) {
    if (!origin || !(cell > 0.0) || !isfinite(cell)) return false;
    for (int i = 0; i < 3; ++i) {
        if (!isfinite(origin[i])) return false;
        g.o[i] = origin[i];
    }
    g.cell = cell;
    return true;
}

inline bool misaligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" int dmvs_mesh_cluster_verts_i64(const float* verts, const uint8_t* rgb, int64_t N, const int32_t* cluster, int64_t K, const double* origin,
                                           double cell, int32_t* cnt, int64_t* pos_q, int64_t* rgb_sum, int32_t blocks, void* stream) {
    Lattice g;
    if (!simplify_sizes_ok(N, 0, K) || blocks < 0 || !simplify_lattice(origin, cell, g)) return DMVS_EINVAL;
    if (misaligned(verts, 3u) || misaligned(cluster, 3u) || misaligned(cnt, 3u) || misaligned(pos_q, 7u) || misaligned(rgb_sum, 7u)) return DMVS_EINVAL;
    if (K > 0 && (!cnt || !pos_q || (rgb && !rgb_sum))) return DMVS_EINVAL;
    if (N > 0 && K > 0 && (!verts || !cluster)) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = K > 0 ? hipMemsetAsync(cnt, 0, (size_t)K * sizeof(int32_t), s) : hipSuccess;
    if (err == hipSuccess && K > 0) err = hipMemsetAsync(pos_q, 0, (size_t)K * 3 * sizeof(int64_t), s);
    if (err == hipSuccess && K > 0 && rgb) err = hipMemsetAsync(rgb_sum, 0, (size_t)K * 3 * sizeof(int64_t), s);
    if (err != hipSuccess) return (int)err;
    if (N == 0 || K == 0) return 0;
    SimplifyMesh m = {verts, nullptr, cluster, (long)N, 0, (long)K};
    const dim3 grid(cloud_sum_blocks(N, blocks)), block(DMVS_BLOCK);
    int* c = reinterpret_cast<int*>(cnt);
    u64 *pq = reinterpret_cast<u64*>(pos_q), *rs = reinterpret_cast<u64*>(rgb_sum);
#ifdef DMVS_MESH_QUADRIC_PLAIN
    constexpr bool combine = false;
#else
    constexpr bool combine = true;
#endif
    if (rgb) hipLaunchKernelGGL((cluster_verts_kernel<combine, true>), grid, block, 0, s, m, rgb, g, c, pq, rs);
    else hipLaunchKernelGGL((cluster_verts_kernel<combine, false>), grid, block, 0, s, m, rgb, g, c, pq, rs);
    return dmvs_launch_status();
}

extern "C" int dmvs_mesh_cluster_quadrics_i64(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int32_t* cluster, int64_t K,
                                              const double* origin, double cell, double scale, double cap, int64_t* quad_q, int64_t* state,
                                              int32_t blocks, void* stream) {
    Lattice g;
    if (!simplify_sizes_ok(N, F, K) || blocks < 0 || !simplify_lattice(origin, cell, g) || !cloud_pow2(scale)) return DMVS_EINVAL;
    if (!(cap >= 0.0) || !(cap < 4611686018427387904.0) || !cloud_sum_fits(3 * F, cap, scale)) return DMVS_EINVAL;      // (false for NaN)
    if (misaligned(verts, 3u) || misaligned(faces, 3u) || misaligned(cluster, 3u) || misaligned(quad_q, 7u) || misaligned(state, 7u)) return DMVS_EINVAL;
    if (!state || (K > 0 && !quad_q)) return DMVS_EINVAL;
    if (F > 0 && (!faces || (N > 0 && K > 0 && (!verts || !cluster)))) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(state, 0, 2 * sizeof(int64_t), s);
    if (err == hipSuccess && K > 0) err = hipMemsetAsync(quad_q, 0, (size_t)K * 10 * sizeof(int64_t), s);
    if (err != hipSuccess) return (int)err;
    if (F == 0) return 0;
    // (N = 0 or K = 0: every face is BAD; the kernel counts them and reads neither verts nor cluster)
    SimplifyMesh m = {verts, faces, cluster, K > 0 ? (long)N : 0, (long)F, (long)K};
    const dim3 grid(cloud_sum_blocks(F, blocks)), block(DMVS_BLOCK);
    u64 *qq = reinterpret_cast<u64*>(quad_q), *st = reinterpret_cast<u64*>(state);
#ifdef DMVS_MESH_QUADRIC_PLAIN
    hipLaunchKernelGGL(cluster_quadrics_kernel<false>, grid, block, 0, s, m, g, scale, cap, qq, st);
#else
    hipLaunchKernelGGL(cluster_quadrics_kernel<true>, grid, block, 0, s, m, g, scale, cap, qq, st);
#endif
    return dmvs_launch_status();
}

extern "C" int dmvs_mesh_cluster_place_f32(int64_t K, const int32_t* cnt, const int64_t* pos_q, const int64_t* rgb_sum, const int64_t* quad_q,
                                           const int64_t* cells, const double* origin, double cell, double scale, double reg, int32_t mode,
                                           float* out_verts, uint8_t* out_rgb, int64_t* state, void* stream) {
    Lattice g;
    if (!simplify_sizes_ok(0, 0, K) || !simplify_lattice(origin, cell, g) || !cloud_pow2(scale) || !(reg > 0.0) || !isfinite(reg)) return DMVS_EINVAL;
    if (mode != DMVS_SIMPLIFY_QUADRIC && mode != DMVS_SIMPLIFY_MEAN) return DMVS_EINVAL;
    if (misaligned(cnt, 3u) || misaligned(out_verts, 3u) || misaligned(pos_q, 7u) || misaligned(rgb_sum, 7u) || misaligned(quad_q, 7u) ||
        misaligned(cells, 7u) || misaligned(state, 7u))
        return DMVS_EINVAL;
    if (!state || (K > 0 && (!cnt || !pos_q || !quad_q || !cells || !out_verts || (out_rgb != nullptr) != (rgb_sum != nullptr)))) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t err = hipMemsetAsync(state, 0, sizeof(int64_t), s);
    if (err != hipSuccess) return (int)err;
    if (K == 0) return 0;
    PlaceArgs a = {cnt, pos_q, rgb_sum, quad_q, cells, (long)K, scale, reg, (int)mode};
    hipLaunchKernelGGL(cluster_place_kernel, dim3(dmvs_ceil_div(K, DMVS_BLOCK)), dim3(DMVS_BLOCK), 0, s, a, g, out_verts, out_rgb,
                       reinterpret_cast<u64*>(state));
    return dmvs_launch_status();
}

extern "C" int dmvs_mesh_cluster_remap_i32(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int32_t* cluster, int64_t K,
                                           const float* new_verts, int32_t* out_faces, uint8_t* keep, int64_t* state, int32_t blocks, void* stream) {
    if (!simplify_sizes_ok(N, F, K) || blocks < 0) return DMVS_EINVAL;
    if (misaligned(verts, 3u) || misaligned(faces, 3u) || misaligned(cluster, 3u) || misaligned(new_verts, 3u) || misaligned(out_faces, 3u) ||
        misaligned(state, 7u))
        return DMVS_EINVAL;
    if (!state || (F > 0 && (!faces || !out_faces || !keep))) return DMVS_EINVAL;
    if (F > 0 && N > 0 && K > 0 && (!cluster || (new_verts && !verts))) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t err = hipMemsetAsync(state, 0, 3 * sizeof(int64_t), s);
    if (err != hipSuccess) return (int)err;
    if (F == 0) return 0;
    SimplifyMesh m = {verts, faces, cluster, (long)N, (long)F, (long)K};
    hipLaunchKernelGGL(cluster_remap_kernel, dim3(cloud_sum_blocks(F, blocks)), dim3(DMVS_BLOCK), 0, s, m, new_verts, out_faces, keep,
                       reinterpret_cast<u64*>(state));
    return dmvs_launch_status();
}
