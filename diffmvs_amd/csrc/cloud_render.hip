// Ground-truth depth maps from a scanned cloud (diffmvs_amd/cloud_render.py): dmvs_cloud_splat_zmin_f32 and dmvs_cloud_splat_sum_f32, a
// scatter with a z-buffer.  The contract (projection, footprint, slots) is in include/dmvs.h.
//
// One lane per point, grid-stride.  A launch carries up to DMVS_SPLAT_VIEW_CHUNK views as a KERNEL ARGUMENT: their 15 doubles each are
// wave-uniform (scalar loads from the argument segment, no vector register, no global table), and a point's 12 bytes are read once per
// chunk instead of once per view.  Per (point, view): nine fp64 multiply-adds, three fp64 divisions (u, v, the radius), the clamped square
// footprint, then per footprint pixel
//   pass 1 (z-min):  one u32 integer atomic-min of the fp32 depth's BIT PATTERN (z > near > 0: positive floats order like unsigned
//                    integers).  A plain load of the pixel first lets the lane skip the atomic when its depth cannot lower the pixel: the
//                    minimum only ever falls, so a value read earlier -- even a stale one from this CU's L1 -- is an upper bound of the
//                    current one and the skip cannot change the result.  Once the front surface is in, most points lose this test.
//   pass 2 (sum):    reads the FINISHED z-buffer (another launch) and, where the point lies within (1 + tau) of it, adds its fixed-point
//                    depth (u64) and 1 (int32) with integer atomics.
// Integer min and integer add are associative and commutative: every output is bitwise independent of the grid, the launch order and the
// order of the points.  No float atomic anywhere.  r_max <= DMVS_SPLAT_MAX_RADIUS bounds a lane's footprint loop at 33 x 33 trips.
// The per-view slots are 32-bit counters in LDS (a workgroup sees at most N < 2^31 points; only points that are NOT drawn, or whose radius
// was clamped, touch them), then one u64 integer atomic per non-zero slot per view per workgroup; the optional `work` pair goes through
// cloud_block_sum.  With a real loop over the chunk's views (not an unrolled one with 32 register counters: 119 VGPRs and 138 spilled
// SGPRs) the z-min kernel takes 42 VGPRs (46 with the work counters) and the sum kernel 40, no scratch, 8 waves per SIMD.
#include <float.h>

#include "cloud_walk.h"      // CloudTransform / cloud_move, CloudSums / cloud_block_sum, dmvs_atomic_min_u32 / dmvs_peek_u32

namespace {

#define SPLAT_VC DMVS_SPLAT_VIEW_CHUNK

struct SplatView { double p0[4], p1[4], e2[4], f, near, far; };      // = DMVS_SPLAT_VIEW_DOUBLES doubles, the layout of `views`
struct SplatViews {
    SplatView v[SPLAT_VC];
    int nv;                                                          // live views of this launch
};
struct SplatParams {
    double radius, r_min, r_max, tau1, scale;                        // tau1 = 1.0 + tau
    int H, W, pretest;
};
struct SplatFoot {
    int c0, c1, r0, r1;
    float z32;
    bool clamped;
};

// -1: draw `ft`; otherwise the slot that counts the point (1: outside (near, far], 2: off the image)
__device__ __forceinline__ int splat_project(double X, double Y, double Z, const SplatView& vw, const SplatParams& p, SplatFoot& ft) {
#pragma clang fp contract(off)
    const double x = ((vw.p0[0] * X + vw.p0[1] * Y) + vw.p0[2] * Z) + vw.p0[3];
    const double y = ((vw.p1[0] * X + vw.p1[1] * Y) + vw.p1[2] * Z) + vw.p1[3];
    const double z = ((vw.e2[0] * X + vw.e2[1] * Y) + vw.e2[2] * Z) + vw.e2[3];
    if (!(z > vw.near && z <= vw.far)) return 1;
    const double u = x / z, v = y / z;
    if (!(isfinite(u) && isfinite(v))) return 2;                     // (an overflowed product: nowhere on the image)
    const double raw = p.radius * vw.f / z;
    const double r = fmin(fmax(raw, p.r_min), p.r_max);
    // clamped in fp64 BEFORE the conversion: u, v of 1e300 never reach an integer
    const double c0 = fmax(ceil(u - r), 0.0), c1 = fmin(floor(u + r), (double)(p.W - 1));
    const double r0 = fmax(ceil(v - r), 0.0), r1 = fmin(floor(v + r), (double)(p.H - 1));
    if (!(c0 <= c1 && r0 <= r1)) return 2;
    ft.c0 = (int)c0, ft.c1 = (int)c1, ft.r0 = (int)r0, ft.r1 = (int)r1;
    ft.z32 = (float)z;
    ft.clamped = raw > p.r_max;
    return -1;
}

template <bool SUM, bool WORK>
__global__ void __launch_bounds__(DMVS_BLOCK)
splat_kernel(const float* __restrict__ pts, long N, CloudTransform T, SplatViews vs, SplatParams p, unsigned* zbuf,
             unsigned long long* __restrict__ sum, int* __restrict__ cnt, unsigned long long* __restrict__ counts,
             unsigned long long* __restrict__ work) {
    __shared__ int slots[SPLAT_VC * DMVS_SPLAT_SLOTS];               // per-view counters of this workgroup (N < 2^31)
    if (!SUM) {
        if (threadIdx.x < SPLAT_VC * DMVS_SPLAT_SLOTS) slots[threadIdx.x] = 0;
        __syncthreads();
    }
    unsigned long long visited = 0, issued = 0;
    const long HW = (long)p.H * p.W;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    for (long i = tid; i < N; i += stride) {
        float fx = pts[3 * i], fy = pts[3 * i + 1], fz = pts[3 * i + 2];
        cloud_move(T, fx, fy, fz);
        const bool finite = isfinite(fx) && isfinite(fy) && isfinite(fz);
        const double X = fx, Y = fy, Z = fz;
        for (int k = 0; k < vs.nv; ++k) {                            // (wave-uniform: the view's doubles are scalar loads)
            SplatFoot ft;
            const int slot = finite ? splat_project(X, Y, Z, vs.v[k], p, ft) : 0;
            if (slot >= 0) {
                if (!SUM) atomicAdd(&slots[k * DMVS_SPLAT_SLOTS + slot], 1);
                continue;
            }
            if (!SUM && ft.clamped) atomicAdd(&slots[k * DMVS_SPLAT_SLOTS + 3], 1);
            const unsigned zbits = __float_as_uint(ft.z32);
            unsigned long long q = 0;
            if (SUM) q = (unsigned long long)llrint((double)ft.z32 * p.scale);
            for (int row = ft.r0; row <= ft.r1; ++row) {
                const long base = (long)k * HW + (long)row * p.W;
                for (int col = ft.c0; col <= ft.c1; ++col) {
                    if (!SUM) {
                        if (WORK) ++visited;
                        if (p.pretest && !(zbits < dmvs_peek_u32(zbuf + base + col))) continue;
                        if (WORK) ++issued;
                        dmvs_atomic_min_u32(zbuf + base + col, zbits);
                    } else {
                        const float front = __uint_as_float(zbuf[base + col]);
                        if ((double)ft.z32 <= (double)front * p.tau1) {
                            atomicAdd(sum + base + col, q);
                            atomicAdd(cnt + base + col, 1);
                        }
                    }
                }
            }
        }
    }
    if (SUM) return;
    __syncthreads();
    if ((int)threadIdx.x < vs.nv * DMVS_SPLAT_SLOTS && slots[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)slots[threadIdx.x]);
    if (WORK) {                                                      // footprint pixels visited, atomics issued (compiled out without `work`)
        CloudSums<2> w;
        w.v[0] = visited, w.v[1] = issued;
        cloud_block_sum(w, 2, work);
    }
}

inline bool splat_nonneg(double v) { return v >= 0.0 && isfinite(v); }      // (false for NaN)

// what both passes check before anything is touched; 0 or DMVS_EINVAL.  far_max: the largest `far` of the views
inline int splat_args(const float* points, int64_t N, const double* transform, const double* views, int64_t V, int32_t H, int32_t W, double radius,
                      double r_min, double r_max, int32_t blocks, const void* zbuf, CloudTransform& T, double& far_max) {
    if (N < 0 || V < 0 || H < 0 || W < 0 || blocks < 0 || N > 2147483647L) return DMVS_EINVAL;      // (32-bit counters: slots, cnt)
    const int64_t HW = (int64_t)H * W;
    if (HW > 2147483647L || (HW > 0 && V > (1L << 40) / HW)) return DMVS_EINVAL;      // a plane is indexed in 31 bits, the buffer in 40
    if (!splat_nonneg(radius) || !splat_nonneg(r_min) || !(r_max >= r_min) || !(r_max <= (double)DMVS_SPLAT_MAX_RADIUS)) return DMVS_EINVAL;
    if (((uintptr_t)points & 3u) || ((uintptr_t)zbuf & 3u)) return DMVS_EINVAL;
    if (cloud_transform_arg(transform, T) != 0) return DMVS_EINVAL;
    if (V > 0 && !views) return DMVS_EINVAL;
    far_max = 0.0;
    for (int64_t v = 0; v < V; ++v) {
        const double* q = views + v * DMVS_SPLAT_VIEW_DOUBLES;
        for (int k = 0; k < 12; ++k)
            if (!isfinite(q[k])) return DMVS_EINVAL;
        if (!splat_nonneg(q[12]) || !(q[13] > 0.0) || !(q[14] > q[13]) || !(q[14] <= (double)FLT_MAX)) return DMVS_EINVAL;
        far_max = q[14] > far_max ? q[14] : far_max;
    }
    if (N > 0 && V > 0 && (!points || (HW > 0 && !zbuf))) return DMVS_EINVAL;
    return 0;
}

template <bool SUM>
inline int splat_launch(const float* points, int64_t N, const CloudTransform& T, const double* views, int64_t V, int32_t H, int32_t W,
                        const SplatParams& p, int32_t blocks, float* zbuf, uint64_t* sum, int32_t* cnt, unsigned long long* counts, uint64_t* work,
                        hipStream_t s) {
    const long HW = (long)H * W;
    dim3 grid(cloud_sum_blocks(N, blocks)), block(DMVS_BLOCK);
    for (int64_t v0 = 0; v0 < V; v0 += SPLAT_VC) {
        SplatViews vs;
        vs.nv = (int)(V - v0 < SPLAT_VC ? V - v0 : SPLAT_VC);
        for (int k = 0; k < SPLAT_VC; ++k) {
            const double* q = views + (v0 + (k < vs.nv ? k : 0)) * DMVS_SPLAT_VIEW_DOUBLES;      // (unused slots repeat the first: never read)
            for (int j = 0; j < 4; ++j) vs.v[k].p0[j] = q[j], vs.v[k].p1[j] = q[4 + j], vs.v[k].e2[j] = q[8 + j];
            vs.v[k].f = q[12], vs.v[k].near = q[13], vs.v[k].far = q[14];
        }
        unsigned* zb = reinterpret_cast<unsigned*>(zbuf) + v0 * HW;
        unsigned long long* sm = reinterpret_cast<unsigned long long*>(sum) + (sum ? v0 * HW : 0);
        int32_t* cn = cnt + (cnt ? v0 * HW : 0);
        unsigned long long* ct = counts + (counts ? v0 * DMVS_SPLAT_SLOTS : 0);
        unsigned long long* wk = reinterpret_cast<unsigned long long*>(work);
        if (SUM) hipLaunchKernelGGL((splat_kernel<true, false>), grid, block, 0, s, points, (long)N, T, vs, p, zb, sm, cn, ct, wk);
        else if (work) hipLaunchKernelGGL((splat_kernel<false, true>), grid, block, 0, s, points, (long)N, T, vs, p, zb, sm, cn, ct, wk);
        else hipLaunchKernelGGL((splat_kernel<false, false>), grid, block, 0, s, points, (long)N, T, vs, p, zb, sm, cn, ct, wk);
        const int rc = dmvs_launch_status();
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace

extern "C" int dmvs_cloud_splat_zmin_f32(const float* points, int64_t N, const double* transform, const double* views, int64_t V, int32_t H, int32_t W,
                                         double radius, double r_min, double r_max, int32_t flags, int32_t blocks, float* zbuf, int64_t* counts,
                                         uint64_t* work, void* stream) {
    CloudTransform T;
    double far_max = 0.0;
    const int rc = splat_args(points, N, transform, views, V, H, W, radius, r_min, r_max, blocks, zbuf, T, far_max);
    if (rc != 0) return rc;
    if ((flags & ~DMVS_SPLAT_NO_PRETEST) || ((uintptr_t)counts & 7u) || ((uintptr_t)work & 7u)) return DMVS_EINVAL;
    if (N > 0 && V > 0 && !counts) return DMVS_EINVAL;
    if (N == 0 || V == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(counts, 0, (size_t)V * DMVS_SPLAT_SLOTS * sizeof(int64_t), s);
    if (err == hipSuccess && work) err = hipMemsetAsync(work, 0, 2 * sizeof(uint64_t), s);
    if (err != hipSuccess) return (int)err;
    SplatParams p;
    p.radius = radius, p.r_min = r_min, p.r_max = r_max, p.tau1 = 1.0, p.scale = 1.0;
    p.H = H, p.W = W, p.pretest = (flags & DMVS_SPLAT_NO_PRETEST) ? 0 : 1;
    return splat_launch<false>(points, N, T, views, V, H, W, p, blocks, zbuf, nullptr, nullptr, reinterpret_cast<unsigned long long*>(counts), work, s);
}

extern "C" int dmvs_cloud_splat_sum_f32(const float* points, int64_t N, const double* transform, const double* views, int64_t V, int32_t H, int32_t W,
                                        double radius, double r_min, double r_max, double tau, double scale, int32_t blocks, const float* zbuf,
                                        uint64_t* sum, int32_t* cnt, void* stream) {
    CloudTransform T;
    double far_max = 0.0;
    const int rc = splat_args(points, N, transform, views, V, H, W, radius, r_min, r_max, blocks, zbuf, T, far_max);
    if (rc != 0) return rc;
    if (!splat_nonneg(tau) || ((uintptr_t)sum & 7u) || ((uintptr_t)cnt & 3u)) return DMVS_EINVAL;
    if (!cloud_pow2(scale) || (V > 0 && !cloud_sum_fits(N, far_max, scale))) return DMVS_EINVAL;
    const int64_t HW = (int64_t)H * W;
    if (N > 0 && V > 0 && HW > 0 && (!sum || !cnt)) return DMVS_EINVAL;
    if (N == 0 || V == 0 || HW == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(sum, 0, (size_t)V * HW * sizeof(uint64_t), s);
    if (err == hipSuccess) err = hipMemsetAsync(cnt, 0, (size_t)V * HW * sizeof(int32_t), s);
    if (err != hipSuccess) return (int)err;
    SplatParams p;
    p.radius = radius, p.r_min = r_min, p.r_max = r_max, p.tau1 = 1.0 + tau, p.scale = scale;
    p.H = H, p.W = W, p.pretest = 0;
    return splat_launch<true>(points, N, T, views, V, H, W, p, blocks, const_cast<float*>(zbuf), sum, cnt, nullptr, nullptr, s);
}
