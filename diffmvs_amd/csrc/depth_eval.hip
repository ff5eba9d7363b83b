// Depth-map scoring (diffmvs_amd/depth_eval.py): dmvs_depth_stats_f32, the per-item integer rows behind abs / abs-rel / RMSE / inlier shares.
//
// One launch scores [B, HW] pixels: blockIdx.y is the batch item, blockIdx.x walks the item's pixels in a grid-stride loop.  A pixel costs
// 8 or 12 bytes of HBM and one fp64 divide; the kernel is a stream, so the fp64 arithmetic hides behind the loads.  Every lane keeps the
// DMVS_DEPTH_SLOTS + T counters of include/dmvs.h as u64 registers; cloud_block_sum (cloud_walk.h: shuffles, LDS, ONE integer atomic per
// slot per workgroup) folds them into the item's row.  Integer sums are associative: the row is bitwise independent of the grid shape, of
// the launch order and of the load width (the rule of dmvs_cloud_stats_f32 and the GroupNorm statistics).
// Loads: where est, gt and mask sit at the same offset inside a 16-byte line (`phase`, in elements), an item's pixels are a scalar head up
// to the first line boundary, float4 quads, and a scalar tail -- items of odd size then still stream 16 bytes per lane.  Otherwise scalars.
#include "cloud_walk.h"      // CloudSums / cloud_block_sum and the host-side shaping of a fixed-point launch

namespace {

#define DEPTH_MAX_T DMVS_DEPTH_MAX_THRESHOLDS
#define DEPTH_NCOUNT (DMVS_DEPTH_SLOTS + DEPTH_MAX_T)

struct DepthParams {
    double thr[DEPTH_MAX_T];      // unused slots hold -inf: never below
    double band_lo, band_hi, big, big_sq, scale, scale_sq;
};

typedef CloudSums<DEPTH_NCOUNT> DepthSums;

__device__ __forceinline__ void depth_score(DepthSums& acc, float est, float gt, float m, const DepthParams& p) {
#pragma clang fp contract(off)
    if (!(m > 0.5f)) return;
    ++acc.v[0];
    if (!isfinite(est) || !isfinite(gt) || !(gt > 0.0f)) {
        ++acc.v[2];
        return;
    }
    const double e = (double)est - (double)gt, a = fabs(e);
    if (!(a >= p.band_lo && a <= p.band_hi)) return;
    const double rel = a / (double)gt, sq = e * e;
    ++acc.v[1];
    acc.v[3] += (a > p.big ? 1ull : 0ull) + (rel > p.big ? 1ull : 0ull) + (sq > p.big_sq ? 1ull : 0ull);
    acc.v[4] += (unsigned long long)llrint(fmin(a, p.big) * p.scale);
    acc.v[5] += (unsigned long long)llrint(fmin(rel, p.big) * p.scale);
    acc.v[6] += (unsigned long long)llrint(fmin(sq, p.big_sq) * p.scale_sq);
#pragma unroll
    for (int t = 0; t < DEPTH_MAX_T; ++t) acc.v[DMVS_DEPTH_SLOTS + t] += a < p.thr[t] ? 1ull : 0ull;
}

template <bool VEC, bool MASK>
__global__ void __launch_bounds__(DMVS_BLOCK)
depth_stats_kernel(const float* __restrict__ est, const float* __restrict__ gt, const float* __restrict__ mask, long HW, int phase, DepthParams p,
                   int T, unsigned long long* __restrict__ out) {
    const long base = (long)blockIdx.y * HW;
    est += base, gt += base;
    if (MASK) mask += base;
    DepthSums acc = {};
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    long head = 0, quads = 0;
    if (VEC) {
        head = (4 - (((long)phase + base) & 3)) & 3;      // scalars in front of the item's first 16-byte line
        head = head < HW ? head : HW;
        quads = (HW - head) >> 2;
        for (long q = tid; q < quads; q += stride) {
            const long i = head + 4 * q;
            const float4 e4 = *reinterpret_cast<const float4*>(est + i), g4 = *reinterpret_cast<const float4*>(gt + i);
            float4 m4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (MASK) m4 = *reinterpret_cast<const float4*>(mask + i);
            depth_score(acc, e4.x, g4.x, m4.x, p);
            depth_score(acc, e4.y, g4.y, m4.y, p);
            depth_score(acc, e4.z, g4.z, m4.z, p);
            depth_score(acc, e4.w, g4.w, m4.w, p);
        }
    }
    const long rest = HW - 4 * quads;                     // VEC: head + tail (at most 6); else every pixel
    for (long k = tid; k < rest; k += stride) {
        const long i = k < head ? k : k + 4 * quads;
        depth_score(acc, est[i], gt[i], MASK ? mask[i] : 1.0f, p);
    }
    cloud_block_sum(acc, DMVS_DEPTH_SLOTS + T, out + (long)blockIdx.y * (DMVS_DEPTH_SLOTS + T));
}

inline bool depth_aligned4(const void* q) { return ((uintptr_t)q & 3u) == 0; }
inline int depth_phase(const void* q) { return (int)(((uintptr_t)q >> 2) & 3u); }

}  // namespace

extern "C" int dmvs_depth_stats_f32(const float* est, const float* gt, const float* mask, int64_t B, int64_t HW, const float* thresholds, int32_t T,
                                    double band_lo, double band_hi, double big, double scale, int32_t blocks, int64_t* out, void* stream) {
    if (B < 0 || HW < 0 || B > 65535 || T < 0 || T > DEPTH_MAX_T || blocks < 0 || (T > 0 && !thresholds)) return DMVS_EINVAL;
    if (B > 0 && !out) return DMVS_EINVAL;
    if (B > 0 && HW > 0 && (!est || !gt)) return DMVS_EINVAL;
    if (!depth_aligned4(est) || !depth_aligned4(gt) || !depth_aligned4(mask) || ((uintptr_t)out & 7u)) return DMVS_EINVAL;
    if (!(big > 0.0) || !isfinite(big) || !cloud_pow2(scale) || !cloud_sum_fits(HW, big, scale)) return DMVS_EINVAL;
    if (!(band_lo >= 0.0) || !(band_hi >= band_lo)) return DMVS_EINVAL;      // (false for NaN)
    DepthParams p;
    for (int t = 0; t < DEPTH_MAX_T; ++t) {
        if (t < T && !(thresholds[t] == thresholds[t])) return DMVS_EINVAL;
        p.thr[t] = t < T ? (double)thresholds[t] : -INFINITY;
    }
    int ex = 0;
    const double mant = frexp(big, &ex);                  // big = mant * 2^ex, mant in [0.5, 1): the power of two at or above big is 2^ex, or big itself
    p.band_lo = band_lo, p.band_hi = band_hi, p.big = big, p.big_sq = big * big, p.scale = scale;
    p.scale_sq = ldexp(scale, -(mant == 0.5 ? ex - 1 : ex));
    if (!(p.scale_sq > 0.0) || !isfinite(p.scale_sq) || !isfinite(p.big_sq)) return DMVS_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(out);
    const hipError_t err = hipMemsetAsync(acc, 0, (size_t)B * (DMVS_DEPTH_SLOTS + T) * sizeof(unsigned long long), s);
    if (err != hipSuccess) return (int)err;
    if (HW == 0) return 0;
    const bool vec = depth_phase(est) == depth_phase(gt) && (!mask || depth_phase(mask) == depth_phase(est));
    // a lane of the 16-byte path takes four pixels per trip; a few thousand workgroups over all items keep the atomics few
    const long per_block = (long)DMVS_BLOCK * (vec ? 4 : 1), nb = (HW + per_block - 1) / per_block;
    const long cap = blocks > 0 ? blocks : (4096 / B > 1 ? 4096 / B : 1);
    dim3 grid((unsigned)(nb < cap ? nb : cap), (unsigned)B), block(DMVS_BLOCK);
    const int phase = depth_phase(est), Ti = (int)T;
    if (vec && mask) hipLaunchKernelGGL((depth_stats_kernel<true, true>), grid, block, 0, s, est, gt, mask, (long)HW, phase, p, Ti, acc);
    else if (vec) hipLaunchKernelGGL((depth_stats_kernel<true, false>), grid, block, 0, s, est, gt, mask, (long)HW, phase, p, Ti, acc);
    else if (mask) hipLaunchKernelGGL((depth_stats_kernel<false, true>), grid, block, 0, s, est, gt, mask, (long)HW, phase, p, Ti, acc);
    else hipLaunchKernelGGL((depth_stats_kernel<false, false>), grid, block, 0, s, est, gt, mask, (long)HW, phase, p, Ti, acc);
    return dmvs_launch_status();
}
