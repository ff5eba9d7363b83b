// Oriented normals of a depth map (diffmvs_amd/fusion.py): dmvs_depth_normals_f32, a least-squares plane in INVERSE depth over a
// (2r + 1)^2 window of the pixel grid.  The contract (support, sums, cofactors, slots) is in include/dmvs.h.
//
// One workgroup per 32 x 8 tile of one view, one lane per pixel.  The tile and its halo of r pixels are staged ONCE in LDS as the fp64
// inverse depth w = 1.0 / depth, with w = 0 for "not usable" (outside the image, masked out, depth not finite or <= 0: a usable w is
// strictly positive), so the 9 .. 81 taps of a pixel cost one ds_read_b64 each and no divide, no global read and no image-border test.
// A half-wave reads 32 consecutive doubles of one LDS row: every bank once.  The window is unrolled (R is a template argument): the
// offsets, their squares and products are literals, the six integer sums are conditional adds, the three fp64 sums a multiply and an add
// each (no contraction).  A launch carries up to DMVS_NORMAL_VIEW_CHUNK views as a KERNEL ARGUMENT (27 doubles each, scalar loads);
// blockIdx.x runs over (view, tile row, tile column).  Each pixel leaves with one 16-byte store.  The slots are 32-bit LDS counters, then
// one u64 integer atomic per non-zero slot per workgroup.  Nothing depends on the tile shape or on the launch order, and there is no
// floating-point atomic.
#include <math.h>

#include "dmvs_common.h"
#include "dmvs_lds_poison.h"

namespace {

#define NORMAL_VC DMVS_NORMAL_VIEW_CHUNK
#define NORMAL_TW 32
#define NORMAL_TH 8
static_assert(NORMAL_TW * NORMAL_TH == DMVS_BLOCK, "one lane per pixel of the tile");

struct NormalView { double K[9], Kinv[9], R[9]; };                   // = DMVS_NORMAL_CAM_DOUBLES doubles, the layout of `cams`
struct NormalViews {
    NormalView v[NORMAL_VC];
    int nv;                                                          // live views of this launch
};
struct NormalParams {
    double rel_jump;
    int H, W, min_pts, tiles_x, tiles_y;
};

template <int R>
__global__ void __launch_bounds__(DMVS_BLOCK)
depth_normals_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid, NormalViews vs, NormalParams p, float4* __restrict__ out,
                     unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
    constexpr int LW = NORMAL_TW + 2 * R, LH = NORMAL_TH + 2 * R;
    __shared__ double w[LH * LW];
    __shared__ int slots[DMVS_NORMAL_SLOTS];
    DMVS_LDS_POISON(w);
    DMVS_LDS_POISON(slots);
    const int tid = threadIdx.x;
    const unsigned per_view = (unsigned)p.tiles_x * (unsigned)p.tiles_y;
    const int view = (int)(blockIdx.x / per_view);                   // (< vs.nv: the grid is nv * per_view workgroups)
    const unsigned tile = blockIdx.x % per_view;
    const int x0 = (int)(tile % (unsigned)p.tiles_x) * NORMAL_TW, y0 = (int)(tile / (unsigned)p.tiles_x) * NORMAL_TH;
    const long HW = (long)p.H * p.W, plane = (long)view * HW;

    if (tid < DMVS_NORMAL_SLOTS) slots[tid] = 0;
    for (int i = tid; i < LH * LW; i += DMVS_BLOCK) {
        const int gy = y0 - R + i / LW, gx = x0 - R + i % LW;
        double wi = 0.0;
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
            const long j = plane + (long)gy * p.W + gx;
            const float d = depth[j];
            if ((!valid || valid[j] != 0) && isfinite(d) && d > 0.0f) wi = 1.0 / (double)d;
        }
        w[i] = wi;
    }
    __syncthreads();

    const int lx = tid % NORMAL_TW, ly = tid / NORMAL_TW, x = x0 + lx, y = y0 + ly;
    if (x < p.W && y < p.H) {
        const double* c = w + (ly + R) * LW + (lx + R);
        const double wc = c[0];
        int slot = 0;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (wc > 0.0) {
            const double gate = p.rel_jump * wc;
            int n = 0, Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0;
            double Tw = 0.0, Tx = 0.0, Ty = 0.0;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const double wj = c[dy * LW + dx];
                    const double dl = wj - wc;
                    if (wj > 0.0 && fabs(dl) <= gate) {
                        n += 1, Sx += dx, Sy += dy, Sxx += dx * dx, Sxy += dx * dy, Syy += dy * dy;
                        Tw += dl;
                        Tx += (double)dx * dl;
                        Ty += (double)dy * dl;
                    }
                }
            }
            const int C00 = Syy * n - Sy * Sy, C01 = -(Sxy * n - Sx * Sy), C02 = Sxy * Sy - Syy * Sx;
            const int C11 = Sxx * n - Sx * Sx, C12 = -(Sxx * Sy - Sxy * Sx), C22 = Sxx * Syy - Sxy * Sxy;
            const int D = Sxx * C00 + Sxy * C01 + Sx * C02;          // (|D| < 2^25 at R = 4: n <= 81, Sxx and Syy <= 540)
            slot = 1;
            if (n >= p.min_pts && D != 0) {
                const NormalView& vw = vs.v[view];
                const double Dd = (double)D;
                const double a = (((double)C00 * Tx + (double)C01 * Ty) + (double)C02 * Tw) / Dd;
                const double b = (((double)C01 * Tx + (double)C11 * Ty) + (double)C12 * Tw) / Dd;
                const double cc = (((double)C02 * Tx + (double)C12 * Ty) + (double)C22 * Tw) / Dd;
                const double xd = (double)x, yd = (double)y;
                const double wf = wc + cc;
                const double c0 = (wf - a * xd) - b * yd;
                const double g0 = (vw.K[0] * a + vw.K[3] * b) + vw.K[6] * c0;
                const double g1 = (vw.K[1] * a + vw.K[4] * b) + vw.K[7] * c0;
                const double g2 = (vw.K[2] * a + vw.K[5] * b) + vw.K[8] * c0;
                const double len = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
                const double r0 = (vw.Kinv[0] * xd + vw.Kinv[1] * yd) + vw.Kinv[2];
                const double r1 = (vw.Kinv[3] * xd + vw.Kinv[4] * yd) + vw.Kinv[5];
                const double r2 = (vw.Kinv[6] * xd + vw.Kinv[7] * yd) + vw.Kinv[8];
                const double rl = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
                slot = 2;
                if (wf > 0.0 && isfinite(len) && len != 0.0) {
                    slot = 3;
                    const double n0 = -g0 / len, n1 = -g1 / len, n2 = -g2 / len;
                    o.x = (float)((vw.R[0] * n0 + vw.R[3] * n1) + vw.R[6] * n2);
                    o.y = (float)((vw.R[1] * n0 + vw.R[4] * n1) + vw.R[7] * n2);
                    o.z = (float)((vw.R[2] * n0 + vw.R[5] * n1) + vw.R[8] * n2);
                    o.w = (float)(wf / (len * rl));
                }
            }
        }
        out[plane + (long)y * p.W + x] = o;
        atomicAdd(&slots[slot], 1);
    }
    __syncthreads();
    if (tid < DMVS_NORMAL_SLOTS && slots[tid]) atomicAdd(counts + view * DMVS_NORMAL_SLOTS + tid, (unsigned long long)slots[tid]);
}

template <int R>
inline void normals_launch(dim3 grid, hipStream_t s, const float* depth, const uint8_t* valid, const NormalViews& vs, const NormalParams& p, float4* out,
                           unsigned long long* counts) {
    hipLaunchKernelGGL(depth_normals_kernel<R>, grid, dim3(DMVS_BLOCK), 0, s, depth, valid, vs, p, out, counts);
}

}  // namespace

extern "C" int dmvs_depth_normals_f32(const float* depth, const uint8_t* valid, const double* cams, int64_t B, int32_t H, int32_t W, int32_t radius,
                                      double rel_jump, int32_t min_pts, float* out, int64_t* counts, void* stream) {
    if (B < 0 || H < 0 || W < 0) return DMVS_EINVAL;
    const int64_t HW = (int64_t)H * W;
    if (HW > 2147483647L || (HW > 0 && B > (1L << 40) / HW)) return DMVS_EINVAL;      // a plane is indexed in 31 bits, the maps in 40
    if (radius < 1 || radius > DMVS_NORMAL_MAX_RADIUS) return DMVS_EINVAL;
    if (min_pts < 3 || min_pts > (2 * radius + 1) * (2 * radius + 1)) return DMVS_EINVAL;
    if (!(rel_jump >= 0.0) || !isfinite(rel_jump)) return DMVS_EINVAL;
    if (((uintptr_t)depth & 3u) || ((uintptr_t)out & 15u) || ((uintptr_t)counts & 7u)) return DMVS_EINVAL;
    const bool work = B > 0 && HW > 0;
    if (work && (!depth || !cams || !out || !counts)) return DMVS_EINVAL;
    if (cams)
        for (int64_t k = 0; k < B * DMVS_NORMAL_CAM_DOUBLES; ++k)
            if (!isfinite(cams[k])) return DMVS_EINVAL;
    if (!work) return 0;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t err = hipMemsetAsync(counts, 0, (size_t)B * DMVS_NORMAL_SLOTS * sizeof(int64_t), s);
    if (err != hipSuccess) return (int)err;
    NormalParams p;
    p.rel_jump = rel_jump, p.H = H, p.W = W, p.min_pts = min_pts;
    p.tiles_x = (int)dmvs_ceil_div(W, NORMAL_TW), p.tiles_y = (int)dmvs_ceil_div(H, NORMAL_TH);
    const long per_view = (long)p.tiles_x * p.tiles_y;               // (< 2^27: H W < 2^31 and a tile is 256 pixels, ragged edges included)
    for (int64_t v0 = 0; v0 < B; v0 += NORMAL_VC) {
        NormalViews vs;
        vs.nv = (int)(B - v0 < NORMAL_VC ? B - v0 : NORMAL_VC);
        for (int k = 0; k < NORMAL_VC; ++k) {
            const double* q = cams + (v0 + (k < vs.nv ? k : 0)) * DMVS_NORMAL_CAM_DOUBLES;      // (unused slots repeat the first: never read)
            for (int j = 0; j < 9; ++j) vs.v[k].K[j] = q[j], vs.v[k].Kinv[j] = q[9 + j], vs.v[k].R[j] = q[18 + j];
        }
        const dim3 grid((unsigned)(per_view * vs.nv));
        const float* dp = depth + v0 * HW;
        const uint8_t* vp = valid ? valid + v0 * HW : nullptr;
        float4* op = reinterpret_cast<float4*>(out) + v0 * HW;
        unsigned long long* ct = reinterpret_cast<unsigned long long*>(counts) + v0 * DMVS_NORMAL_SLOTS;
        switch (radius) {
            case 1: normals_launch<1>(grid, s, dp, vp, vs, p, op, ct); break;
            case 2: normals_launch<2>(grid, s, dp, vp, vs, p, op, ct); break;
            case 3: normals_launch<3>(grid, s, dp, vp, vs, p, op, ct); break;
            default: normals_launch<4>(grid, s, dp, vp, vs, p, op, ct); break;
        }
        const int rc = dmvs_launch_status();
        if (rc != 0) return rc;
    }
    return 0;
}
