// Backward of the stage-1 plane sweep (dmvs_warp_corr_init_f32) w.r.t. the image features through LDS windows: the two
// passes of warp_bwd_win.hip (the window machinery of warp_tile.h) over depth chunks whose footprint fits a window.
//   workgroup = one 16x16 pixel tile x one source view; per depth chunk and channel half:
//     A. stage the source half-window (LDS-DMA), accumulate grad_ref from it;
//     B. zero the window, scatter W_t[g] * ref into it with LDS atomics, flush it row-wise to grad_src with one global
//        atomic per texel-channel.
//   W_t[g] = sum over the planes that share a 2x2 footprint of gcor[g, k] * tapweight_t.
// grad_ref is shared by the S workgroups of a tile: zeroed by the entry point, accumulated with one global atomic per
// (pixel, channel, view).  A chunk whose box exceeds the window gathers / scatters per lane in global memory.
#include "warp_tile.h"

namespace {

constexpr int IWHB = 20;

template <int C>
__global__ void __launch_bounds__(DMVS_BLOCK, 2)
warp_init_bwd_win_kernel(const float* __restrict__ ref, const float* __restrict__ src, const float* __restrict__ rt,
                         const float* __restrict__ disp_min, const float* __restrict__ disp_max, const float* __restrict__ gcor,
                         float* __restrict__ gref, float* __restrict__ gsrc, int B, int S, int D, int H, int W, int Hs, int Ws,
                         int tiles_x, int tiles_y) {
    constexpr int G = 4, CH = C / 2, NCH = CH / 4, CPG = NCH / 2;
    constexpr int MAXD = 256;
    __shared__ __attribute__((aligned(16))) float win[WW * IWHB * WinLane<NCH>::TS];
    __shared__ float s_depth[MAXD];
    __shared__ int red[2][DMVS_BLOCK / 64][5];

    const int tid = threadIdx.x;
    int tq = (int)dmvs_xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int txi = tq % tiles_x; tq /= tiles_x;
    const int tyi = tq % tiles_y;
    const int b = tq / tiles_y;
    const int s = blockIdx.y;
    const int x = txi * TW + (tid & (TW - 1)), y = tyi * TH + (tid >> 4);
    const bool live = x < W && y < H;
    const int xc = min(x, W - 1), yc = min(y, H - 1);
    const long hw = (long)H * W, yx = (long)yc * W + xc;

    const float dmin = disp_min[b], dmax = disp_max[b], dm1 = (float)(D - 1);
    for (int k = tid; k < D; k += DMVS_BLOCK) s_depth[k] = dmvs_disp_to_depth((float)k / dm1, dmin, dmax);

    Ray ray;
    ray.init(rt + ((long)b * S + s) * 12, (float)xc, (float)yc);
    const long voff = ((long)s * B + b) * (long)Hs * Ws * C;
    const float* view = src + voff;
    float* gview = gsrc + voff;
    const float* gp = gcor + (((long)b * S + s) * G) * D * hw + yx;        // + (g * D + k) * hw
    const float* refpix = ref + ((long)b * hw + yx) * C;
    const float inv_cg = 1.0f / (float)(C / G);

    WinLane<NCH> ln;
    ln.init();
    __syncthreads();

    int nred = 0;       // segment_box's reduction buffer alternates from one call to the next
    WinBox full;
    const bool seg = segment_box(ray, s_depth[0], s_depth[D - 1], live, Hs, Ws, red[nred++ & 1], full);
    int nchunk = 1;
    if (seg && full.ncols > 0) {
        const int ex = max(full.ncols - (WW - 5), 0), ey = max(full.nrows - (IWHB - 1), 0);
        nchunk = 1 + max((ex + 4) / 5, ey);
    } else if (!seg) {
        nchunk = max(D / 4, 1);
    }
    nchunk = min(nchunk, D);
    const int dc = (D + nchunk - 1) / nchunk;

    float gr[2][CH];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < CH; ++c) gr[h][c] = 0.0f;

    for (int k0 = 0; k0 < D; k0 += dc) {
        const int k1 = min(k0 + dc, D);
        WinBox bx;
        const bool okseg = segment_box(ray, s_depth[k0], s_depth[k1 - 1], live, Hs, Ws, red[nred++ & 1], bx);
        if (okseg && bx.ncols <= 0) continue;       // every tap of every plane of the chunk is padding: no gradient
        const bool fits = okseg && bx.ncols <= WW && bx.nrows <= IWHB;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* vh = view + h * CH;
            float* gvh = gview + h * CH;
            // plane k of the chunk for walk_footprints: its footprint and the two group gradients of this channel half
            auto sample = [&](int k, SampW& sp, float (&g)[2]) {
                const int kk = min(k, k1 - 1);      // k == k1: sampled once more, not used
                float u, v, z;
                bool fin;
                project_uv(ray, s_depth[kk], u, v, z, fin);
                sp = make_samp(u, v, fin, Hs, Ws);
                g[0] = live ? gp[((long)(2 * h) * D + kk) * hw] : 0.0f;
                g[1] = live ? gp[((long)(2 * h + 1) * D + kk) * hw] : 0.0f;
            };
            // a chunk that does not fit a window (!fits) addresses the four taps in global memory, clamped into the image
            auto tap_offsets = [&](int fx, int fy, int (&off)[4]) {
                if (fits) {
                    win_tap_offsets<NCH>(fx, fy, bx, off);
                } else {
                    const int xa = min(max(fx, 0), Ws - 1), xb = min(max(fx + 1, 0), Ws - 1);
                    const int ya = min(max(fy, 0), Hs - 1), yb = min(max(fy + 1, 0), Hs - 1);
                    off[0] = (ya * Ws + xa) * C; off[1] = (ya * Ws + xb) * C; off[2] = (yb * Ws + xa) * C; off[3] = (yb * Ws + xb) * C;
                }
            };

            __syncthreads();        // previous window (flush of the last pass) is done
            if (fits) win_stage<NCH, C>(win, ln, bx, vh, Ws);
            DMVS_DMA_BARRIER();        // source half-window resident

            // ---- pass A: grad_ref
            walk_footprints<2>(k0, k1, 1.0f, sample, [&](int fx, int fy, const float (&Wt)[4][2]) {
                int off[4];
                tap_offsets(fx, fy, off);
                win_gather<NCH, CPG, 2>(fits ? win : vh, off, Wt, gr[h]);
            });
            if (fits) {
                __syncthreads();    // every lane is done with the source window
                win_zero<NCH>(win, bx.nrows);
                __syncthreads();
            }

            // ---- pass B: scatter (LDS gradient tile, or straight to grad_src when the chunk does not fit)
            const float4* rp4 = reinterpret_cast<const float4*>(refpix + h * CH);
            walk_footprints<2>(k0, k1, 1.0f, sample, [&](int fx, int fy, const float (&Wt)[4][2]) {
                int off[4];
                tap_offsets(fx, fy, off);
                win_scatter<NCH, CPG, 2>(fits ? win : gvh, off, Wt, rp4, inv_cg);
            });
            if (fits) {
                __syncthreads();
                win_flush<NCH, C>(win, ln, bx, gvh, Ws);
            }
        }
    }
    if (live) {
        float* go = gref + ((long)b * hw + yx) * C;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (gr[h][c] != 0.0f) atomicAdd(go + h * CH + c, gr[h][c] * inv_cg);
    }
}

}  // namespace

// called by dmvs_warp_corr_init_bwd_f32 (warp_bwd.hip) for C = 48
int dmvs_warp_init_bwd_win_dispatch(const float* ref, const float* src, const float* rt, const float* disp_min, const float* disp_max,
                                    const float* gcor, float* gref, float* gsrc, int B, int S, int C, int D, int H, int W, int Hs,
                                    int Ws, hipStream_t st) {
    if (C != 48 || D > 256) return DMVS_EINVAL;
    hipError_t e = hipMemsetAsync(gref, 0, sizeof(float) * (size_t)B * H * W * C, st);
    if (e != hipSuccess) return (int)e;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    dim3 grid((unsigned)(tiles_x * tiles_y * B), (unsigned)S), block(DMVS_BLOCK);
    hipLaunchKernelGGL((warp_init_bwd_win_kernel<48>), grid, block, 0, st, ref, src, rt, disp_min, disp_max, gcor, gref, gsrc, B, S, D,
                       H, W, Hs, Ws, tiles_x, tiles_y);
    return dmvs_launch_status();
}
