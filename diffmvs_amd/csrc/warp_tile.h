// Shared by the tile-per-workgroup feature-gradient kernels (warp_bwd_win.hip: GetCost; warp_init_bwd_win.hip: the stage-1 plane
// sweep): the tile / window geometry, the per-pixel projection helpers, the footprint-box reduction, the passes over an LDS window
// (stage, gather, zero, scatter, flush), the walk over the footprints of a pixel's hypotheses, and GetCost's atomic-free pre-pass
// with its scratch layout.  Everything is file-local to the including translation unit (anonymous namespace).  Not for
// warp_bwd.hip: getcost_compact_kernel below would be a second copy of that code object; what it shares is in warp_bwd_common.h.
#pragma once
#include "warp_bwd_common.h"

namespace {

constexpr int TW = 16, TH = 16;      // reference-pixel tile of a workgroup (one lane per pixel)
constexpr int WW = 24;               // window width in texels
template <int C> struct WinCfg { static constexpr int WH = C == 32 ? 22 : 24; };   // rows: 76 KB (C=32) / 46 KB (C=16)

struct SampW {
    int x0, y0;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ void project_uv(const Ray& r, float depth, float& u, float& v, float& pz, bool& fin) {
    const float px = r.rx * depth + r.tx, py = r.ry * depth + r.ty;
    pz = r.rz * depth + r.tz;
    if (pz == 0.0f) pz += 1e-8f;
    // one reciprocal (hardware estimate + one Newton step: within an ulp of the IEEE quotient) shared by u and v
    float inv = __builtin_amdgcn_rcpf(pz);
    inv = fmaf(fmaf(-pz, inv, 1.0f), inv, inv);
    u = px * inv;
    v = py * inv;
    fin = fabsf(u) < 1.0e9f && fabsf(v) < 1.0e9f;
}

__device__ __forceinline__ SampW make_samp(float u, float v, bool fin, int Hs, int Ws) {
    const float fx = floorf(u), fy = floorf(v);
    SampW s;
    s.x0 = fin ? (int)fx : -4;          // -4: all four taps fail the range tests below
    s.y0 = fin ? (int)fy : -4;
    const float wx1 = u - fx, wy1 = v - fy, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
    // zero padding folded into the 1-D weights: a tap outside the image contributes nothing (grid_sample zeros)
    const float ax0 = (unsigned)s.x0 < (unsigned)Ws ? wx0 : 0.0f, ax1 = (unsigned)(s.x0 + 1) < (unsigned)Ws ? wx1 : 0.0f;
    const float ay0 = (unsigned)s.y0 < (unsigned)Hs ? wy0 : 0.0f, ay1 = (unsigned)(s.y0 + 1) < (unsigned)Hs ? wy1 : 0.0f;
    s.w00 = ax0 * ay0;
    s.w01 = ax1 * ay0;
    s.w10 = ax0 * ay1;
    s.w11 = ax1 * ay1;
    return s;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

struct WinBox { int x0, y0, ncols, nrows; };     // texel box of a footprint in a source view; ncols <= 0: every tap is padding

// Footprint box in one view of the workgroup's tile, from the two end depths of each lane's pixel (the projection of a
// depth interval is a straight image segment).  Returns false if some pixel's ends do not span a segment.  Workgroup-
// collective (one barrier); rd is the caller's reduction buffer, alternated between two by the caller: a fast wave may
// already be writing the next call's while a slow one still reads this one's.
__device__ __forceinline__ bool segment_box(const Ray& ray, float depth_first, float depth_last, bool live, int Hs, int Ws,
                                            int (*rd)[5], WinBox& box) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float u0, v0, z0, u1, v1, z1;
    bool f0, f1;
    project_uv(ray, depth_first, u0, v0, z0, f0);
    project_uv(ray, depth_last, u1, v1, z1, f1);
    int bad = live && (!f0 || !f1 || ((z0 < 0.0f) != (z1 < 0.0f)));     // a pole between the ends: not a segment
    int bx0 = 0x3fffffff, by0 = 0x3fffffff, bx1 = -0x3fffffff, by1 = -0x3fffffff;
    if (live && !bad) {
        const int ax = max((int)floorf(fminf(u0, u1)), 0), cx = min((int)floorf(fmaxf(u0, u1)) + 1, Ws - 1);
        const int ay = max((int)floorf(fminf(v0, v1)), 0), cy = min((int)floorf(fmaxf(v0, v1)) + 1, Hs - 1);
        if (ax <= cx && ay <= cy) {      // else: every tap of every hypothesis of this pixel is padding
            bx0 = ax; bx1 = cx; by0 = ay; by1 = cy;
        }
    }
    bx0 = wave_min(bx0); by0 = wave_min(by0); bx1 = wave_max(bx1); by1 = wave_max(by1); bad = wave_max(bad);
    if (lane == 0) {
        rd[wave][0] = bx0; rd[wave][1] = by0; rd[wave][2] = bx1; rd[wave][3] = by1; rd[wave][4] = bad;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < DMVS_BLOCK / 64; ++q) {
        bx0 = min(bx0, rd[q][0]); by0 = min(by0, rd[q][1]);
        bx1 = max(bx1, rd[q][2]); by1 = max(by1, rd[q][3]); bad = max(bad, rd[q][4]);
    }
    box.x0 = bx0; box.y0 = by0; box.ncols = bx1 - bx0 + 1; box.nrows = by1 - by0 + 1;
    return !bad;
}

// Footprint boxes of one 16x16 tile in every view, from the two end hypotheses of each pixel; returns whether all of them
// fit a win_w x win_h texel window.  Workgroup-collective.  sbox == nullptr: only the verdict is wanted.
__device__ __forceinline__ bool tile_boxes(const dmvs_getcost_desc& d, int b, int xc, int yc, bool live, float depth_first,
                                           float depth_last, int (*red)[DMVS_BLOCK / 64][5], int (*sbox)[4], int max_s, int win_w,
                                           int win_h) {
    bool allfit = d.S <= max_s;
    for (int s = 0; s < d.S && s < max_s; ++s) {
        Ray ray;
        ray.init(d.rt + ((long)b * d.S + s) * 12, (float)xc, (float)yc);
        WinBox bx;
        const bool seg = segment_box(ray, depth_first, depth_last, live, d.H, d.W, red[s & 1], bx);
        if (!seg || (bx.ncols > 0 && (bx.ncols > win_w || bx.nrows > win_h))) allfit = false;
        if (sbox && threadIdx.x == 0) {
            sbox[s][0] = bx.x0; sbox[s][1] = bx.y0; sbox[s][2] = bx.ncols; sbox[s][3] = bx.nrows;
        }
    }
    return allfit;
}

// this tile's position and the two end hypotheses of the lane's pixel (reference module.py:259-276)
template <int N>
__device__ __forceinline__ void tile_pixel(const dmvs_getcost_desc& d, int tile, int tiles_x, int tiles_y, int& b, int& xc, int& yc,
                                           bool& live, float& lo, float& step) {
    int tq = tile;
    const int txi = tq % tiles_x; tq /= tiles_x;
    const int tyi = tq % tiles_y;
    b = tq / tiles_y;
    const int x = txi * TW + (threadIdx.x & (TW - 1)), y = tyi * TH + (threadIdx.x >> 4);
    live = x < d.W && y < d.H;
    xc = min(x, d.W - 1);
    yc = min(y, d.H - 1);
    const long pc = ((long)b * d.H + yc) * d.W + xc;
    const float cur_inv = d.inv_depth[pc];
    float radius = (float)(N / 2) * d.interval;
    if (d.confidence) {
        const float r0 = d.min_radius * radius, r1 = d.max_radius * radius;
        radius = r0 + (1.0f - d.confidence[pc]) * (r1 - r0);
    }
    lo = cur_inv - radius;
    step = (cur_inv + radius - lo) / (float)(N - 1);
}

// ---- LDS window of a WinBox: row r, texel column c, channel q at float (r * WW + c) * TS + q, where TS = 4 * (NCH + 1) is
// the texel stride for NCH float4 of channels plus one of padding.  The window holds NCH * 4 channels of a global texel of
// CG floats (the caller offsets the global pointer to the window's first channel); Ws = texels per global row.

// the (column, float4) a lane moves in each of its SUBS turns at a window row: staging and flush share the assignment
template <int NCH>
struct WinLane {
    static constexpr int TS = 4 * (NCH + 1), SLOTS = WW * (NCH + 1), SUBS = (SLOTS + 63) / 64;
    int dcol[SUBS], dch[SUBS];          // dch == NCH: nothing to move (padding float4, or past the row)
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < SUBS; ++i) {
            const int slot = i * 64 + (threadIdx.x & 63);
            dcol[i] = slot / (NCH + 1);
            dch[i] = slot < SLOTS ? slot - dcol[i] * (NCH + 1) : NCH;
        }
    }
};

// LDS-DMA of the box of `view` into the window, a row per wave; the caller waits (DMVS_DMA_BARRIER)
template <int NCH, int CG>
__device__ __forceinline__ void win_stage(float* win, const WinLane<NCH>& ln, const WinBox& bx, const float* view, int Ws) {
    using L = WinLane<NCH>;
    for (int r = threadIdx.x >> 6; r < bx.nrows; r += DMVS_BLOCK / 64) {
        const float* rowp = view + ((long)(bx.y0 + r) * Ws + bx.x0) * CG;
#pragma unroll
        for (int i = 0; i < L::SUBS; ++i) {
            if (ln.dch[i] < NCH && ln.dcol[i] < bx.ncols) {
                const float* srcp = rowp + ln.dcol[i] * CG + ln.dch[i] * 4;
                float* dstp = win + (r * L::SLOTS + i * 64) * 4;
                __builtin_amdgcn_global_load_lds(srcp, DMVS_LDS_PTR(dstp), 16, 0, 0);
            }
        }
    }
}

template <int NCH>
__device__ __forceinline__ void win_zero(float* win, int nrows) {
    for (int e = threadIdx.x * 4; e < nrows * (WW * WinLane<NCH>::TS); e += DMVS_BLOCK * 4)
        *reinterpret_cast<float4*>(win + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// adds the window to the box of `gview`: one global atomic per window texel-channel, rows contiguous in global memory
template <int NCH, int CG>
__device__ __forceinline__ void win_flush(const float* win, const WinLane<NCH>& ln, const WinBox& bx, float* gview, int Ws) {
    using L = WinLane<NCH>;
    for (int r = threadIdx.x >> 6; r < bx.nrows; r += DMVS_BLOCK / 64) {
        float* growp = gview + ((long)(bx.y0 + r) * Ws + bx.x0) * CG;
#pragma unroll
        for (int i = 0; i < L::SUBS; ++i) {
            if (ln.dch[i] < NCH && ln.dcol[i] < bx.ncols) {
                const float4 q = *reinterpret_cast<const float4*>(win + (r * L::SLOTS + i * 64 + (threadIdx.x & 63)) * 4);
                float* gp = growp + ln.dcol[i] * CG + ln.dch[i] * 4;
                if (q.x != 0.0f) atomicAdd(gp, q.x);
                if (q.y != 0.0f) atomicAdd(gp + 1, q.y);
                if (q.z != 0.0f) atomicAdd(gp + 2, q.z);
                if (q.w != 0.0f) atomicAdd(gp + 3, q.w);
            }
        }
    }
}

// window offsets of the 2x2 footprint at (fx, fy); taps outside the box are clamped into it (they carry zero weight)
template <int NCH>
__device__ __forceinline__ void win_tap_offsets(int fx, int fy, const WinBox& bx, int (&off)[4]) {
    constexpr int TS = WinLane<NCH>::TS;
    const int xa = min(max(fx - bx.x0, 0), bx.ncols - 1), xb = min(max(fx + 1 - bx.x0, 0), bx.ncols - 1);
    const int ya = min(max(fy - bx.y0, 0), bx.nrows - 1), yb = min(max(fy + 1 - bx.y0, 0), bx.nrows - 1);
    const int ra = __mul24(ya, WW * TS), rb = __mul24(yb, WW * TS), ca = __mul24(xa, TS), cb = __mul24(xb, TS);
    off[0] = ra + ca; off[1] = ra + cb; off[2] = rb + ca; off[3] = rb + cb;
}

// Pass A at one footprint: gr[c] += Wt[t][group of c] * base[off[t] + c] over the four taps.  NG groups of CPG float4 each.
// base + off[t]: the window, or global memory where a box does not fit one.
template <int NCH, int CPG, int NG>
__device__ __forceinline__ void win_gather(const float* base, const int (&off)[4], const float (&Wt)[4][NG], float (&gr)[4 * NCH]) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const float4 q = *reinterpret_cast<const float4*>(base + off[t] + 4 * j);
            const float wt = Wt[t][j / CPG];
            gr[4 * j] = fmaf(wt, q.x, gr[4 * j]);
            gr[4 * j + 1] = fmaf(wt, q.y, gr[4 * j + 1]);
            gr[4 * j + 2] = fmaf(wt, q.z, gr[4 * j + 2]);
            gr[4 * j + 3] = fmaf(wt, q.w, gr[4 * j + 3]);
        }
}

// Pass B at one footprint: base[off[t] + c] += Wt[t][group of c] * inv_cg * ref4[c] with atomics (neighbouring pixels share
// texels).  A tap whose NG weights are all zero is a padding tap (make_samp) and is skipped.
template <int NCH, int CPG, int NG>
__device__ __forceinline__ void win_scatter(float* base, const int (&off)[4], const float (&Wt)[4][NG], const float4* ref4,
                                            float inv_cg) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        bool pad = true;
#pragma unroll
        for (int g = 0; g < NG; ++g) pad = pad && Wt[t][g] == 0.0f;
        if (pad) continue;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const float4 q = ref4[j];
            const float wt = Wt[t][j / CPG] * inv_cg;
            atomicAdd(base + off[t] + 4 * j, wt * q.x);
            atomicAdd(base + off[t] + 4 * j + 1, wt * q.y);
            atomicAdd(base + off[t] + 4 * j + 2, wt * q.z);
            atomicAdd(base + off[t] + 4 * j + 3, wt * q.w);
        }
    }
}

// Walks hypotheses k0 .. k1-1 of the lane's pixel and calls emit(fx, fy, Wt) once per distinct 2x2 footprint with the tap
// weights accumulated over the hypotheses that share it: Wt[t][g] = sum_k g_k[g] * scale * tapweight_t(k).  The hypotheses of a
// pixel walk the epipolar line in sub-texel steps, so a footprint serves several.  sample(k, sp, g) gives hypothesis k's tap
// position and weights and its NG group gradients; scale (GetCost's view weight) multiplies them here, after the emit:
// multiplied inside the sampler, GetCost's C = 32 kernels spill more.  A rolled loop with ONE emit site (an emit body is 4 * C LDS reads or atomics: neither
// unrolled nor repeated after the loop): iteration k1 only flushes the last footprint, so sample is also called with
// k == k1 and its result ignored -- a sampler that indexes memory with k clamps it.
template <int NG, class Sample, class Emit>
__device__ __forceinline__ void walk_footprints(int k0, int k1, float scale, Sample&& sample, Emit&& emit) {
    int fx = 0, fy = 0;
    bool open = false;
    float Wt[4][NG];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < NG; ++g) Wt[t][g] = 0.0f;
#pragma unroll 1
    for (int k = k0; k <= k1; ++k) {
        SampW sp;
        float gk[NG];
        sample(k, sp, gk);
        const bool change = k == k1 || !open || sp.x0 != fx || sp.y0 != fy;
        if (open && change) emit(fx, fy, Wt);
        if (k == k1) break;
        if (change) {
            open = true;
            fx = sp.x0;
            fy = sp.y0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int g = 0; g < NG; ++g) Wt[t][g] = 0.0f;
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float gc = gk[g] * scale;
            Wt[0][g] = fmaf(gc, sp.w00, Wt[0][g]);
            Wt[1][g] = fmaf(gc, sp.w01, Wt[1][g]);
            Wt[2][g] = fmaf(gc, sp.w10, Wt[2][g]);
            Wt[3][g] = fmaf(gc, sp.w11, Wt[3][g]);
        }
    }
}

// Scratch layout (int32), n = number of tiles:  [0] tiles listed for the gather kernel, [1] mode (1 = the gather
// kernel takes every tile), [2..3] unused, flags[n] (1 = some view's footprint exceeds the window), list[n] (the
// flagged tiles, ascending), boxes[n][MAXS][4] (x0, y0, ncols, nrows per view).  No atomics anywhere: same-address
// device atomics from ~10^3 workgroups serialise at ~0.1 us each, more than the whole pre-pass costs.
constexpr int MAXS = DMVS_GETCOST_MAX_WINDOW_VIEWS;       // per-view footprint boxes kept per tile (entry points fall back to the gather kernels beyond)
__device__ __forceinline__ int* ws_flags(int* ws) { return ws + 4; }
__device__ __forceinline__ int* ws_list(int* ws, int ntiles) { return ws + 4 + ntiles; }
__device__ __forceinline__ int* ws_boxes(int* ws, int ntiles) { return ws + 4 + 2 * ntiles; }

// Pre-pass 1: every tile's per-view footprint boxes and its fit flag.
template <int N>
__global__ void __launch_bounds__(DMVS_BLOCK) getcost_fit_kernel(const dmvs_getcost_desc d, int tiles_x, int tiles_y, int win_w,
                                                                 int win_h) {
    __shared__ int red[2][DMVS_BLOCK / 64][5];
    __shared__ int sbox[MAXS][4];
    const int tile = blockIdx.x, ntiles = gridDim.x;
    int b, xc, yc;
    bool live;
    float lo, step;
    tile_pixel<N>(d, tile, tiles_x, tiles_y, b, xc, yc, live, lo, step);
    const float dmin = d.disp_min[b], dmax = d.disp_max[b];
    const bool fits = tile_boxes(d, b, xc, yc, live, hyp_depth(0, lo, step, dmin, dmax), hyp_depth(N - 1, lo, step, dmin, dmax), red,
                                 sbox, MAXS, win_w, win_h);
    __syncthreads();
    if (threadIdx.x < 4 * MAXS && threadIdx.x < 4 * d.S)
        ws_boxes(d.worklist, ntiles)[(size_t)tile * (4 * MAXS) + threadIdx.x] = sbox[threadIdx.x >> 2][threadIdx.x & 3];
    if (threadIdx.x == 0) ws_flags(d.worklist)[tile] = fits ? 0 : 1;
}

// Pre-pass 2 (one workgroup): count the flagged tiles, pick the mode, list the flagged tiles in ascending order.
// If most tiles are flagged (a depth map that is noise rather than surfaces, e.g. an untrained network) the window
// kernel stands down and the gather kernel takes every tile: the hybrid only pays off while the windows carry a good
// share of the work.
__global__ void __launch_bounds__(DMVS_BLOCK) getcost_compact_kernel(int* __restrict__ ws, int ntiles) {
    __shared__ int cnt[DMVS_BLOCK + 1];
    const int tid = threadIdx.x;
    const int seg = (ntiles + DMVS_BLOCK - 1) / DMVS_BLOCK, t0 = tid * seg, t1 = min(t0 + seg, ntiles);
    const int* flags = ws_flags(ws);
    int c = 0;
    for (int t = t0; t < t1; ++t) c += flags[t];
    cnt[tid + 1] = c;
    __syncthreads();
    if (tid == 0) {
        cnt[0] = 0;
        for (int i = 1; i <= DMVS_BLOCK; ++i) cnt[i] += cnt[i - 1];
        ws[0] = cnt[DMVS_BLOCK];
        ws[1] = (long)cnt[DMVS_BLOCK] * 4 > (long)ntiles * 3 ? 1 : 0;      // > 75 % flagged: gather everything
    }
    __syncthreads();
    int* list = ws_list(ws, ntiles);
    int o = cnt[tid];
    for (int t = t0; t < t1; ++t)
        if (flags[t]) list[o++] = t;
}

// launches the two pre-pass kernels for d (d.worklist must be set): per-tile fit flags, boxes, mode, ordered list
template <int C>
int launch_getcost_prepass(const dmvs_getcost_desc& d, hipStream_t st) {
    const int tiles_x = (d.W + TW - 1) / TW, tiles_y = (d.H + TH - 1) / TH;
    dim3 grid((unsigned)(tiles_x * tiles_y * d.B)), block(DMVS_BLOCK);
    if (d.n == 4) hipLaunchKernelGGL((getcost_fit_kernel<4>), grid, block, 0, st, d, tiles_x, tiles_y, WW, WinCfg<C>::WH);
    else if (d.n == 6) hipLaunchKernelGGL((getcost_fit_kernel<6>), grid, block, 0, st, d, tiles_x, tiles_y, WW, WinCfg<C>::WH);
    else return DMVS_EINVAL;
    hipLaunchKernelGGL(getcost_compact_kernel, dim3(1), block, 0, st, d.worklist, (int)grid.x);
    return dmvs_launch_status();
}

}  // namespace
