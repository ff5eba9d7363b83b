// A surface from depth maps (diffmvs_amd/mesh.py): dmvs_tsdf_integrate_f32 averages the truncated signed distance of every view into a
// dense voxel volume, dmvs_tsdf_flags_u8 / dmvs_tsdf_vertices_f32 / dmvs_tsdf_faces_i32 take the zero set out of it as a surface-nets
// mesh.  The contract (the fp64 order, the integer sums, the numbering of vertices and faces) is in include/dmvs.h.
//
// Integration: one workgroup per brick of 16 x 4 x 4 voxels, one lane per voxel (a wave reads four 64-byte rows of S and of Wt).  The
// lane keeps its voxel's S, Wt and colour sums in registers over the up to DMVS_TSDF_VIEW_CHUNK views of a launch, which arrive as a
// KERNEL ARGUMENT (12 doubles each, scalar loads), so the volume is read and written once per eight views; the depth maps are gathered
// (neighbouring voxels project to neighbouring pixels).  Every voxel has one owner: plain read-modify-write, integer sums, no atomics.
//
// The cull: the first 8 * nv lanes project the brick's eight corner voxels into one view each; z and the four edge functions
//   x + 0.5 z,  x - (W - 0.5) z,  y + 0.5 z,  y - (H - 0.5) z
// are affine in the world point, and a voxel's coordinate ox + i h is monotone in i, so over the brick each lies between its corner
// values -- up to rounding.  A (brick, view) pair is skipped only if a corner maximum (minimum) is beyond zero by a MARGIN of 2^-40 times
// the sum of the absolute values of the terms: the rounding of the three multiplies and three adds of a row is below 2^-50 of that sum,
// so every voxel's own x, y, z are then on the same side by more than 2^-41 of it, i.e. z <= 0, or (z > 0) u = x / z is below -0.5 or above
// W - 0.5 by more than a relative 2^-41 (rint(-0.5) = -0 and a tie at W - 0.5 would still be inside: the margin excludes both), likewise v.
// Each of these the per-voxel code skips by itself: the cull changes no bit.  A margin that is not finite never culls.
#include <math.h>

#include "dmvs_common.h"
#include "dmvs_lds_poison.h"

namespace {

#define TSDF_VC DMVS_TSDF_VIEW_CHUNK
#define TSDF_BX 16
#define TSDF_BY 4
#define TSDF_BZ 4
static_assert(TSDF_BX * TSDF_BY * TSDF_BZ == DMVS_BLOCK, "one lane per voxel of the brick");
static_assert(8 * TSDF_VC <= DMVS_BLOCK, "one lane per (view, corner) of the cull");
#define TSDF_MARGIN 9.094947017729282e-13      // 2^-40

struct TsdfViews {
    double p[TSDF_VC][DMVS_TSDF_VIEW_DOUBLES];      // rows 0 and 1 of P = K E[:3], row 2 of E
    int nv;                                         // live views of this launch
};
struct TsdfVolume {
    double ox, oy, oz, h;
    int nx, ny, nz, bricks_x, bricks_y;
};

__global__ void __launch_bounds__(DMVS_BLOCK)
tsdf_integrate_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid, const uint8_t* __restrict__ rgb, TsdfViews vs, TsdfVolume g,
                      int H, int W, double tau, int cull, int* __restrict__ S, int* __restrict__ Wt, uint4* __restrict__ C) {
#pragma clang fp contract(off)
    __shared__ double edge[TSDF_VC][8][5];
    __shared__ int skip[TSDF_VC];
    DMVS_LDS_POISON(edge);
    DMVS_LDS_POISON(skip);
    const int tid = threadIdx.x;
    const unsigned per_slab = (unsigned)g.bricks_x * (unsigned)g.bricks_y;
    const unsigned in_slab = blockIdx.x % per_slab;
    const int i0 = (int)(in_slab % (unsigned)g.bricks_x) * TSDF_BX, j0 = (int)(in_slab / (unsigned)g.bricks_x) * TSDF_BY;
    const int k0 = (int)(blockIdx.x / per_slab) * TSDF_BZ;
    const double Wm = (double)W - 0.5, Hm = (double)H - 0.5;

    if (cull) {
        const int i1 = min(i0 + TSDF_BX, g.nx) - 1, j1 = min(j0 + TSDF_BY, g.ny) - 1, k1 = min(k0 + TSDF_BZ, g.nz) - 1;
        if (tid < 8 * vs.nv) {
            const double* p = vs.p[tid >> 3];
            const double X = g.ox + (double)((tid & 1) ? i1 : i0) * g.h, Y = g.oy + (double)((tid & 2) ? j1 : j0) * g.h;
            const double Z = g.oz + (double)((tid & 4) ? k1 : k0) * g.h;
            const double x = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3], y = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7];
            const double z = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11];
            double* e = edge[tid >> 3][tid & 7];
            e[0] = z, e[1] = x + 0.5 * z, e[2] = x - Wm * z, e[3] = y + 0.5 * z, e[4] = y - Hm * z;
        }
        __syncthreads();
        if (tid < vs.nv) {
            const double* p = vs.p[tid];
            const double Xa = fmax(fabs(g.ox + (double)i0 * g.h), fabs(g.ox + (double)i1 * g.h));
            const double Ya = fmax(fabs(g.oy + (double)j0 * g.h), fabs(g.oy + (double)j1 * g.h));
            const double Za = fmax(fabs(g.oz + (double)k0 * g.h), fabs(g.oz + (double)k1 * g.h));
            const double Mx = ((fabs(p[0]) * Xa + fabs(p[1]) * Ya) + fabs(p[2]) * Za) + fabs(p[3]);
            const double My = ((fabs(p[4]) * Xa + fabs(p[5]) * Ya) + fabs(p[6]) * Za) + fabs(p[7]);
            const double Mz = ((fabs(p[8]) * Xa + fabs(p[9]) * Ya) + fabs(p[10]) * Za) + fabs(p[11]);
            // (+ 1e-300: below the normal range a rounding is an absolute 2^-1075, not a relative 2^-53)
            const double mz = TSDF_MARGIN * Mz + 1e-300, mu = TSDF_MARGIN * (Mx + ((double)W + 1.0) * Mz) + 1e-300;
            const double mv = TSDF_MARGIN * (My + ((double)H + 1.0) * Mz) + 1e-300;
            double zmax = edge[tid][0][0], lmax = edge[tid][0][1], rmin = edge[tid][0][2], tmax = edge[tid][0][3], bmin = edge[tid][0][4];
            for (int c = 1; c < 8; ++c) {
                const double* e = edge[tid][c];
                zmax = fmax(zmax, e[0]), lmax = fmax(lmax, e[1]), rmin = fmin(rmin, e[2]), tmax = fmax(tmax, e[3]), bmin = fmin(bmin, e[4]);
            }
            // (every comparison is false for a NaN or an infinite margin: no cull)
            skip[tid] = (zmax < -mz) || (lmax < -mu) || (rmin > mu) || (tmax < -mv) || (bmin > mv);
        }
        __syncthreads();
    }

    const int li = tid % TSDF_BX, lj = (tid / TSDF_BX) % TSDF_BY, lk = tid / (TSDF_BX * TSDF_BY);
    const int i = i0 + li, j = j0 + lj, k = k0 + lk;
    if (i >= g.nx || j >= g.ny || k >= g.nz) return;
    const long vox = ((long)k * g.ny + j) * g.nx + i;                // (< 2^31)
    const double X = g.ox + (double)i * g.h, Y = g.oy + (double)j * g.h, Z = g.oz + (double)k * g.h;
    const long HW = (long)H * W;
    int s = S[vox], wt = Wt[vox];
    uint4 col;                                                       // what this launch adds to C
    col.x = col.y = col.z = col.w = 0u;
    const double Wl = (double)(W - 1), Hl = (double)(H - 1);
    for (int v = 0; v < vs.nv; ++v) {
        if (cull && skip[v]) continue;
        const double* p = vs.p[v];
        const double z = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11];
        if (!(z > 0.0)) continue;
        const double x = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3], y = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7];
        const double u = x / z, w = y / z;
        if (!isfinite(u) || !isfinite(w)) continue;
        const double pu = rint(u), pv = rint(w);
        if (!(pu >= 0.0 && pu <= Wl && pv >= 0.0 && pv <= Hl)) continue;
        const long pix = (long)v * HW + (long)(int)pv * W + (int)pu;
        if (valid && valid[pix] == 0) continue;
        const float df = depth[pix];
        const double d = (double)df;
        if (!(isfinite(df) && d > 0.0)) continue;
        const double sdf = d - z;
        if (sdf < -tau) continue;
        s += (int)rint(fmin(sdf / tau, 1.0) * 16384.0);
        wt += 1;
        if (rgb && sdf <= tau) {
            const uint8_t* c = rgb + 3 * pix;
            col.x += c[0], col.y += c[1], col.z += c[2], col.w += 1u;
        }
    }
    S[vox] = s, Wt[vox] = wt;
    if (C && col.w) {
        uint4 a = C[vox];
        a.x += col.x, a.y += col.y, a.z += col.z, a.w += col.w;
        C[vox] = a;
    }
}

// ----------------------------------------------------------------------------------------------------------------- surface nets
__device__ __forceinline__ int tsdf_corner(int c, int nx, long nxy) { return (c & 1) + ((c >> 1) & 1) * nx + (int)((c >> 2) * nxy); }

// cell[v] = 1 iff v = (i, j, k) is a cell of the (nx-1)(ny-1)(nz-1) grid whose 8 corners are observed and not all of one sign
__global__ void __launch_bounds__(DMVS_BLOCK)
tsdf_cell_kernel(const int* __restrict__ S, const int* __restrict__ Wt, int nx, int ny, int nz, int min_weight, uint8_t* __restrict__ cell) {
    const long n = (long)nx * ny * nz, nxy = (long)nx * ny;
    const long v = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (v >= n) return;
    const int i = (int)(v % nx), j = (int)(v / nx % ny), k = (int)(v / nxy);
    uint8_t f = 0;
    if (i < nx - 1 && j < ny - 1 && k < nz - 1) {
        int observed = 1, inside = 0;
        for (int c = 0; c < 8; ++c) {
            const long q = v + tsdf_corner(c, nx, nxy);
            observed &= Wt[q] >= min_weight;
            inside += S[q] < 0;
        }
        f = observed && inside != 0 && inside != 8;       // (signs differ somewhere <=> they differ along one of the 12 edges: the cube's edge graph is connected)
    }
    cell[v] = f;
}

// quad[v]: bit a set iff the edge from voxel v to its +a neighbour crosses (both observed, signs differ) and its four cells have a vertex
__global__ void __launch_bounds__(DMVS_BLOCK)
tsdf_quad_kernel(const int* __restrict__ S, const int* __restrict__ Wt, int nx, int ny, int nz, int min_weight, const uint8_t* __restrict__ cell,
                 uint8_t* __restrict__ quad) {
    const long n = (long)nx * ny * nz, nxy = (long)nx * ny;
    const long v = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (v >= n) return;
    const int pos[3] = {(int)(v % nx), (int)(v / nx % ny), (int)(v / nxy)};
    const int dims[3] = {nx, ny, nz};
    const long step[3] = {1, nx, nxy};
    uint8_t f = 0;
    if (Wt[v] >= min_weight) {
        const int in0 = S[v] < 0;
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            if (pos[a] + 1 >= dims[a]) continue;
            const long q = v + step[a];
            if (!(Wt[q] >= min_weight) || (S[q] < 0) == in0) continue;
            // the cells at (b, c) offsets -1 / 0; along a the cell index is the voxel's, < dims[a] - 1 as the neighbour exists
            if (pos[b] < 1 || pos[b] >= dims[b] - 1 || pos[c] < 1 || pos[c] >= dims[c] - 1) continue;
            if (cell[v - step[b] - step[c]] && cell[v - step[c]] && cell[v] && cell[v - step[b]]) f |= (uint8_t)(1 << a);
        }
    }
    quad[v] = f;
}

__global__ void __launch_bounds__(DMVS_BLOCK)
tsdf_vertices_kernel(const int* __restrict__ S, const int* __restrict__ Wt, const uint4* __restrict__ C, TsdfVolume g, const uint8_t* __restrict__ cell,
                     const int* __restrict__ cell_cum, float* __restrict__ verts, uint8_t* __restrict__ rgb) {
#pragma clang fp contract(off)
    const long n = (long)g.nx * g.ny * g.nz, nxy = (long)g.nx * g.ny;
    const long v = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (v >= n || !cell[v]) return;
    double f[8];
    int in[8];
    unsigned long long cr = 0, cg = 0, cb = 0, cn = 0;
    for (int c = 0; c < 8; ++c) {
        const long q = v + tsdf_corner(c, g.nx, nxy);
        const int s = S[q];
        f[c] = (double)s / (double)Wt[q];
        in[c] = s < 0;
        if (C) {
            const uint4 a = C[q];
            cr += a.x, cg += a.y, cb += a.z, cn += a.w;
        }
    }
    double ax = 0.0, ay = 0.0, az = 0.0;
    int m = 0;
    // the 12 edges (a, b), a < b, one bit apart, in lexicographic order: for a = 0 .. 7 the clear bits of a, lowest first
#pragma unroll
    for (int a = 0; a < 8; ++a) {
#pragma unroll
        for (int bit = 0; bit < 3; ++bit) {
            if (a & (1 << bit)) continue;
            const int b = a | (1 << bit);
            if (in[a] == in[b]) continue;
            const double t = f[a] / (f[a] - f[b]);
            ax += bit == 0 ? t : (double)(a & 1);
            ay += bit == 1 ? t : (double)((a >> 1) & 1);
            az += bit == 2 ? t : (double)((a >> 2) & 1);
            m += 1;
        }
    }
    const int i = (int)(v % g.nx), j = (int)(v / g.nx % g.ny), k = (int)(v / nxy);
    const double md = (double)m;
    const long o = (long)cell_cum[v] - 1;                            // vertices are numbered in ascending cell index
    verts[3 * o + 0] = (float)(g.ox + ((double)i + ax / md) * g.h);
    verts[3 * o + 1] = (float)(g.oy + ((double)j + ay / md) * g.h);
    verts[3 * o + 2] = (float)(g.oz + ((double)k + az / md) * g.h);
    uint8_t r8 = 0, g8 = 0, b8 = 0;
    if (cn > 0) r8 = (uint8_t)((2 * cr + cn) / (2 * cn)), g8 = (uint8_t)((2 * cg + cn) / (2 * cn)), b8 = (uint8_t)((2 * cb + cn) / (2 * cn));
    rgb[3 * o + 0] = r8, rgb[3 * o + 1] = g8, rgb[3 * o + 2] = b8;
}

__global__ void __launch_bounds__(DMVS_BLOCK)
tsdf_faces_kernel(const int* __restrict__ S, int nx, int ny, int nz, const uint8_t* __restrict__ quad, const int* __restrict__ quad_cum,
                  const int* __restrict__ cell_cum, int* __restrict__ faces) {
    const long n = (long)nx * ny * nz, nxy = (long)nx * ny;
    const long v = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (v >= n) return;
    const int f = quad[v];
    if (!f) return;
    const long step[3] = {1, nx, nxy};
    const int inside = S[v] < 0;
    long o = (long)quad_cum[v] - ((f & 1) + ((f >> 1) & 1) + ((f >> 2) & 1));      // quads in front of this voxel's
    for (int a = 0; a < 3; ++a) {
        if (!(f & (1 << a))) continue;
        const long sb = step[(a + 1) % 3], sc = step[(a + 2) % 3];
        const int q0 = cell_cum[v - sb - sc] - 1, q1 = cell_cum[v - sc] - 1, q2 = cell_cum[v] - 1, q3 = cell_cum[v - sb] - 1;
        int* t = faces + 6 * o;
        if (inside) t[0] = q0, t[1] = q1, t[2] = q2, t[3] = q0, t[4] = q2, t[5] = q3;
        else t[0] = q3, t[1] = q2, t[2] = q1, t[3] = q3, t[4] = q1, t[5] = q0;
        o += 1;
    }
}

// the checks every entry point shares -> 0, or DMVS_EINVAL; *n = the number of voxels
inline int tsdf_volume_args(int32_t nx, int32_t ny, int32_t nz, const double* origin, double h, TsdfVolume* g, int64_t* n) {
    if (nx < 0 || ny < 0 || nz < 0) return DMVS_EINVAL;
    *n = (int64_t)nx * ny;
    if (*n > 2147483647L) return DMVS_EINVAL;
    *n *= nz;
    if (*n > 2147483647L) return DMVS_EINVAL;
    if (origin) {
        if (!isfinite(origin[0]) || !isfinite(origin[1]) || !isfinite(origin[2]) || !(h > 0.0) || !isfinite(h)) return DMVS_EINVAL;
        g->ox = origin[0], g->oy = origin[1], g->oz = origin[2], g->h = h;
    }
    g->nx = nx, g->ny = ny, g->nz = nz;
    g->bricks_x = (int)dmvs_ceil_div(nx, TSDF_BX), g->bricks_y = (int)dmvs_ceil_div(ny, TSDF_BY);
    return 0;
}

}  // namespace

extern "C" int dmvs_tsdf_integrate_f32(const float* depth, const uint8_t* valid, const uint8_t* rgb, const double* views, int64_t V, int32_t H, int32_t W,
                                       int32_t nx, int32_t ny, int32_t nz, const double* origin, double h, double tau, int32_t flags, int32_t* S,
                                       int32_t* Wt, uint32_t* C, void* stream) {
    TsdfVolume g;
    int64_t n = 0;
    if (!origin || tsdf_volume_args(nx, ny, nz, origin, h, &g, &n) != 0) return DMVS_EINVAL;
    if (V < 0 || V > DMVS_TSDF_MAX_VIEWS || H < 0 || W < 0) return DMVS_EINVAL;
    const int64_t HW = (int64_t)H * W;
    if (HW > 2147483647L) return DMVS_EINVAL;                        // (V <= 65535: the maps are indexed in 47 bits)
    if (!(tau > 0.0) || !isfinite(tau)) return DMVS_EINVAL;
    if (flags & ~DMVS_TSDF_NO_CULL) return DMVS_EINVAL;
    if (((uintptr_t)depth & 3u) || ((uintptr_t)S & 3u) || ((uintptr_t)Wt & 3u) || ((uintptr_t)C & 15u)) return DMVS_EINVAL;
    if (rgb && !C) return DMVS_EINVAL;
    const bool work = V > 0 && HW > 0 && n > 0;
    if (work && (!depth || !views || !S || !Wt)) return DMVS_EINVAL;
    if (views)
        for (int64_t k = 0; k < V * DMVS_TSDF_VIEW_DOUBLES; ++k)
            if (!isfinite(views[k])) return DMVS_EINVAL;
    if (!work) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((long)g.bricks_x * g.bricks_y * dmvs_ceil_div(nz, TSDF_BZ)));      // (< 2^31 / 16 + the ragged edges)
    for (int64_t v0 = 0; v0 < V; v0 += TSDF_VC) {
        TsdfViews vs;
        vs.nv = (int)(V - v0 < TSDF_VC ? V - v0 : TSDF_VC);
        for (int k = 0; k < TSDF_VC; ++k) {
            const double* q = views + (v0 + (k < vs.nv ? k : 0)) * DMVS_TSDF_VIEW_DOUBLES;      // (unused slots repeat the first: never read)
            for (int j = 0; j < DMVS_TSDF_VIEW_DOUBLES; ++j) vs.p[k][j] = q[j];
        }
        hipLaunchKernelGGL(tsdf_integrate_kernel, grid, dim3(DMVS_BLOCK), 0, s, depth + v0 * HW, valid ? valid + v0 * HW : nullptr,
                           rgb ? rgb + 3 * v0 * HW : nullptr, vs, g, (int)H, (int)W, tau, (flags & DMVS_TSDF_NO_CULL) ? 0 : 1, S, Wt,
                           reinterpret_cast<uint4*>(C));
        const int rc = dmvs_launch_status();
        if (rc != 0) return rc;
    }
    return 0;
}

extern "C" int dmvs_tsdf_flags_u8(const int32_t* S, const int32_t* Wt, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight, uint8_t* cell, uint8_t* quad,
                                  void* stream) {
    TsdfVolume g;
    int64_t n = 0;
    if (tsdf_volume_args(nx, ny, nz, nullptr, 0.0, &g, &n) != 0 || min_weight < 1) return DMVS_EINVAL;
    if (((uintptr_t)S & 3u) || ((uintptr_t)Wt & 3u)) return DMVS_EINVAL;
    if (n == 0) return 0;
    if (!S || !Wt || !cell || !quad) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(dmvs_ceil_div(n, DMVS_BLOCK));
    hipLaunchKernelGGL(tsdf_cell_kernel, grid, dim3(DMVS_BLOCK), 0, s, S, Wt, (int)nx, (int)ny, (int)nz, (int)min_weight, cell);
    int rc = dmvs_launch_status();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(tsdf_quad_kernel, grid, dim3(DMVS_BLOCK), 0, s, S, Wt, (int)nx, (int)ny, (int)nz, (int)min_weight, cell, quad);
    return dmvs_launch_status();
}

extern "C" int dmvs_tsdf_vertices_f32(const int32_t* S, const int32_t* Wt, const uint32_t* C, int32_t nx, int32_t ny, int32_t nz, const double* origin, double h,
                                      const uint8_t* cell, const int32_t* cell_cum, int64_t N, float* verts, uint8_t* rgb, void* stream) {
    TsdfVolume g;
    int64_t n = 0;
    if (!origin || tsdf_volume_args(nx, ny, nz, origin, h, &g, &n) != 0) return DMVS_EINVAL;
    if (N < 0 || N > n) return DMVS_EINVAL;
    if (((uintptr_t)S & 3u) || ((uintptr_t)Wt & 3u) || ((uintptr_t)C & 15u) || ((uintptr_t)cell_cum & 3u) || ((uintptr_t)verts & 3u)) return DMVS_EINVAL;
    if (n == 0 || N == 0) return 0;
    if (!S || !Wt || !cell || !cell_cum || !verts || !rgb) return DMVS_EINVAL;
    hipLaunchKernelGGL(tsdf_vertices_kernel, dim3(dmvs_ceil_div(n, DMVS_BLOCK)), dim3(DMVS_BLOCK), 0, (hipStream_t)stream, S, Wt,
                       reinterpret_cast<const uint4*>(C), g, cell, cell_cum, verts, rgb);
    return dmvs_launch_status();
}

extern "C" int dmvs_tsdf_faces_i32(const int32_t* S, int32_t nx, int32_t ny, int32_t nz, const uint8_t* quad, const int32_t* quad_cum, const int32_t* cell_cum,
                                   int64_t Q, int32_t* faces, void* stream) {
    TsdfVolume g;
    int64_t n = 0;
    if (tsdf_volume_args(nx, ny, nz, nullptr, 0.0, &g, &n) != 0) return DMVS_EINVAL;
    if (Q < 0 || Q > 3 * n || Q > DMVS_TSDF_MAX_QUADS) return DMVS_EINVAL;
    if (((uintptr_t)S & 3u) || ((uintptr_t)quad_cum & 3u) || ((uintptr_t)cell_cum & 3u) || ((uintptr_t)faces & 3u)) return DMVS_EINVAL;
    if (n == 0 || Q == 0) return 0;
    if (!S || !quad || !quad_cum || !cell_cum || !faces) return DMVS_EINVAL;
    hipLaunchKernelGGL(tsdf_faces_kernel, dim3(dmvs_ceil_div(n, DMVS_BLOCK)), dim3(DMVS_BLOCK), 0, (hipStream_t)stream, S, (int)nx, (int)ny, (int)nz, quad,
                       quad_cum, cell_cum, faces);
    return dmvs_launch_status();
}
