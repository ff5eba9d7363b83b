// Triangle meshes into the views (diffmvs_amd/mesh_render.py): dmvs_mesh_raster_fill_u64, dmvs_mesh_raster_zid_u64 and
// dmvs_mesh_raster_resolve_f32.  The contract (projection, snapping, the slots, coverage and its tie rule, the depth) is in include/dmvs.h.
//
// One lane per face, grid-stride; a launch carries up to DMVS_SPLAT_VIEW_CHUNK views as a kernel argument, as the splat does, so a face's
// three vertices are read once per chunk.  Per (face, view) raster_setup projects the three vertices in fp64 and snaps them to 1/256 pixel;
// from there coverage is integer arithmetic (edge values below 2^59) and does not depend on who evaluates it.  The lane then walks the
// clipped box itself when it holds at most DMVS_RASTER_SMALL pixels -- a mesh extracted at the resolution of its views has boxes of 1 to 3
// pixels -- and otherwise appends (face, view) to the caller's queue, which raster_wave_kernel drains after it: one wave per entry, the
// setup redone (wave-uniform), the box in 8 x 8 tiles with one lane per pixel.  A whole-image triangle costs H W / 64 trips instead of
// H W in one lane beside 63 idle ones.  With the queue full the lane walks the large box itself (work[2]).
// A covered pixel takes ONE u64 integer atomic-min of (bits of the fp32 depth << 32 | face) behind a plain load: the minimum only ever
// falls, so a stale value is an upper bound and the skip cannot change the result.  Integer min, integer adds: zid and counts are bitwise
// independent of the grid, of the queue and of the order of the faces.
// The resolve pass reads the finished zid, one lane per pixel with the view as blockIdx.y (wave-uniform view arguments): depth and face are
// the two words; the normal and the colour redo the setup of the winning face.
#include <float.h>

#include "cloud_walk.h"      // CloudTransform / cloud_move, CloudSums / cloud_block_sum, dmvs_atomic_min_u64 / dmvs_peek_u64

namespace {

#define RASTER_VC DMVS_SPLAT_VIEW_CHUNK
#define RASTER_EMPTY 0xffffffffffffffffull

struct RasterView { double p0[4], p1[4], e[12], near, far; };        // = DMVS_RASTER_VIEW_DOUBLES doubles, the layout of `views`
struct RasterViews {
    RasterView v[RASTER_VC];
    int nv;                                                          // live views of this launch
};
struct RasterMesh {
    const float* verts;
    const int32_t* faces;
    long N, F;
    CloudTransform T;
};
struct RasterFace {                                                  // one (face, view) after step 8, vertices 1 and 2 swapped where A was negative
    long sx[3], sy[3], A;
    double z[3];
    int id[3];                                                       // vertex indices in the same order
    int c0, c1, r0, r1;
};

__device__ __forceinline__ long raster_min(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long raster_max(long a, long b) { return a > b ? a : b; }

__device__ __forceinline__ bool raster_vertex(const RasterMesh& m, int i, double& X, double& Y, double& Z) {
    if (i < 0 || (long)i >= m.N) return false;
    float fx = m.verts[3 * (long)i], fy = m.verts[3 * (long)i + 1], fz = m.verts[3 * (long)i + 2];
    cloud_move(m.T, fx, fy, fz);
    X = fx, Y = fy, Z = fz;
    return isfinite(fx) && isfinite(fy) && isfinite(fz);
}

// steps 1 to 8 of the contract: the slot that counts the (face, view); DMVS_RASTER_SLOTS - 1 = drawn, and `ft` is then complete
__device__ __forceinline__ int raster_setup(const RasterMesh& m, long f, const RasterView& vw, int flags, int H, int W, RasterFace& ft) {
#pragma clang fp contract(off)
    double u[3], v[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        double X = 0.0, Y = 0.0, Z = 0.0;
        ft.id[k] = m.faces[3 * f + k];
        ok = raster_vertex(m, ft.id[k], X, Y, Z) && ok;
        const double x = ((vw.p0[0] * X + vw.p0[1] * Y) + vw.p0[2] * Z) + vw.p0[3];
        const double y = ((vw.p1[0] * X + vw.p1[1] * Y) + vw.p1[2] * Z) + vw.p1[3];
        ft.z[k] = ((vw.e[8] * X + vw.e[9] * Y) + vw.e[10] * Z) + vw.e[11];
        u[k] = x / ft.z[k], v[k] = y / ft.z[k];
    }
    if (!ok) return 0;
    if (ft.z[0] <= vw.near || ft.z[1] <= vw.near || ft.z[2] <= vw.near) return 1;
    if (ft.z[0] > vw.far && ft.z[1] > vw.far && ft.z[2] > vw.far) return 2;
    for (int k = 0; k < 3; ++k)
        if (!(fabs(u[k]) <= 1048576.0 && fabs(v[k]) <= 1048576.0)) return 3;      // (false for NaN)
    for (int k = 0; k < 3; ++k) ft.sx[k] = llrint(u[k] * 256.0), ft.sy[k] = llrint(v[k] * 256.0);
    ft.A = (ft.sx[1] - ft.sx[0]) * (ft.sy[2] - ft.sy[0]) - (ft.sy[1] - ft.sy[0]) * (ft.sx[2] - ft.sx[0]);
    if (ft.A == 0) return 4;
    if (((flags & DMVS_RASTER_CULL_NEG) && ft.A < 0) || ((flags & DMVS_RASTER_CULL_POS) && ft.A > 0)) return 5;
    if (ft.A < 0) {
        const long tx = ft.sx[1], ty = ft.sy[1];
        const double tz = ft.z[1];
        const int ti = ft.id[1];
        ft.sx[1] = ft.sx[2], ft.sy[1] = ft.sy[2], ft.z[1] = ft.z[2], ft.id[1] = ft.id[2];
        ft.sx[2] = tx, ft.sy[2] = ty, ft.z[2] = tz, ft.id[2] = ti;
        ft.A = -ft.A;
    }
    const long x0 = raster_min(ft.sx[0], raster_min(ft.sx[1], ft.sx[2])), x1 = raster_max(ft.sx[0], raster_max(ft.sx[1], ft.sx[2]));
    const long y0 = raster_min(ft.sy[0], raster_min(ft.sy[1], ft.sy[2])), y1 = raster_max(ft.sy[0], raster_max(ft.sy[1], ft.sy[2]));
    const long c0 = raster_max((x0 + 255) >> 8, 0L), c1 = raster_min(x1 >> 8, (long)W - 1);      // ceil(min / 256) .. floor(max / 256), clipped
    const long r0 = raster_max((y0 + 255) >> 8, 0L), r1 = raster_min(y1 >> 8, (long)H - 1);
    if (c0 > c1 || r0 > r1) return 6;
    ft.c0 = (int)c0, ft.c1 = (int)c1, ft.r0 = (int)r0, ft.r1 = (int)r1;
    return 7;
}

// step 9: the three edge values of a pixel; true iff it is covered
__device__ __forceinline__ bool raster_edges(const RasterFace& ft, int px, int py, long e[3]) {
    bool in = true;
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const long dx = ft.sx[b] - ft.sx[a], dy = ft.sy[b] - ft.sy[a];
        e[k] = dx * (256L * py - ft.sy[a]) - dy * (256L * px - ft.sx[a]);
        in = in && (e[k] > 0 || (e[k] == 0 && (dy > 0 || (dy == 0 && dx > 0))));
    }
    return in;
}

// step 10: the weights and the depth of a covered pixel
__device__ __forceinline__ double raster_depth(const RasterFace& ft, const long e[3], double wq[3]) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) wq[k] = ((double)e[k] / (double)ft.A) * (1.0 / ft.z[k]);
    return 1.0 / ((wq[0] + wq[1]) + wq[2]);
}

struct RasterWork { unsigned long long covered, issued; };

__device__ __forceinline__ void raster_pixel(const RasterFace& ft, unsigned face, double far, int px, int py, unsigned long long* zrow,
                                             RasterWork& wk) {
    long e[3];
    if (!raster_edges(ft, px, py, e)) return;
    ++wk.covered;
    double wq[3];
    const double zp = raster_depth(ft, e, wq);
    if (!(zp <= far)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)zp) << 32) | face;
    if (!(key < dmvs_peek_u64(zrow + px))) return;
    ++wk.issued;
    dmvs_atomic_min_u64(zrow + px, key);
}

__global__ void __launch_bounds__(DMVS_BLOCK)
raster_lane_kernel(RasterMesh m, RasterViews vs, int flags, int H, int W, unsigned long long* zid, unsigned long long* __restrict__ counts,
                   unsigned long long* __restrict__ work, unsigned long long* __restrict__ queue, long queue_cap) {
    // per-view counters of this workgroup (F < 2^31).  Only faces that are NOT drawn touch them: the last slot of a view is what is
    // left of the workgroup's faces (`mine`, summed in the extra entry)
    __shared__ int slots[RASTER_VC * DMVS_RASTER_SLOTS + 1];
    if (threadIdx.x <= RASTER_VC * DMVS_RASTER_SLOTS) slots[threadIdx.x] = 0;
    __syncthreads();
    int mine = 0;
    RasterWork wk = {0, 0};
    unsigned long long fell = 0;
    const long HW = (long)H * W;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    for (long f = tid; f < m.F; f += stride) {
        ++mine;
        for (int k = 0; k < vs.nv; ++k) {                            // (wave-uniform: the view's doubles are scalar loads)
            RasterFace ft;
            const int slot = raster_setup(m, f, vs.v[k], flags, H, W, ft);
            if (slot != DMVS_RASTER_SLOTS - 1) {
                atomicAdd(&slots[k * DMVS_RASTER_SLOTS + slot], 1);
                continue;
            }
            if ((long)(ft.c1 - ft.c0 + 1) * (ft.r1 - ft.r0 + 1) > DMVS_RASTER_SMALL) {
                if (queue_cap > 0) {
                    const unsigned long long at = atomicAdd(queue, 1ull);      // queue[0]: entries asked for (may pass the capacity)
                    if (at < (unsigned long long)queue_cap) {
                        queue[1 + at] = ((unsigned long long)k << 32) | (unsigned long long)f;
                        continue;
                    }
                }
                ++fell;
            }
            for (int row = ft.r0; row <= ft.r1; ++row)
                for (int col = ft.c0; col <= ft.c1; ++col) raster_pixel(ft, (unsigned)f, vs.v[k].far, col, row, zid + k * HW + (long)row * W, wk);
        }
    }
    if (mine) atomicAdd(&slots[RASTER_VC * DMVS_RASTER_SLOTS], mine);
    __syncthreads();
    if ((int)threadIdx.x < vs.nv * DMVS_RASTER_SLOTS) {
        int c = slots[threadIdx.x];
        if (threadIdx.x % DMVS_RASTER_SLOTS == DMVS_RASTER_SLOTS - 1) {
            c = slots[RASTER_VC * DMVS_RASTER_SLOTS];
            for (int j = 1; j < DMVS_RASTER_SLOTS; ++j) c -= slots[threadIdx.x - j];
        }
        if (c) atomicAdd(counts + threadIdx.x, (unsigned long long)c);
    }
    if (work) {
        CloudSums<3> w;
        w.v[0] = wk.covered, w.v[1] = wk.issued, w.v[2] = fell;
        cloud_block_sum(w, 3, work);
    }
}

// the queue of the launch above: one wave per entry, lanes over 8 x 8 pixel tiles of the box
__global__ void __launch_bounds__(DMVS_BLOCK)
raster_wave_kernel(RasterMesh m, RasterViews vs, int flags, int H, int W, unsigned long long* zid, unsigned long long* __restrict__ work,
                   const unsigned long long* __restrict__ queue, long queue_cap) {
    RasterWork wk = {0, 0};
    const long HW = (long)H * W;
    const unsigned long long asked = queue[0];
    const long n = asked < (unsigned long long)queue_cap ? (long)asked : queue_cap;
    const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    const long wave = (long)blockIdx.x * (DMVS_BLOCK / 64) + (threadIdx.x >> 6), waves = (long)gridDim.x * (DMVS_BLOCK / 64);
    for (long q = wave; q < n; q += waves) {
        const unsigned long long ent = queue[1 + q];
        const int k = (int)(ent >> 32);
        const long f = (long)(ent & 0xffffffffull);
        if (k >= vs.nv || f >= m.F) continue;                        // (never: the entries are this launch's own)
        RasterFace ft;
        if (raster_setup(m, f, vs.v[k], flags, H, W, ft) != DMVS_RASTER_SLOTS - 1) continue;
        const int tx = (ft.c1 - ft.c0 + 8) >> 3, ty = (ft.r1 - ft.r0 + 8) >> 3;
        for (long t = 0; t < (long)tx * ty; ++t) {
            const int col = ft.c0 + (int)(t % tx) * 8 + lx, row = ft.r0 + (int)(t / tx) * 8 + ly;
            if (col <= ft.c1 && row <= ft.r1) raster_pixel(ft, (unsigned)f, vs.v[k].far, col, row, zid + k * HW + (long)row * W, wk);
        }
    }
    if (work) {
        CloudSums<2> w;
        w.v[0] = wk.covered, w.v[1] = wk.issued;
        cloud_block_sum(w, 2, work);
    }
}

template <bool NORMAL, bool RGB>
__global__ void __launch_bounds__(DMVS_BLOCK)
raster_resolve_kernel(RasterMesh m, RasterViews vs, int H, int W, const unsigned long long* __restrict__ zid, const uint8_t* __restrict__ vrgb,
                      float* __restrict__ depth, int32_t* __restrict__ face, float* __restrict__ normal, uint8_t* __restrict__ rgb) {
#pragma clang fp contract(off)
    const long HW = (long)H * W;
    const int k = blockIdx.y;
    const long p = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x;
    if (p >= HW) return;
    const long at = k * HW + p;
    const unsigned long long key = zid[at];
    const bool hit = key != RASTER_EMPTY && (long)(key & 0xffffffffull) < m.F;
    const long f = (long)(key & 0xffffffffull);
    depth[at] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    face[at] = hit ? (int32_t)f : -1;
    const RasterView& vw = vs.v[k];
    if (NORMAL) {
        double n[3] = {0.0, 0.0, 0.0};
        double P[3][3];
        bool ok = hit;
        for (int j = 0; j < 3 && ok; ++j) ok = raster_vertex(m, m.faces[3 * f + j], P[j][0], P[j][1], P[j][2]);
        if (ok) {
            const double ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
            const double bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const double len = sqrt((cx * cx + cy * cy) + cz * cz);
            if (len > 0.0 && isfinite(len)) {
                n[0] = cx / len, n[1] = cy / len, n[2] = cz / len;
                double d[3];
                for (int i = 0; i < 3; ++i) {
                    const double* e = vw.e + 4 * i;
                    const double nc = (e[0] * n[0] + e[1] * n[1]) + e[2] * n[2];
                    const double pc = ((e[0] * P[0][0] + e[1] * P[0][1]) + e[2] * P[0][2]) + e[3];
                    d[i] = nc * pc;
                }
                if ((d[0] + d[1]) + d[2] > 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
            }
        }
        for (int i = 0; i < 3; ++i) normal[3 * at + i] = (float)n[i];
    }
    if (RGB) {
        int c[3] = {0, 0, 0};
        RasterFace ft;
        long e[3];
        if (hit && raster_setup(m, f, vw, 0, H, W, ft) == DMVS_RASTER_SLOTS - 1 && raster_edges(ft, (int)(p % W), (int)(p / W), e)) {
            double wq[3];
            const double zp = raster_depth(ft, e, wq);
            for (int i = 0; i < 3; ++i) {
                const double b0 = wq[0] * zp, b1 = wq[1] * zp, b2 = wq[2] * zp;
                const double v = rint((b0 * (double)vrgb[3 * (long)ft.id[0] + i] + b1 * (double)vrgb[3 * (long)ft.id[1] + i])
                                      + b2 * (double)vrgb[3 * (long)ft.id[2] + i]);
                c[i] = (int)fmin(fmax(v, 0.0), 255.0);
            }
        }
        for (int i = 0; i < 3; ++i) rgb[3 * at + i] = (uint8_t)c[i];
    }
}

// what both entry points check before anything is touched; 0 or DMVS_EINVAL
inline int raster_args(const float* verts, int64_t N, const int32_t* faces, int64_t F, const double* transform, const double* views, int64_t V,
                       int32_t H, int32_t W, const void* zid, CloudTransform& T) {
    if (N < 0 || F < 0 || V < 0 || H < 0 || W < 0 || N > 2147483647L || F > 2147483647L) return DMVS_EINVAL;
    const int64_t HW = (int64_t)H * W;
    if (HW > 2147483647L || (HW > 0 && V > (1L << 40) / HW)) return DMVS_EINVAL;      // a plane is indexed in 31 bits, the buffer in 40
    if (((uintptr_t)verts & 3u) || ((uintptr_t)faces & 3u) || ((uintptr_t)zid & 7u)) return DMVS_EINVAL;
    if (cloud_transform_arg(transform, T) != 0) return DMVS_EINVAL;
    if (V > 0 && !views) return DMVS_EINVAL;
    for (int64_t v = 0; v < V; ++v) {
        const double* q = views + v * DMVS_RASTER_VIEW_DOUBLES;
        for (int k = 0; k < DMVS_RASTER_VIEW_DOUBLES; ++k)
            if (!isfinite(q[k])) return DMVS_EINVAL;
        if (!(q[20] > 0.0) || !(q[21] > q[20]) || !(q[21] <= (double)FLT_MAX)) return DMVS_EINVAL;
    }
    if (F > 0 && V > 0 && (!faces || (N > 0 && !verts) || (HW > 0 && !zid))) return DMVS_EINVAL;
    return 0;
}

inline void raster_views(const double* views, int64_t v0, int64_t V, RasterViews& vs) {
    vs.nv = (int)(V - v0 < RASTER_VC ? V - v0 : RASTER_VC);
    for (int k = 0; k < RASTER_VC; ++k) {
        const double* q = views + (v0 + (k < vs.nv ? k : 0)) * DMVS_RASTER_VIEW_DOUBLES;      // (unused slots repeat the first: never read)
        for (int j = 0; j < 4; ++j) vs.v[k].p0[j] = q[j], vs.v[k].p1[j] = q[4 + j];
        for (int j = 0; j < 12; ++j) vs.v[k].e[j] = q[8 + j];
        vs.v[k].near = q[20], vs.v[k].far = q[21];
    }
}

}  // namespace

extern "C" int dmvs_mesh_raster_fill_u64(uint64_t* zid, int64_t n, void* stream) {
    if (n < 0 || n > (1L << 40) || ((uintptr_t)zid & 7u) || (n > 0 && !zid)) return DMVS_EINVAL;
    if (n == 0) return 0;
    const hipError_t err = hipMemsetAsync(zid, 0xff, (size_t)n * sizeof(uint64_t), (hipStream_t)stream);
    return err == hipSuccess ? 0 : (int)err;
}

extern "C" int dmvs_mesh_raster_zid_u64(const float* verts, int64_t N, const int32_t* faces, int64_t F, const double* transform, const double* views,
                                        int64_t V, int32_t H, int32_t W, int32_t flags, int32_t blocks, uint64_t* zid, int64_t* counts,
                                        uint64_t* work, uint64_t* queue, int64_t queue_cap, void* stream) {
    RasterMesh m;
    const int rc = raster_args(verts, N, faces, F, transform, views, V, H, W, zid, m.T);
    if (rc != 0) return rc;
    if (blocks < 0 || (flags & ~(DMVS_RASTER_CULL_NEG | DMVS_RASTER_CULL_POS)) || flags == (DMVS_RASTER_CULL_NEG | DMVS_RASTER_CULL_POS)) return DMVS_EINVAL;
    if (((uintptr_t)counts & 7u) || ((uintptr_t)work & 7u) || ((uintptr_t)queue & 7u)) return DMVS_EINVAL;
    if (queue_cap < 0 || queue_cap > 2147483647L || (queue_cap > 0 && !queue) || (V > 0 && !counts)) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = V > 0 ? hipMemsetAsync(counts, 0, (size_t)V * DMVS_RASTER_SLOTS * sizeof(int64_t), s) : hipSuccess;
    if (err == hipSuccess && work) err = hipMemsetAsync(work, 0, 3 * sizeof(uint64_t), s);
    if (err != hipSuccess) return (int)err;
    if (F == 0 || V == 0) return 0;
    m.verts = verts, m.faces = faces, m.N = (long)N, m.F = (long)F;
    const long HW = (long)H * W;
    dim3 grid(cloud_sum_blocks(F, blocks)), block(DMVS_BLOCK);
    // the wave pass: enough waves to fill the chip, no more than the queue can hold
    const long wb = (queue_cap + DMVS_BLOCK / 64 - 1) / (DMVS_BLOCK / 64), wcap = blocks > 0 ? blocks : 2048;
    dim3 wgrid((unsigned)(wb < wcap ? wb : wcap));
    unsigned long long* wk = reinterpret_cast<unsigned long long*>(work);
    unsigned long long* qu = reinterpret_cast<unsigned long long*>(queue);
    for (int64_t v0 = 0; v0 < V; v0 += RASTER_VC) {
        RasterViews vs;
        raster_views(views, v0, V, vs);
        unsigned long long* zb = reinterpret_cast<unsigned long long*>(zid) + v0 * HW;
        unsigned long long* ct = reinterpret_cast<unsigned long long*>(counts) + v0 * DMVS_RASTER_SLOTS;
        if (queue_cap > 0 && hipMemsetAsync(queue, 0, sizeof(uint64_t), s) != hipSuccess) return dmvs_launch_status();
        hipLaunchKernelGGL(raster_lane_kernel, grid, block, 0, s, m, vs, (int)flags, (int)H, (int)W, zb, ct, wk, qu, (long)queue_cap);
        if (queue_cap > 0) hipLaunchKernelGGL(raster_wave_kernel, wgrid, block, 0, s, m, vs, (int)flags, (int)H, (int)W, zb, wk, qu, (long)queue_cap);
        const int lrc = dmvs_launch_status();
        if (lrc != 0) return lrc;
    }
    return 0;
}

extern "C" int dmvs_mesh_raster_resolve_f32(const uint64_t* zid, const float* verts, int64_t N, const int32_t* faces, int64_t F,
                                            const double* transform, const double* views, int64_t V, int32_t H, int32_t W, const uint8_t* vrgb,
                                            float* depth, int32_t* face, float* normal, uint8_t* rgb, void* stream) {
    RasterMesh m;
    const int rc = raster_args(verts, N, faces, F, transform, views, V, H, W, zid, m.T);
    if (rc != 0) return rc;
    if (((uintptr_t)depth & 3u) || ((uintptr_t)face & 3u) || ((uintptr_t)normal & 3u)) return DMVS_EINVAL;
    if (rgb && !vrgb && N > 0) return DMVS_EINVAL;                  // a colour output needs the vertex colours
    const long HW = (long)H * W;
    if (V > 0 && HW > 0 && (!zid || !depth || !face || (F > 0 && (!faces || (N > 0 && !verts))))) return DMVS_EINVAL;
    if (V == 0 || HW == 0) return 0;
    m.verts = verts, m.faces = faces, m.N = (long)N, m.F = (long)F;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t v0 = 0; v0 < V; v0 += RASTER_VC) {
        RasterViews vs;
        raster_views(views, v0, V, vs);
        dim3 grid(dmvs_ceil_div(HW, DMVS_BLOCK), vs.nv), block(DMVS_BLOCK);
        const unsigned long long* zb = reinterpret_cast<const unsigned long long*>(zid) + v0 * HW;
        float* dp = depth + v0 * HW;
        int32_t* fc = face + v0 * HW;
        float* nm = normal ? normal + 3 * v0 * HW : nullptr;
        uint8_t* cl = rgb ? rgb + 3 * v0 * HW : nullptr;
        if (nm && cl) hipLaunchKernelGGL((raster_resolve_kernel<true, true>), grid, block, 0, s, m, vs, (int)H, (int)W, zb, vrgb, dp, fc, nm, cl);
        else if (nm) hipLaunchKernelGGL((raster_resolve_kernel<true, false>), grid, block, 0, s, m, vs, (int)H, (int)W, zb, vrgb, dp, fc, nm, cl);
        else if (cl) hipLaunchKernelGGL((raster_resolve_kernel<false, true>), grid, block, 0, s, m, vs, (int)H, (int)W, zb, vrgb, dp, fc, nm, cl);
        else hipLaunchKernelGGL((raster_resolve_kernel<false, false>), grid, block, 0, s, m, vs, (int)H, (int)W, zb, vrgb, dp, fc, nm, cl);
        const int lrc = dmvs_launch_status();
        if (lrc != 0) return lrc;
    }
    return 0;
}
