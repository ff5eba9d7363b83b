// Cleaning and scoring an extracted mesh (diffmvs_amd/mesh_clean.py, diffmvs_amd/mesh_eval.py): dmvs_mesh_label_round_i32,
// dmvs_mesh_face_tally_i64 and dmvs_mesh_sample_f32.  The contract (the hook and shortcut rules, the area and sampling arithmetic) is in
// include/dmvs.h.
//
// Labelling.  label[] is a forest of pointers to smaller vertex indices of the same component.  A round hooks every face (the smallest
// grandparent of its three vertices is pushed into their parents and into them) and then shortcuts every vertex to its grandparent, so
// path lengths halve per round instead of shrinking by one.  Every write is a u32 atomic-min behind a plain load: labels only fall, every
// value is a vertex of the same component, and a stale load can only be too high -- it costs a spurious atomic or one more round, never a
// wrong label.  Nothing here waits for another workgroup; the only cross-launch fact used is that a launch sees what earlier launches
// wrote.  The caller repeats rounds until one issues no atomic: that fixpoint is unique (the smallest index of the component).
//
// Tally.  A big component sends every face to the same two counters, and atomics on one address are served one after the other.  The wave
// sums, with shuffles, the lanes that share its smallest root, then those of the next one, up to TALLY_ROOTS times (surface-nets faces are
// numbered in voxel order: a wave is mostly one component with a few floaters' faces in between).  The largest lot stays in registers
// across the grid-stride passes, smaller ones go out as one pair of atomics each, and the waves of a workgroup meet in LDS at the end: one
// pair of atomics per workgroup for the big component.  Lanes whose root is not among the first TALLY_ROOTS issue their own.  Integer adds either way: the sums are the same bits.  Compiled with -DDMVS_MESH_TALLY_PLAIN
// the combine is off (tools/mesh_clean_bench.py builds that variant beside the product and measures both).
//
// Sampling.  One lane per sample: a binary search in the running area sums, two exact R2 coordinates, one fp64 affine combination.
#include "cloud_walk.h"      // dmvs_atomic_min_u32 / dmvs_peek_u32, cloud_pow2, cloud_sum_blocks

namespace {

// ------------------------------------------------------------------------------------------ labelling
// lowers *p to m when the (possibly stale) value there is larger; 1 if an atomic was issued
__device__ __forceinline__ int label_lower(unsigned* p, unsigned m) {
    if (!(dmvs_peek_u32(p) > m)) return 0;
    dmvs_atomic_min_u32(p, m);
    return 1;
}

// the workgroup's count into *out: waves reduce with shuffles, the workgroup through LDS, one atomic.  A workgroup adds at most `most`, so
// that the total of a launch stays below 2^31 (dmvs.h)
__device__ __forceinline__ void label_block_count(int c, int most, int* out) {
    __shared__ int part[DMVS_BLOCK / 64];
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_down(c, off);
        c = c > most - o ? most : c + o;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int v = 0;
        for (int w = 0; w < DMVS_BLOCK / 64; ++w) v = part[w] > most - v ? most : v + part[w];
        if (v) atomicAdd(out, v);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(DMVS_BLOCK)
label_hook_kernel(const int32_t* __restrict__ faces, long F, long N, unsigned* label, int* state, int most) {
    int wrote = 0, bad = 0;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    for (long f = tid; f < F; f += stride) {
        const int32_t x[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        if (x[0] < 0 || x[1] < 0 || x[2] < 0 || (long)x[0] >= N || (long)x[1] >= N || (long)x[2] >= N) {
            ++bad;
            continue;
        }
        unsigned par[3], m = 0xffffffffu;
        for (int k = 0; k < 3; ++k) {
            par[k] = dmvs_peek_u32(label + x[k]);
            // (a label is a vertex index: a caller's value outside [0, N) is never followed)
            const unsigned gp = (long)par[k] < N ? dmvs_peek_u32(label + par[k]) : par[k];
            m = gp < m ? gp : m;
        }
        for (int k = 0; k < 3; ++k) {
            if ((long)par[k] < N) wrote += label_lower(label + par[k], m);
            wrote += label_lower(label + x[k], m);
        }
    }
    label_block_count(wrote, most, state);
    label_block_count(bad, most, state + 1);
}

__global__ void __launch_bounds__(DMVS_BLOCK)
label_shortcut_kernel(long N, unsigned* label, int* state, int most) {
    int wrote = 0;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    for (long v = tid; v < N; v += stride) {
        const unsigned par = dmvs_peek_u32(label + v);
        if ((long)par >= N) continue;
        wrote += label_lower(label + v, dmvs_peek_u32(label + par));
    }
    label_block_count(wrote, most, state);
}

// ------------------------------------------------------------------------------------------ areas and component sums
struct MeshArrays {
    const float* verts;
    const int32_t* faces;
    long N, F;
};

__device__ __forceinline__ bool mesh_face(const MeshArrays& m, long f, int32_t x[3]) {
    x[0] = m.faces[3 * f], x[1] = m.faces[3 * f + 1], x[2] = m.faces[3 * f + 2];
    return x[0] >= 0 && x[1] >= 0 && x[2] >= 0 && (long)x[0] < m.N && (long)x[1] < m.N && (long)x[2] < m.N;
}

__device__ __forceinline__ long long tally_area_q(const MeshArrays& m, const int32_t x[3], double scale, double cap) {
#pragma clang fp contract(off)
    double p[3][3];
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) p[k][i] = (double)m.verts[3 * (long)x[k] + i];
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    return isfinite(area) ? (long long)llrint(fmin(area * scale, cap)) : 0ll;
}

#define TALLY_ROOTS 4      // distinct roots of one wave that are summed across its lanes; lanes with further ones issue their own atomics

template <bool COMBINE>
__global__ void __launch_bounds__(DMVS_BLOCK)
tally_kernel(MeshArrays m, const int32_t* __restrict__ label, double scale, double cap, int64_t* __restrict__ area_q, int* comp_faces,
             unsigned long long* comp_area) {
    __shared__ unsigned w_root[DMVS_BLOCK / 64];
    __shared__ int w_cnt[DMVS_BLOCK / 64];
    __shared__ unsigned long long w_sum[DMVS_BLOCK / 64];
    // what the wave holds back (the same in all its lanes): faces and area of acc_root not yet added to the tables
    unsigned acc_root = 0;
    int acc_cnt = 0;
    unsigned long long acc_sum = 0;
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    // the trip count is the wave's, not the lane's: every lane of a wave reaches every shuffle
    for (long f0 = tid - (threadIdx.x & 63); f0 < m.F; f0 += stride) {
        const long f = f0 + (threadIdx.x & 63);
        int root = -1;
        long long q = 0;
        if (f < m.F) {
            int32_t x[3];
            if (mesh_face(m, f, x)) {
                q = tally_area_q(m, x, scale, cap);
                root = label[x[0]];
                if (root < 0 || (long)root >= m.N) root = -1;      // (never with labels of dmvs_mesh_label_round_i32)
                if (root < 0) q = 0;
            }
            area_q[f] = q;
        }
        if (!COMBINE) {
            if (root >= 0) {
                atomicAdd(comp_faces + root, 1);
                if (q) atomicAdd(comp_area + root, (unsigned long long)q);
            }
            continue;
        }
        // up to TALLY_ROOTS times: the smallest root among the lanes still waiting, the count and area of the lanes that have it
        bool waiting = root >= 0;
        for (int pass = 0; pass < TALLY_ROOTS; ++pass) {
            unsigned lead = waiting ? (unsigned)root : 0xffffffffu;
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned o = __shfl_xor(lead, off);
                lead = o < lead ? o : lead;
            }
            if (lead == 0xffffffffu) break;                   // (wave-uniform) nobody waits
            const bool mine = waiting && (unsigned)root == lead;
            int cnt = mine ? 1 : 0;
            unsigned long long sum = mine ? (unsigned long long)q : 0ull;
            for (int off = 32; off > 0; off >>= 1) {
                cnt += __shfl_xor(cnt, off);
                sum += __shfl_xor(sum, off);
            }
            waiting = waiting && !mine;
            if (acc_cnt == 0 || acc_root == lead) {
                acc_root = lead, acc_cnt += cnt, acc_sum += sum;      // (at most F < 2^31 faces, their areas below 2^62: dmvs.h)
                continue;
            }
            // another root than the one held back: the smaller lot goes out, the larger stays
            unsigned out_root = lead;
            int out_cnt = cnt;
            unsigned long long out_sum = sum;
            if (cnt > acc_cnt) {
                out_root = acc_root, out_cnt = acc_cnt, out_sum = acc_sum;
                acc_root = lead, acc_cnt = cnt, acc_sum = sum;
            }
            if ((threadIdx.x & 63) == 0) {
                atomicAdd(comp_faces + out_root, out_cnt);
                if (out_sum) atomicAdd(comp_area + out_root, out_sum);
            }
        }
        if (waiting) {                                        // more roots in one wave than that: every lane left for itself
            atomicAdd(comp_faces + root, 1);
            if (q) atomicAdd(comp_area + root, (unsigned long long)q);
        }
    }
    if (!COMBINE) return;
    // the workgroup's waves meet in LDS: one pair of atomics per distinct root
    if ((threadIdx.x & 63) == 0) w_root[threadIdx.x >> 6] = acc_root, w_cnt[threadIdx.x >> 6] = acc_cnt, w_sum[threadIdx.x >> 6] = acc_sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < DMVS_BLOCK / 64; ++w) {
            if (w_cnt[w] == 0) continue;
            for (int v = w + 1; v < DMVS_BLOCK / 64; ++v)
                if (w_cnt[v] > 0 && w_root[v] == w_root[w]) w_cnt[w] += w_cnt[v], w_sum[w] += w_sum[v], w_cnt[v] = 0;
            atomicAdd(comp_faces + w_root[w], w_cnt[w]);
            if (w_sum[w]) atomicAdd(comp_area + w_root[w], w_sum[w]);
        }
    }
}

// ------------------------------------------------------------------------------------------ sampling
__global__ void __launch_bounds__(DMVS_BLOCK)
sample_kernel(MeshArrays m, const int64_t* __restrict__ area_cum, int64_t a0, long M, float* __restrict__ points, int32_t* __restrict__ face_of) {
#pragma clang fp contract(off)
    const long tid = (long)blockIdx.x * DMVS_BLOCK + threadIdx.x, stride = (long)gridDim.x * DMVS_BLOCK;
    for (long k = tid; k < M; k += stride) {
        const int64_t t = (int64_t)k * a0 + (a0 >> 1);
        long lo = 0, hi = m.F;                              // the smallest f with area_cum[f] > t (F if none: the caller's M was too large)
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (area_cum[mid] > t) hi = mid; else lo = mid + 1;
        }
        int32_t x[3];
        float out[3] = {0.0f, 0.0f, 0.0f};
        int32_t fo = -1;
        if (lo < m.F && mesh_face(m, lo, x)) {
            double r1 = (double)(uint32_t)((uint32_t)k * 3242174889u) * (1.0 / 4294967296.0);
            double r2 = (double)(uint32_t)((uint32_t)k * 2447445414u) * (1.0 / 4294967296.0);
            if (r1 + r2 > 1.0) r1 = 1.0 - r1, r2 = 1.0 - r2;
            for (int i = 0; i < 3; ++i) {
                const double p0 = (double)m.verts[3 * (long)x[0] + i];
                const double a = (double)m.verts[3 * (long)x[1] + i] - p0, b = (double)m.verts[3 * (long)x[2] + i] - p0;
                out[i] = (float)((p0 + r1 * a) + r2 * b);
            }
            fo = (int32_t)lo;
        }
        points[3 * k] = out[0], points[3 * k + 1] = out[1], points[3 * k + 2] = out[2];
        face_of[k] = fo;
    }
}

inline bool mesh_sizes_ok(int64_t N, int64_t F) { return N >= 0 && F >= 0 && N <= 2147483647L && F <= 2147483647L; }

}  // namespace

extern "C" int dmvs_mesh_label_round_i32(const int32_t* faces, int64_t F, int64_t N, int32_t* label, int32_t* state, int32_t blocks, void* stream) {
    if (!mesh_sizes_ok(N, F) || blocks < 0) return DMVS_EINVAL;
    if (((uintptr_t)faces & 3u) || ((uintptr_t)label & 3u) || ((uintptr_t)state & 3u)) return DMVS_EINVAL;
    if (!state || (F > 0 && !faces) || (N > 0 && !label)) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t err = hipMemsetAsync(state, 0, 2 * sizeof(int32_t), s);
    if (err != hipSuccess) return (int)err;
    if (F == 0 || N == 0) return 0;      // (N = 0: every face is out of range; the caller's labels are an empty array either way)
    unsigned* lab = reinterpret_cast<unsigned*>(label);
    int* st = reinterpret_cast<int*>(state);
    const unsigned gf = cloud_sum_blocks(F, blocks), gn = cloud_sum_blocks(N, blocks);
    const int most = (int)(2147483647L / ((long)gf + gn));
    hipLaunchKernelGGL(label_hook_kernel, dim3(gf), dim3(DMVS_BLOCK), 0, s, faces, (long)F, (long)N, lab, st, most);
    hipLaunchKernelGGL(label_shortcut_kernel, dim3(gn), dim3(DMVS_BLOCK), 0, s, (long)N, lab, st, most);
    return dmvs_launch_status();
}

extern "C" int dmvs_mesh_face_tally_i64(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int32_t* label, double scale, double cap,
                                        int64_t* area_q, int32_t* comp_faces, int64_t* comp_area, int32_t blocks, void* stream) {
    if (!mesh_sizes_ok(N, F) || blocks < 0 || !cloud_pow2(scale)) return DMVS_EINVAL;
    if (!(cap >= 0.0) || !(cap < 4611686018427387904.0)) return DMVS_EINVAL;      // (false for NaN; llrint stays in range)
    if (((uintptr_t)verts & 3u) || ((uintptr_t)faces & 3u) || ((uintptr_t)label & 3u) || ((uintptr_t)comp_faces & 3u)) return DMVS_EINVAL;
    if (((uintptr_t)area_q & 7u) || ((uintptr_t)comp_area & 7u)) return DMVS_EINVAL;
    if (N > 0 && (!comp_faces || !comp_area)) return DMVS_EINVAL;
    if (F > 0 && N > 0 && (!faces || !area_q || !verts || !label)) return DMVS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = N > 0 ? hipMemsetAsync(comp_faces, 0, (size_t)N * sizeof(int32_t), s) : hipSuccess;
    if (err == hipSuccess && N > 0) err = hipMemsetAsync(comp_area, 0, (size_t)N * sizeof(int64_t), s);
    if (err != hipSuccess) return (int)err;
    if (F == 0 || N == 0) return 0;
    MeshArrays m = {verts, faces, (long)N, (long)F};
    const dim3 grid(cloud_sum_blocks(F, blocks > 0 ? blocks : 2048)), block(DMVS_BLOCK);      // (a workgroup ends in a pair of atomics: no more of them than fill the chip)
    int* cf = reinterpret_cast<int*>(comp_faces);
    unsigned long long* ca = reinterpret_cast<unsigned long long*>(comp_area);
#ifdef DMVS_MESH_TALLY_PLAIN
    hipLaunchKernelGGL(tally_kernel<false>, grid, block, 0, s, m, label, scale, cap, area_q, cf, ca);
#else
    hipLaunchKernelGGL(tally_kernel<true>, grid, block, 0, s, m, label, scale, cap, area_q, cf, ca);
#endif
    return dmvs_launch_status();
}

extern "C" int dmvs_mesh_sample_f32(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int64_t* area_cum, int64_t a0, int64_t M,
                                    float* points, int32_t* face_of, int32_t blocks, void* stream) {
    if (!mesh_sizes_ok(N, F) || blocks < 0 || a0 < 1 || M < 0 || M > 2147483647L) return DMVS_EINVAL;
    if (((uintptr_t)verts & 3u) || ((uintptr_t)faces & 3u) || ((uintptr_t)points & 3u) || ((uintptr_t)face_of & 3u) || ((uintptr_t)area_cum & 7u))
        return DMVS_EINVAL;
    if (M > 0 && F > 0 && N > 0 && (!points || !face_of || !faces || !area_cum || !verts)) return DMVS_EINVAL;
    if (M > 0 && (double)M * (double)a0 >= 9223372036854775808.0) return DMVS_EINVAL;      // k a0 must stay an int64
    if (M == 0 || F == 0 || N == 0) return 0;
    MeshArrays m = {verts, faces, (long)N, (long)F};
    hipLaunchKernelGGL(sample_kernel, dim3(cloud_sum_blocks(M, blocks)), dim3(DMVS_BLOCK), 0, (hipStream_t)stream, m, area_cum, a0, (long)M, points,
                       face_of);
    return dmvs_launch_status();
}
