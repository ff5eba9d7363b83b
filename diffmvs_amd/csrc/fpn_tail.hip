// FeatureNet's FPN tail for stage 2 (reference models/module.py:409-411) in ONE kernel:
//   intra  = inner1(c2) + nearest_up2(c3)      1x1, 32 -> 64, bias: exact fp32 (v_mfma_f32_16x16x4_f32, the chain of conv1x1_px4_kernel)
//   stage2 = out2(intra)                       3x3, 64 -> 32, zero padding, no bias / BN / activation: split-bf16, channel-last fp32 output
// As two launches the 64-channel `intra` is written and read back by its only reader (DiffMVS has no out3): 2 x 3.02 GB per 576-image headline
// step.  Here it never leaves LDS:
//   * work unit = (image, strip of S = 32 output columns, segment of R = 64 output rows); persistent workgroups of 4 waves take units round-robin,
//     the grid comes from the occupancy query (two workgroups per CU: LDS);
//   * inside a unit the workgroup marches DOWN the rows, two rows per step, over a ring of `intra` as bf16 triples
//     [plane hi / mid / lo][4 row slots][chunk of 8 channels][34 positions][8 channels] (slot = (image row + 4) & 3, position p = column X0 - 1 + p):
//     exactly the four rows that two output rows read.  `intra` rows are paired ODD row first, (Y0 - 1 + 2p, Y0 + 2p), so that an output pair reads
//     two whole intra pairs; a pair therefore reads TWO c3 rows, of which one was staged for the pair above: the c3 staging buffer has two row
//     slots (c3 row & 1) and one new row per step;
//   * every wave does both layers.  Step j:
//       phase 1 (LDS is read only)   out2: wave (n-tile nt = wave & 1, row rr = wave >> 1) computes output row Y0 + 2 (j - 2) + rr, both 16-pixel
//                                    groups, for its 16 output channels: 24 (chunk, tap group) steps of 12 MFMAs; the lane's pre-split weights
//                                    (ops.split_weights(out2), 147,456 bytes: neither registers nor LDS hold them) stream from L2 two steps
//                                    ahead in three register sets, the pixel operands from the ring one step ahead in two
//                                    inner1: wave w computes output channels 16 w .. + 15 of intra rows Y0 - 1 + 2j, Y0 + 2j (3 groups of 16
//                                    positions each) from the staged c2 rows -- its 8 weight registers never change -- then + bias, + the staged
//                                    c3 value of (row >> 1, column >> 1), ZERO outside the image (out2 pads with zeros, not with bias + 0)
//       barrier (LDS only)
//       phase 2                      the 16-byte LDS-DMA pieces of the next pair's c2 rows and its new c3 row are issued (the staging buffers are
//                                    free: inner1's values are in registers); out2's accumulators leave as 16-byte channel-last stores (128
//                                    contiguous bytes per pixel over the 8 lanes / waves that hold it); inner1's values -> dmvs_split3_bf16x8,
//                                    once per element, into the ring over the rows out2 finished with
//       barrier (DMVS_DMA_BARRIER: it publishes the staged rows)
//     (the DMA flies under phase 2 and the other resident workgroup's phase 1, not under this workgroup's weight stream: vector-memory
//     operations return in order, so a DMA issued in front of a weight load would make that load's wait a wait for HBM; and not under the
//     fp32 MFMAs, which stop the CU's vector memory)
//   * steps 0-1 of a unit only stage and run inner1 (the row above the segment is recomputed with the same instructions on the same operands as
//     in the segment above: every value depends only on its position in the image), the last step only finishes out2;
//   * bits: per `intra` value the k-ordered fp32 chain of conv1x1_px4_kernel (channel groups of 4 ascending, weights as the first operand),
//     acc * 1 + bias, + c3; per output accumulator the matrix instructions of conv2d_mfma_kernel's split form, channel-last instantiation, in its
//     order: chunk outermost, tap group g (slots beyond tap 8 read tap 8's operand against zero weights), the six partial products lo*hi, hi*lo,
//     mid*mid, mid*hi, hi*mid, hi*hi (pixel part * weight part), weights as the first operand (D[cout 4*kq + r][pixel m]); the triples are what its
//     conversion pass builds from the stored fp32 value: the result is the two launches' bit for bit.
// LDS: 52,224 (ring) + 10,240 (c2 rows: [2][32 channels][40 = the aligned cover of columns X0 - 1 .. X0 + 32]) + 12,288 (c3: [2 slots][64][24])
// = 74,752 bytes.  Costs of the unit shape: inner1 computes 3 groups of 16 positions for 34 (32 output columns), 66 rows per 64; out2 has no padding
// at W % 32 == 0.

#include "dmvs_common.h"
#include "dmvs_ring.h"
#include "dmvs_lds_poison.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));

constexpr int PB = 256;                     // threads per workgroup
constexpr int US = 32, UR = 64;             // a unit's output columns / rows
constexpr int NP = US + 2;                  // ring positions per row: columns X0 - 1 .. X0 + 32
constexpr int NCH = 8;                      // chunks of 8 intra channels
typedef dmvs_ring<NCH, NP> Ring;            // 52,224 bytes
constexpr int PLQ = Ring::PLQ, RINGQ = Ring::RINGQ;
constexpr int SW = US + 8;                  // a staged c2 row: the 16-byte aligned cover of columns X0 - 1 .. X0 + 32 = columns X0 - 4 .. X0 + 35
constexpr int C2PIECE = 2 * 32 * SW / 4;    // [2 rows][32 channels][40]: 640 16-byte pieces
constexpr int CW = US / 2 + 8;              // a staged c3 row: c3 columns X0 / 2 - 4 .. X0 / 2 + 19 (needed: X0 / 2 - 1 .. X0 / 2 + 16)
constexpr int C3PIECE = 64 * CW / 4;        // [64 channels][24]: 384 pieces per row slot
constexpr int LDSF = RINGQ * 4 + C2PIECE * 4 + 2 * C3PIECE * 4;
constexpr int NSTEP = NCH * 3;              // (chunk, tap group) steps of an output row

__global__ void __launch_bounds__(PB) __attribute__((amdgpu_waves_per_eu(2, 2)))      // two workgroups per CU (LDS): 2 waves per SIMD
featurenet_fpn_tail_kernel(const float* __restrict__ c2, const float* __restrict__ c3, const float* __restrict__ w1, const float* __restrict__ b1,
                           const u32x4s* __restrict__ ws2, float* __restrict__ y, int N, int H, int W, int nsx, int nsy) {
    // ONE LDS object (stem.hip): the ring, the c2 staging rows, the two c3 staging rows
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    DMVS_LDS_POISON(lds);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, kq = lane >> 4;
    const int H2 = H >> 1, W2 = W >> 1;
    const int iplane = H * W, iplane3 = H2 * W2;
    const int nunits = nsx * nsy * N;

    // inner1: this wave's 16 output channels; the lane's weights [channel group c] for (cin 4c + kq, cout 16 wave + m), bias of couts 16 wave + 4 kq + r
    float w1r[8], b1r[4];
#pragma unroll
    for (int c = 0; c < 8; ++c) w1r[c] = w1[(4 * c + kq) * 64 + 16 * wave + m];
#pragma unroll
    for (int r = 0; r < 4; ++r) b1r[r] = b1 ? b1[16 * wave + 4 * kq + r] : 0.0f;
    // out2: this wave's n-tile and row of the pair; the lane's pre-split weights [chunk][tap group][plane] for (tap slot kq, cout 16 nt + m)
    const int nt = wave & 1, rr = wave >> 1;
    unsigned lwb = (unsigned)(kq * 32 + nt * 16 + m) * 16u;      // byte offset of the lane's quad inside a (chunk, tap group, plane) slab of 2048 bytes
    auto wload = [&](int sp) -> u32x4s {      // uniform slab base + 32-bit lane offset: one address register for all 72 loads of a row
        return *reinterpret_cast<const u32x4s*>(reinterpret_cast<const char*>(ws2 + sp * 128) + lwb);
    };
    int taps = 0;       // (ky | kx << 2) of tap group g in bits 4g .. 4g + 3: dmvs_ring::operand
#pragma unroll
    for (int g = 0; g < 3; ++g) taps |= dmvs_tap_slot<3, 3, 2>(g, kq) << (4 * g);
    u32x4s* const ring = reinterpret_cast<u32x4s*>(lds);
    float* const st2 = lds + RINGQ * 4;
    float* const st3 = st2 + C2PIECE * 4;

    int lm = m, ltid = tid;      // (redefined opaquely per step)

    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const dmvs_unit u(unit, nsx, nsy, US, UR, H);
        const int n = u.n, X0 = u.X0, Y0 = u.Y0, Yend = u.Yend;
        const int Q = (Yend - Y0 + 1) >> 1;      // output row pairs (H is even): intra pairs 0 .. Q, steps 0 .. Q + 1
        const float* const c2b = c2 + (long)n * 32 * iplane;
        const float* const c3b = c3 + (long)n * 64 * iplane3;
        float* const yb = y + (long)n * 32 * iplane;

        // the 16-byte LDS-DMA pieces of intra pair p: c2 rows Y0 - 1 + 2p, Y0 + 2p and c3 row Y0 / 2 + p (with_above: also c3 row Y0 / 2 + p - 1,
        // which every later pair finds staged by the pair above).  A piece lies wholly inside or outside the tensors (W % 8 == 0); outside, it
        // reads the zero source
        auto stage_c3 = [&](int row3, int lt) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k * PB + wave * 64 < C3PIECE) {      // (wave-uniform: 384 pieces = 6 waves' worth)
                    const int e = k * PB + lt;
                    const int ch = e / (CW / 4), pc = e - ch * (CW / 4);
                    const int col = (X0 >> 1) - 4 + 4 * pc;
                    const bool ok = row3 >= 0 && row3 < H2 && col >= 0 && col < W2;
                    const float* srcp = ok ? c3b + (ch * iplane3 + row3 * W2 + col) : dmvs_zero16;
                    float* dstp = st3 + (((row3 + 2) & 1) * C3PIECE + k * PB + wave * 64) * 4;
                    __builtin_amdgcn_global_load_lds(srcp, DMVS_LDS_PTR(dstp), 16, 0, 0);
                }
            }
        };
        auto stage = [&](int p, bool with_above, int lt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k * PB + wave * 64 < C2PIECE)      // (wave-uniform: 640 pieces = 10 waves' worth)
                    dmvs_stage_piece<2, 32, SW>(c2b, iplane, H, W, Y0 - 1 + 2 * p, X0 - 4, true, k * PB + lt, st2 + (k * PB + wave * 64) * 4);
            }
            stage_c3((Y0 >> 1) + p, lt);
            if (with_above) stage_c3((Y0 >> 1) + p - 1, lt);
        };
        stage(0, true, ltid);
        DMVS_DMA_BARRIER();

        for (int j = 0; j < Q + 2; ++j) {
            DMVS_OPAQUE(lm);
            DMVS_OPAQUE(ltid);
            DMVS_OPAQUE(lwb);
            const bool do_out = j >= 2, do_in = j <= Q;      // (wave-uniform)
            // ---- phase 1, out2: output row orow, positions 16 grp + m, couts 16 nt + 4 kq + r
            const int orow = Y0 + 2 * (j - 2) + rr;
            f32x4 oacc[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
            if (do_out) {
                auto qp_of = [&](int s) { return Ring::operand(s, taps, orow, lm); };
                u32x4s wq[3][3];         // [register set][plane]: the weights of steps s, s + 1, s + 2
                bf16x8 pq[2][3][2];      // [register set][plane][group]: the pixel operands of steps s, s + 1
#pragma unroll
                for (int s0 = 0; s0 < 2; ++s0)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) wq[s0][pl] = wload(s0 * 3 + pl);
                {
                    const int qp = qp_of(0);
#pragma unroll
                    for (int grp = 0; grp < 2; ++grp)
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) pq[0][pl][grp] = __builtin_bit_cast(bf16x8, ring[pl * PLQ + qp + 16 * grp]);
                }
#pragma unroll
                for (int s = 0; s < NSTEP; ++s) {
                    const int wb = s % 3, pb = s & 1;
                    __builtin_amdgcn_sched_barrier(0);
                    if (s + 2 < NSTEP) {
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) wq[(s + 2) % 3][pl] = wload((s + 2) * 3 + pl);
                    }
                    if (s + 1 < NSTEP) {
                        const int qn = qp_of(s + 1);
#pragma unroll
                        for (int grp = 0; grp < 2; ++grp)
#pragma unroll
                            for (int pl = 0; pl < 3; ++pl) pq[pb ^ 1][pl][grp] = __builtin_bit_cast(bf16x8, ring[pl * PLQ + qn + 16 * grp]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    // (the two groups' MFMAs of one product are independent)
                    dmvs_split_step<2, false>(pq[pb][0], pq[pb][1], pq[pb][2], __builtin_bit_cast(bf16x8, wq[wb][0]), __builtin_bit_cast(bf16x8, wq[wb][1]),
                                              __builtin_bit_cast(bf16x8, wq[wb][2]), oacc);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- phase 1, inner1: intra rows Y0 - 1 + 2j + li, positions 16 grp + m (3 groups cover the 34), couts 16 wave + 4 kq + r
            float iv[6][4];
            if (do_in) {
#pragma unroll
                for (int it = 0; it < 6; ++it) {
                    const int li = it / 3, grp = it - li * 3;
                    const int row = Y0 - 1 + 2 * j + li;
                    const int pp = min(grp * 16 + lm, NP - 1);
                    const float* xp = st2 + (li * 32 + kq) * SW + 3 + pp;
                    f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int c = 0; c < 8; ++c) a = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[c], xp[4 * c * SW], a, 0, 0, 0);
                    const int col = X0 - 1 + pp;
                    const bool inside = row >= 0 && row < H && col >= 0 && col < W;
                    // c3 row row >> 1 = Y0 / 2 + j - 1 + li lies in staging slot (row >> 1) & 1, c3 column col >> 1 at index ((pp - 1) >> 1) + 4
                    const float* rp = st3 + ((((row + 4) >> 1) & 1) * 64 + 16 * wave + 4 * kq) * CW + ((pp - 1) >> 1) + 4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = (a[r] + b1r[r]) + rp[r * CW];
                        iv[it][r] = inside ? v : 0.0f;
                    }
                }
            }
            DMVS_LDS_BARRIER();     // everyone is done reading the ring rows and the staging buffers phase 2 overwrites (ds accesses only)
            // ---- phase 2: the next pair starts streaming; the output stores; inner1's values as bf16 triples into the ring
            if (j + 1 <= Q) stage(j + 1, false, ltid);
            if (do_out) {
#pragma unroll
                for (int grp = 0; grp < 2; ++grp) {
                    const int col = X0 + grp * 16 + m;
                    if (col < W) *reinterpret_cast<f32x4*>(yb + ((orow * W + col) * 32 + nt * 16 + 4 * kq)) = oacc[grp];
                }
            }
            if (do_in) {
#pragma unroll
                for (int it = 0; it < 6; ++it) {
                    const int li = it / 3, grp = it - li * 3;
                    const int row = Y0 - 1 + 2 * j + li;
                    const int pp = grp * 16 + m;
                    if (pp < NP) {
                        // channels 16 wave + 4 kq .. + 3 = chunk 2 wave + (kq >> 1), k-slots 4 (kq & 1) .. + 3: 8 bytes per plane
                        dmvs_store_split4(iv[it], reinterpret_cast<dmvs_u32x2*>(ring + Ring::index(row, 2 * wave + (kq >> 1), pp)) + (kq & 1), PLQ * 2);
                    }
                }
            }
            DMVS_DMA_BARRIER();     // the staged rows have landed, the ring holds the next step's rows
        }
    }
}

}  // namespace

extern "C" int dmvs_featurenet_fpn_tail_f32(const float* c2, const float* c3, const float* w_inner, const float* b_inner, const void* wsplit_out,
                                            float* y, int32_t N, int32_t H, int32_t W, int32_t tune, void* stream) {
    if (!c2 || !c3 || !w_inner || !wsplit_out || !y || N <= 0 || H <= 0 || W <= 0) return DMVS_EINVAL;
    // c3 is the half-resolution map (H even) and its rows are whole 16-byte pieces (W % 8 == 0); 32-bit offsets inside an image
    if ((H & 1) || (W & 7) || (long)64 * H * W >= (1L << 31)) return DMVS_EINVAL;
    if ((((uintptr_t)c2 | (uintptr_t)c3 | (uintptr_t)y | (uintptr_t)wsplit_out) & 15) || ((uintptr_t)w_inner & 3) || ((uintptr_t)b_inner & 3))
        return DMVS_EINVAL;
    const int nsx = (W + US - 1) / US, nsy = (H + UR - 1) / UR;
    const long nunits = (long)nsx * nsy * N;
    if (nunits >= (1L << 31)) return DMVS_EINVAL;
    // persistent workgroups: as many as are resident at once; tune & 0xffff forces the grid (tests: results do not depend on it)
    static const int resident = dmvs_resident_workgroups(reinterpret_cast<const void*>(featurenet_fpn_tail_kernel), PB);
    hipLaunchKernelGGL(featurenet_fpn_tail_kernel, dim3(dmvs_persistent_grid(tune, resident, nunits)), dim3(PB), 0, (hipStream_t)stream, c2, c3, w_inner, b_inner,
                       reinterpret_cast<const u32x4s*>(wsplit_out), y, N, H, W, nsx, nsy);
    return dmvs_launch_status();
}
