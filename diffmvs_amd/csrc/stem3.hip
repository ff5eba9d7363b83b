// FeatureNet stem, three layers in ONE kernel: conv0.0 (3->8, 3x3) + conv0.1 (8->8, 3x3) at full resolution and conv1.0 (8->16, 5x5, stride 2) on
// top of them, each with folded BN + ReLU (reference models/module.py:364-371, :399-400).  In inference the full-resolution 8-channel map c0 has
// exactly one consumer, conv1.0: as two launches (stem.hip + the generic stride-2 kernel) it is written and read back -- 12 GB per 576-image
// headline step -- and conv1.0 runs the exact-fp32 MFMA because a chunked LDS-tiled kernel cannot pay for the split's conversion pass.  Here c0
// never leaves LDS, and conv0.1's epilogue, which holds every c0 value in a register anyway, writes it as the bf16 triples conv1.0 multiplies.
//   * work unit = (image, strip of 32 output columns, segment of 32 output rows); persistent workgroups take units round-robin;
//   * inside a unit the workgroup marches DOWN the rows with three LDS rings instead of a halo'd tile.  Step k consumes 4 new input rows
//     (group k, staged by 16-byte LDS-DMA one whole step ahead: issued behind the second barrier of step k - 2, waited for at that of step k - 1) and produces
//       mid rows 4k .. 4k+3  (conv0.0: exact-fp32 MFMA on row pairs, K = (ci, input row j, kx) = 36, as in stem.hip)      -> mid ring, bf16 triples
//       c0  rows 4k .. 4k+3  (conv0.1: split-bf16 on row pairs, K = 96 = 3 steps of v_mfma_f32_16x16x32_bf16, k >= 1)     -> c0 ring, bf16 triples
//       2 output rows        (conv1.0: split-bf16, K = 8 channels x 28 tap slots (25 taps + 3 zero-weight slots) = 7 steps, k >= 2;
//                             one 16-pixel group per wave, 16-byte NCHW stores through transposed accumulators)
//     ("row r" of a ring = image row Y0 - 5 + r (input), Y0 - 6 + r (mid), Y0 - 7 + r (c0), Y0 = the segment's first full-resolution row; the
//     mid and c0 rings hold 8 rows, slot = r & 7, the input ring three groups of 4.)  Steps 0 and 1 are the warm-up: they recompute the mid / c0 rows above the segment's first output row,
//     with the same instructions on the same operands as the segment above -- every value depends only on its position in the image;
//   * the intermediates are ZERO outside the image (the next layer's zero padding), not the previous layer applied to padding;
//   * every split product is the sum of six partial products, smallest first: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi; one accumulator
//     per output;
//   * two barriers per step: an LDS-only one after conv0.0 (mid complete) and the DMA-publishing one after conv0.1 (c0 complete, the next step's input
//     group has landed; the group after that is issued right behind it, into the slot conv0.0 finished with before the first barrier).
// Halo recompute: conv0.1 (67 x 68)/(64 x 64), conv0.0 (69 x 70)/(64 x 64) -- stem.hip's 18 x 18 tile costs 1.27 for conv0.0.

#include "dmvs_common.h"
#include "dmvs_ring.h"
#include "dmvs_lds_poison.h"

#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));

constexpr int UC = 32, UR = 32;                     // a unit's output columns / rows (half resolution)
constexpr int INW = 72;                             // input ring row: the 16-byte aligned cover of columns 2*ox0 - 4 .. + 67
constexpr int INROW = 3 * INW, INGRP = 4 * INROW;   // ring layout [12 rows][3 channels][72]: a group of 4 rows is 216 contiguous 16-byte pieces
constexpr int INSLOTS = 3;                          // groups k - 1 and k under conv0.0 of step k, group k + 1 landing
constexpr int INF = INSLOTS * INGRP;
constexpr int NPIECE = INGRP / 4;                   // 216 <= DMVS_BLOCK: one DMA instruction per wave and step
constexpr int MW = 2 * UC + 5, CW = 2 * UC + 3;     // mid ring row: columns 2*ox0 - 3 .. + 65 (69); c0 ring row: 2*ox0 - 2 .. + 64 (67)
constexpr int MPL = 8 * MW, CPL = 8 * CW;           // one bf16 plane [8 rows][positions] of 16-byte (8-channel) entries
constexpr int MIDF = 3 * MPL * 4, C0F = 3 * CPL * 4;
constexpr int K0S = 9;                              // conv0.0: 36 k-slots = 9 MFMA steps
constexpr int K2S = 7;                              // conv1.0: 28 tap slots x 8 channels = 7 bf16 MFMA steps

__global__ void __launch_bounds__(DMVS_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))      // two workgroups per CU (LDS): at most 256 registers
featurenet_stem3_kernel(const float* __restrict__ x, const float* __restrict__ w0, const float* __restrict__ scale0, const float* __restrict__ shift0,
                        const float* __restrict__ w1, const float* __restrict__ scale1, const float* __restrict__ shift1,
                        const float* __restrict__ w2, const float* __restrict__ scale2, const float* __restrict__ shift2, float* __restrict__ y,
                        int N, int H, int W, int nsx, int nsy) {
    // ONE LDS object (stem.hip: separate arrays get alias scopes and an early vmcnt(0) that waits the prefetch out): 61.1 KB
    __shared__ __attribute__((aligned(16))) float lds[INF + MIDF + C0F];
    DMVS_LDS_POISON(lds);
    float* const s_in = lds;
    float* const s_mid = lds + INF;
    float* const s_c0 = s_mid + MIDF;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, kq = lane >> 4;
    const int Ho = H >> 1, Wo = W >> 1;
    const long plane = (long)H * W, oplane = (long)Ho * Wo;
    const int nunits = nsx * nsy * N;

    // conv0.0: A = paired w0[k = 4s + kq][row m] (rows 0-7: tap row ky = j for the pair's first mid row, rows 8-15: ky = j - 1 for the second),
    // B offsets of k = (ci, j, kx) from the pair's first input row; koff_b: the same for a window that starts at ring row 10 (rows j >= 2 wrap)
    float a0[K0S];
    int koff[K0S];          // koff_a | (koff_b + 4 * INSLOTS * INROW) << 16
#pragma unroll
    for (int s = 0; s < K0S; ++s) {
        const int k = 4 * s + kq;
        const int ci = k / 12, j = (k - ci * 12) / 3, kx = k % 3;
        const int ky = m < 8 ? j : j - 1;
        a0[s] = (ky >= 0 && ky <= 2) ? w0[(ci * 9 + ky * 3 + kx) * 8 + (m & 7)] : 0.0f;
        const int koff_a = j * INROW + ci * INW + kx;
        koff[s] = koff_a | ((koff_a + (j >= 2 ? 0 : 4 * INSLOTS * INROW)) << 16);
    }
    // the lane's D rows 4*kq + r of conv0.0 AND conv0.1 (weights are the A operand of both): channel (4*kq + r) & 7 of pair row kq >> 1
    float sc0[4], sh0[4], sc1[4], sh1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = (4 * kq + r) & 7;
        sc0[r] = scale0 ? scale0[co] : 1.0f;
        sh0[r] = shift0 ? shift0[co] : 0.0f;
        sc1[r] = scale1 ? scale1[co] : 1.0f;
        sh1[r] = shift1 ? shift1[co] : 0.0f;
    }
    // conv0.1: the lane's paired weights as bf16 triples (matrix ROW m: the weights are the A operand), and its (mid row j, kx) slot of every step
    bf16x8 w1h[3], w1m[3], w1l[3];
    int off1[3];        // j | kx << 4
#pragma unroll
    for (int g = 0; g < 3; ++g) off1[g] = dmvs_tap_slot<4, 3>(g, kq);
    dmvs_conv01_paired_weights(w1, m, kq, w1h, w1m, w1l);
    // conv1.0: B = w2[k = (tap slot sl = 4s + kq, channel j)][cout m] as bf16 triples; slots 25-27 carry zero weights and read tap 24's operand
    bf16x8 w2h[K2S], w2m[K2S], w2l[K2S];
    int off2[K2S];      // ky | kx << 4
#pragma unroll
    for (int s = 0; s < K2S; ++s) {
        const int sl = 4 * s + kq;
        float wv[8];
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) wv[ci] = sl < 25 ? w2[(ci * 25 + sl) * 16 + m] : 0.0f;
        dmvs_split3_bf16x8(wv, w2h[s], w2m[s], w2l[s]);
        off2[s] = dmvs_tap_slot<5, 5>(s, kq);
    }
    const float sc2 = scale2 ? scale2[m] : 1.0f, sh2 = shift2 ? shift2[m] : 0.0f;
    const bool vec = (Wo & 3) == 0 && ((uintptr_t)y & 15) == 0;

    // input staging: group kg of a unit = image rows Y0 - 5 + 4*kg .. + 3, all 3 channels, columns X0 - 4 .. X0 + 67, as 216 16-byte pieces
    // (piece = (row i, channel, 4 columns): wholly inside or outside the image because W % 4 == 0); lane tid stages piece tid
    const int p_i = tid / (NPIECE / 4), p_rem = tid - p_i * (NPIECE / 4);
    const int p_ci = p_rem / (INW / 4), p_c = (p_rem - p_ci * (INW / 4)) * 4;
    auto stage = [&](int unit, int kg, int slot) {
        const dmvs_unit u(unit, nsx, nsy, UC, UR, Ho);
        const int row = 2 * u.Y0 - 5 + 4 * kg + p_i, col = 2 * u.X0 - 4 + p_c;
        if (tid < NPIECE) {
            const bool ok = row >= 0 && row < H && col >= 0 && col < W;
            const float* srcp = ok ? x + ((long)u.n * 3 + p_ci) * plane + (long)row * W + col : dmvs_zero16;
            float* dstp = s_in + slot * INGRP + wave * 256;
            __builtin_amdgcn_global_load_lds(srcp, DMVS_LDS_PTR(dstp), 16, 0, 0);
        }
    };

    auto steps_of = [&](int unit) {      // two output rows per step, two warm-up steps
        const dmvs_unit u(unit, nsx, nsy, UC, UR, Ho);
        return ((u.Yend - u.Y0 + 2) >> 1) + 2;
    };
    // the staging cursor runs TWO groups ahead of the step, across unit boundaries: a group is issued right behind the DMA-publishing barrier
    // of step k - 2 and waited for at that of step k - 1, so it has a whole step to land
    int s_unit = blockIdx.x, s_k = 0, s_slot = 0, s_steps = s_unit < nunits ? steps_of(s_unit) : 0;
    auto stage_next = [&]() {
        if (s_unit < nunits) {
            stage(s_unit, s_k, s_slot);
            s_slot = s_slot == INSLOTS - 1 ? 0 : s_slot + 1;
            if (++s_k == s_steps) {
                s_unit += gridDim.x;
                s_k = 0;
                s_steps = s_unit < nunits ? steps_of(s_unit) : 0;
            }
        }
    };
    int islot = 0, pslot = INSLOTS - 1;             // ring slots of the current step's input group and of the one before (run on across units)
    int unit = blockIdx.x;
    stage_next();
    stage_next();
    DMVS_DMA_BARRIER();
    for (; unit < nunits; unit += gridDim.x) {
        const dmvs_unit u(unit, nsx, nsy, UC, UR, Ho);      // in output (half-resolution) columns and rows
        const int n = u.n, ox0 = u.X0, oy0 = u.Y0, X0 = 2 * ox0, Y0 = 2 * oy0;
        const int nsteps = steps_of(unit);
        for (int k = 0; k < nsteps; ++k, pslot = islot, islot = islot == INSLOTS - 1 ? 0 : islot + 1) {
            // ---- conv0.0 -> mid rows 4k .. 4k+3: slots (row pair q, position) row-major over 2 x 69, 16 per MFMA group; step 0 needs pair 1 only.
            // A wave runs its groups (wave, wave + 4, wave + 8) two at a time: independent accumulator chains and epilogues -- one group
            // at a time, a wave (two per SIMD) waits out every LDS, MFMA and VALU latency in turn
            {
                const int sbeg = k == 0 ? MW : 0;
                const int ng = (2 * MW - sbeg + 15) >> 4;
                auto conv00 = [&](auto ngc, int g0) {
                    constexpr int NG = decltype(ngc)::value;
                    int q[NG], pm[NG];
                    float b[NG][K0S];
                    f32x4 acc[NG];
#pragma unroll
                    for (int i = 0; i < NG; ++i) {
                        const int p = min(sbeg + (g0 + 4 * i) * 16 + m, 2 * MW - 1);
                        q[i] = p >= MW ? 1 : 0;
                        pm[i] = p - q[i] * MW;
                        const int rb = q[i] ? 4 * islot : 4 * pslot + 2;       // ring row of the pair's first input row (input row 4k + 2q - 2)
                        const bool wrap = rb == 4 * INSLOTS - 2;
                        const float* ip = s_in + rb * INROW + pm[i] - (wrap ? 4 * INSLOTS * INROW : 0);
                        const int sh = wrap ? 16 : 0;
#pragma unroll
                        for (int s = 0; s < K0S; ++s) b[i][s] = ip[(koff[s] >> sh) & 0xffff];
                        acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    }
#pragma unroll
                    for (int s = 0; s < K0S; ++s)
#pragma unroll
                        for (int i = 0; i < NG; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b[i][s], acc[i], 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < NG; ++i) {
                        // D[row = 4*kq + r][col = m]: rows 0-7 = the 8 channels of mid pixel (4k + 2q, pm), rows 8-15 = those of (4k + 2q + 1, pm)
                        const int ml = 4 * k + 2 * q[i] + (kq >> 1);
                        const int gy = Y0 - 6 + ml, gx = X0 - 3 + pm[i];
                        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
                        if (sbeg + (g0 + 4 * i) * 16 + m < 2 * MW) {
                            float v[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = inside ? fmaxf(fmaf(acc[i][r], sc0[r], sh0[r]), 0.0f) : 0.0f;
                            dmvs_store_split4(v, reinterpret_cast<dmvs_u32x2*>(s_mid) + ((ml & 7) * MW + pm[i]) * 2 + (kq & 1), MPL * 2);
                        }
                    }
                };
                const int cnt = (ng - wave + 3) >> 2;       // groups wave, wave + 4, ... < ng
                if (cnt >= 2) conv00(std::integral_constant<int, 2>{}, wave);
                if (cnt & 1) conv00(std::integral_constant<int, 1>{}, wave + (cnt & 2) * 4);
            }
            DMVS_LDS_BARRIER();     // mid complete (ds_writes only; the group in flight stays in flight); everyone is done with the input group of step k - 1

            // ---- conv0.1 -> c0 rows 4k .. 4k+3 from mid rows 4k-2 .. 4k+3: slots (row pair, position) over 2 x 67
            if (k >= 1) {
                const u32x4s* const q_hi = reinterpret_cast<const u32x4s*>(s_mid);
                for (int g = (wave + 1) & 3; g < (2 * CW + 15) / 16; g += DMVS_BLOCK / 64) {       // (the wave with three conv0.0 groups takes two here)
                    const int p = min(g * 16 + m, 2 * CW - 1);
                    const int pr = p >= CW ? 1 : 0, pc = p - pr * CW;
                    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                    // all nine operand reads first, fenced: left alone the scheduler reuses one register quad per plane and waits out the
                    // LDS latency eight times per group
                    bf16x8 ph[3], pmid[3], pl[3];
#pragma unroll
                    for (int g3 = 0; g3 < 3; ++g3) {
                        const int mr = (4 * k + 6 + 2 * pr + (off1[g3] & 15)) & 7;         // mid row 4k - 2 + 2 pr + j
                        const int qp = mr * MW + pc + (off1[g3] >> 4);
                        ph[g3] = __builtin_bit_cast(bf16x8, q_hi[qp]);
                        pmid[g3] = __builtin_bit_cast(bf16x8, q_hi[MPL + qp]);
                        pl[g3] = __builtin_bit_cast(bf16x8, q_hi[2 * MPL + qp]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int g3 = 0; g3 < 3; ++g3) dmvs_split_step<1, false>(&ph[g3], &pmid[g3], &pl[g3], w1h[g3], w1m[g3], w1l[g3], &acc);
                    // D[row = 4*kq + r][col = m]: rows 0-7 = the 8 channels of c0 pixel (4k + 2 pr, pc), rows 8-15 = those of the row below
                    const int cl = 4 * k + 2 * pr + (kq >> 1);
                    const int gy = Y0 - 7 + cl, gx = X0 - 2 + pc;
                    const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    if (g * 16 + m < 2 * CW) {
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = inside ? fmaxf(fmaf(acc[r], sc1[r], sh1[r]), 0.0f) : 0.0f;
                        dmvs_store_split4(v, reinterpret_cast<dmvs_u32x2*>(s_c0) + ((cl & 7) * CW + pc) * 2 + (kq & 1), CPL * 2);
                    }
                }
            }
            DMVS_DMA_BARRIER();     // c0 complete; the next step's input group has landed
            stage_next();           // group k + 2, into the slot of group k - 1

            // ---- conv1.0: output rows oy0 + 2(k-2) + {0, 1} from c0 rows 4k-3 .. 4k+3; wave = (row, 16-pixel half), pixels are the A operand
            if (k >= 2) {
                const u32x4s* const q_hi = reinterpret_cast<const u32x4s*>(s_c0);
                const int orow = wave >> 1, i0 = 16 * (wave & 1);
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                // operand reads run two k-steps ahead of the MFMAs, fenced (see conv0.1)
                bf16x8 ph[K2S], pmid[K2S], pl[K2S];
                auto fetch = [&](int s) {
                    const int cr = (4 * k + 5 + 2 * orow + (off2[s] & 15)) & 7;             // c0 row 4k - 3 + 2 orow + ky
                    const int qp = cr * CW + 2 * (i0 + m) + (off2[s] >> 4);
                    ph[s] = __builtin_bit_cast(bf16x8, q_hi[qp]);
                    pmid[s] = __builtin_bit_cast(bf16x8, q_hi[CPL + qp]);
                    pl[s] = __builtin_bit_cast(bf16x8, q_hi[2 * CPL + qp]);
                };
                fetch(0);
                fetch(1);
#pragma unroll
                for (int s = 0; s < K2S; ++s) {
                    if (s + 2 < K2S) fetch(s + 2);
                    __builtin_amdgcn_sched_barrier(0);
                    dmvs_split_step<1, true>(&ph[s], &pmid[s], &pl[s], w2h[s], w2m[s], w2l[s], &acc);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // D[row = pixel 4*kq + r][col = cout m]: 4 consecutive pixels of one (row, channel)
                const int oy = oy0 + 2 * (k - 2) + orow, ox = ox0 + i0 + 4 * kq;
                if (oy < Ho && ox < Wo) {
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(fmaf(acc[r], sc2, sh2), 0.0f);
                    float* dst = y + ((long)n * 16 + m) * oplane + (long)oy * Wo + ox;
                    if (vec) {
                        *reinterpret_cast<f32x4*>(dst) = v;
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (ox + r < Wo) dst[r] = v[r];
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" int dmvs_featurenet_stem3_f32(const float* x, const float* w0, const float* scale0, const float* shift0, const float* w1,
                                         const float* scale1, const float* shift1, const float* w2, const float* scale2, const float* shift2,
                                         float* y, int32_t N, int32_t H, int32_t W, int32_t tune, void* stream) {
    (void)tune;
    if (!x || !w0 || !w1 || !w2 || !y || N <= 0 || H <= 0 || W <= 0) return DMVS_EINVAL;
    if ((long)3 * H * W >= (1L << 31)) return DMVS_EINVAL;
    // even sizes (stride 2 over an even image), rows of whole 16-byte pieces on a 16-byte aligned tensor
    if ((H & 1) || (W & 3) || ((uintptr_t)x & 15)) return DMVS_EINVAL;
    const int nsx = (W / 2 + UC - 1) / UC, nsy = (H / 2 + UR - 1) / UR;
    const long nunits = (long)nsx * nsy * N;
    if (nunits >= (1L << 31)) return DMVS_EINVAL;
    // persistent workgroups: as many as are resident at once (61.1 KB of LDS: 2 per CU)
    static const int resident = dmvs_resident_workgroups(reinterpret_cast<const void*>(featurenet_stem3_kernel));
    const unsigned grid = (unsigned)(nunits < resident ? nunits : resident);
    hipLaunchKernelGGL(featurenet_stem3_kernel, dim3(grid), dim3(DMVS_BLOCK), 0, (hipStream_t)stream, x, w0, scale0, shift0, w1, scale1, shift1, w2,
                       scale2, shift2, y, N, H, W, nsx, nsy);
    return dmvs_launch_status();
}
