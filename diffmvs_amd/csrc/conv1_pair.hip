// FeatureNet conv1.1 + conv1.2 (16 -> 16 -> 16 channels, 3x3, stride 1, pad 1, folded BN + ReLU each; reference models/module.py:368-371) in ONE
// kernel, both layers in split-bf16 arithmetic.  As two launches the 16-channel map between them is written and read back by its only reader
// (6 of the 12 GB the two launches move per 576-image headline step) and every 16 x 16 tile pays, per 8-channel chunk, a DMA wait, two barriers
// and the fp32 -> bf16-triple conversion of an 18 x 18 halo tile around 72 matrix instructions per wave.  Here the intermediate never leaves LDS:
//   * work unit = (image, strip of S = 80 output columns, segment of R = 64 output rows); persistent workgroups of 8 waves take units round-robin,
//     the grid comes from the occupancy query;
//   * inside a unit the workgroup marches DOWN the rows, two rows per step, with two LDS rings of bf16 triples
//     [plane hi / mid / lo][4 row slots][chunk of 8 channels][84 positions][8 channels] (slot = (image row + 4) & 3; input position q = column
//     X0 - 2 + q, mid position p = column X0 - 1 + p).  A ring holds exactly the four rows that two output rows read;
//   * the waves are SPECIALISED: waves 0-3 run conv1.1 and hold only its 72 weight registers (2 chunks x 3 tap groups x 3 planes x 16 bytes, taken
//     as they are from ops.split_weights()), waves 4-7 run conv1.2 one row pair behind and hold only conv1.2's.  Step j:
//       phase 1 (rings are read only)  waves 4-7 issue the 16-byte LDS-DMA pieces of input rows Y0 - 2 + 2j, + 1 into an fp32 staging buffer
//                                      [2 rows][16 channels][88 = the aligned cover of columns X0 - 2 .. X0 + 81]: they land under the MFMAs
//                                      waves 0-3: mid rows Y0 + 2j - 5, - 4 (12 groups of 16 positions: 3 per wave) -> accumulators
//                                      waves 4-7: output rows Y0 + 2j - 8, - 7 (10 groups: 3, 3, 2, 2) -> accumulators
//       barrier (DMVS_DMA_BARRIER: it publishes the staged rows)
//       phase 2 (rings are written)    waves 0-3: BN + ReLU on the accumulators, ZERO outside the image (conv1.2's padding is zero, not
//                                      relu(bn1(conv(padding)))), dmvs_split3_bf16x8, into the mid ring over the rows conv1.2 finished with
//                                      waves 4-7: BN + ReLU, 16-byte NCHW stores (behind the barrier: its vector-memory wait never waits for
//                                      a store); then the staged rows -> dmvs_split3_bf16x8, ONCE per input element -> input ring
//       barrier (LDS only: the stores stay in flight)
//     LDS: 2 x 32,256 (rings) + 11,264 (staging) = 75,776 bytes, two workgroups = 16 waves per CU, 4 per SIMD at <= 128 registers;
//     (first form: the input through registers, 8 4-byte loads per lane held across phase 1 -- 16 more registers in waves 4-7, spilled weight quads
//     reloaded from scratch inside phase 1, whose vector-memory waits then also waited for the loads: 5.8 ms per 576 images against 3.3 for this one)
//   * steps 0-3 of a unit are the warm-up: they stage the input rows and recompute the mid row above the segment with the same instructions on
//     the same operands as the segment above -- every value depends only on its position in the image, not on N, the grid or the unit split;
//   * per output accumulator the matrix instructions are those of conv2d_mfma_kernel's split form (conv2d_tiled.h, the lean NCHW instantiation), in
//     its order and orientation: chunk outermost, tap group g (taps 4g .. 4g+3, slots beyond tap 8 read tap 8's operand against zero weights), the
//     six partial products lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi, pixels as the first operand (D[pixel 4*kq + r][cout m]); the epilogue is its
//     acc * scale + shift, max(., 0).  conv1.1's epilogue splits the fp32 values it would have stored, so the triples are what conv1.2's conversion
//     pass builds from them: the result is the two launches' bit for bit.
// Costs of the unit shape.  Matrix work: a mid row is 82 positions in 6 groups of 16, an output row 80 in 5: 11 groups for 10.125 useful, 8.6 % padding
// (S = 64: 9 for 8.125, 10.8 %; S = 160: 21 for 20.125 but 127 KB of rings per workgroup).  Rows: a 64-row segment computes 65.. 66 mid rows (+ 2.3 % of conv1.1) and
// runs 36 steps of which the first two only load and the last two only finish conv1.2; 576 x 4 x 4 = 9216 units over 512 resident workgroups are 18
// each, no tail.  (R = 128 halves the warm-up but leaves 9 units per workgroup; R = 256 leaves 4.5: a 10 % tail.)

#include "dmvs_common.h"
#include "dmvs_ring.h"
#include "dmvs_lds_poison.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));

constexpr int PB = 512;                     // threads per workgroup: waves 0-3 conv1.1, waves 4-7 conv1.2
constexpr int US = 80, UR = 64;             // a unit's output columns / rows
constexpr int NP = US + 4;                  // ring positions per row: input columns X0 - 2 .. X0 + 81 (mid: X0 - 1 .. X0 + 80 in positions 0 .. 81)
typedef dmvs_ring<2, NP> Ring;              // two chunks of 8 channels: 32,256 bytes
constexpr int PLQ = Ring::PLQ, RINGQ = Ring::RINGQ;
constexpr int NLOAD = 2 * 2 * NP;           // conversion items of a step: (row of the pair, chunk, position)
constexpr int SW = US + 8;                  // fp32 staging row: the 16-byte aligned cover of columns X0 - 2 .. X0 + 81 = columns X0 - 4 .. X0 + 83
constexpr int STAGEF = 2 * 16 * SW;         // staging buffer [2 rows][16 channels][88]: 704 16-byte pieces, 11,264 bytes
constexpr int NPIECE = STAGEF / 4;

// (DMVS_OPAQUE at the top of every step: left alone hipcc hoists every lane-dependent address of the step -- staging pieces, conversion items,
// operand positions -- out of the step loop, keeps them all live and spills)

__global__ void __launch_bounds__(PB) __attribute__((amdgpu_waves_per_eu(4, 4)))      // two workgroups per CU (LDS): at most 128 registers
featurenet_conv1_pair_kernel(const float* __restrict__ x, const u32x4s* __restrict__ ws1, const float* __restrict__ scale1,
                             const float* __restrict__ shift1, const u32x4s* __restrict__ ws2, const float* __restrict__ scale2,
                             const float* __restrict__ shift2, float* __restrict__ y, int N, int H, int W, int nsx, int nsy) {
    // ONE LDS object (stem.hip): the input ring, the mid ring, the fp32 staging buffer: 75,776 bytes
    __shared__ __attribute__((aligned(16))) float lds[2 * RINGQ * 4 + STAGEF];
    DMVS_LDS_POISON(lds);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, kq = lane >> 4;
    const int role = wave >> 2, wr = wave & 3;          // 0: conv1.1 (input ring -> mid ring), 1: conv1.2 (mid ring -> y)
    const long plane = (long)H * W;
    const int iplane = H * W;
    const int nunits = nsx * nsy * N;

    // this wave's layer: the lane's pre-split weights [chunk][tap group][plane] for (tap slot kq, cout m), its BN scale / shift
    const u32x4s* const wsp = role ? ws2 : ws1;
    u32x4s wq[2][3][3];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) wq[c][g][pl] = wsp[(((c * 3 + g) * 3 + pl) * 4 + kq) * 16 + m];
    const float* const scp = role ? scale2 : scale1;
    const float* const shp = role ? shift2 : shift1;
    const float sc = scp ? scp[m] : 1.0f, sh = shp ? shp[m] : 0.0f;
    int taps = 0;       // (ky | kx << 2) of tap group g in bits 4g .. 4g + 3: dmvs_ring::operand
#pragma unroll
    for (int g = 0; g < 3; ++g) taps |= dmvs_tap_slot<3, 3, 2>(g, kq) << (4 * g);
    const u32x4s* const src = reinterpret_cast<const u32x4s*>(lds) + role * RINGQ;      // the ring this wave's layer reads
    u32x4s* const in_q = reinterpret_cast<u32x4s*>(lds);
    uint16_t* const mid_h = reinterpret_cast<uint16_t*>(lds) + RINGQ * 8;
    float* const stage = lds + 2 * RINGQ * 4;
    const int pmax = role ? US - 1 : US + 1;    // last position of a row of this layer

    const int tb = tid - PB / 2;       // lane index among the conv1.2 waves: they stage and convert the input
    int lm = m, ltb = tb;              // (redefined opaquely per step)

    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const dmvs_unit u(unit, nsx, nsy, US, UR, H);
        const int n = u.n, X0 = u.X0, Y0 = u.Y0, Yend = u.Yend;
        const int nsteps = ((Yend - Y0 + 2) >> 1) + 4;
        const float* const xb = x + (long)n * 16 * plane;
        float* const yb = y + (long)n * 16 * plane;
        // rows this wave's layer computes: mid rows Y0 - 1 .. Yend + 1 inside the image (outside it they are written as zeros), output rows Y0 .. Yend
        const int row_lo = role ? Y0 : max(Y0 - 1, 0), row_hi = role ? Yend : min(Yend + 1, H - 1);
        // positions of a row this layer needs in the image's last, partial strip: groups wholly beyond them are skipped
        const int wlim = min(US, W - X0) + (role ? 0 : 2);
        // one 16-position group of this wave's layer: row `row`, positions 16 * cg .. + 15 (clamped to the row's last one) -> D[pixel 4*kq + r][cout m]
        auto conv_group = [&](int row, int cg) -> f32x4 {
            const int p = min(cg * 16 + lm, pmax);
            // The operand reads of the next tap group are issued, fenced, as this group's MFMAs free their registers: lo after the first MFMA, mid after
            // the fourth, hi (live to the sixth) into a second quad -- 16 operand registers.  (Left alone the scheduler reuses one quad per plane and waits
            // out the LDS latency twice per tap group; all three planes double-buffered are 24 registers, and the kernel spills.)
            bf16x8 ph[2], pm, pl;
            auto qp_of = [&](int s) { return Ring::operand(s, taps, row, p); };
            {
                const int qp = qp_of(0);
                pl = __builtin_bit_cast(bf16x8, src[2 * PLQ + qp]);
                ph[0] = __builtin_bit_cast(bf16x8, src[qp]);
                pm = __builtin_bit_cast(bf16x8, src[PLQ + qp]);
            }
            f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const int b = s & 1, c = s / 3, g = s - c * 3;
                const int qn = s + 1 < 6 ? qp_of(s + 1) : 0;
                const bf16x8 wh = __builtin_bit_cast(bf16x8, wq[c][g][0]), wm = __builtin_bit_cast(bf16x8, wq[c][g][1]),
                             wl = __builtin_bit_cast(bf16x8, wq[c][g][2]);
                __builtin_amdgcn_sched_barrier(0);
                a = dmvs_mfma_bf16(pl, wh, a);      // the six partial products in the order of dmvs_split_step (dmvs_bf16.h)
                __builtin_amdgcn_sched_barrier(0);
                if (s + 1 < 6) pl = __builtin_bit_cast(bf16x8, src[2 * PLQ + qn]);
                __builtin_amdgcn_sched_barrier(0);
                a = dmvs_mfma_bf16(ph[b], wl, a);
                a = dmvs_mfma_bf16(pm, wm, a);
                a = dmvs_mfma_bf16(pm, wh, a);
                __builtin_amdgcn_sched_barrier(0);
                if (s + 1 < 6) {
                    ph[b ^ 1] = __builtin_bit_cast(bf16x8, src[qn]);
                    pm = __builtin_bit_cast(bf16x8, src[PLQ + qn]);
                }
                __builtin_amdgcn_sched_barrier(0);
                a = dmvs_mfma_bf16(ph[b], wm, a);
                a = dmvs_mfma_bf16(ph[b], wh, a);
                __builtin_amdgcn_sched_barrier(0);
            }
            return a;
        };
        // (the two roles are two code paths with their own barriers: what one keeps across a barrier -- three accumulators there, sixteen loaded
        // values here -- does not occupy registers in the other)
        if (role) {
            for (int j = 0; j < nsteps; ++j) {
                // ---- phase 1: input rows Y0 - 2 + 2j, + 1 start streaming into the staging buffer (16-byte LDS-DMA pieces: piece = (row, channel,
                // 4 columns), wholly inside or outside the image because W % 4 == 0), then output rows Y0 + 2j - 8, - 7 into accumulators
                const int lrow0 = Y0 - 2 + 2 * j;
                DMVS_OPAQUE(lm);
                DMVS_OPAQUE(ltb);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (k * (PB / 2) + wr * 64 < NPIECE)       // (wave-uniform: 704 pieces = 11 waves' worth)
                        dmvs_stage_piece<2, 16, SW>(xb, iplane, H, W, lrow0, X0 - 4, lrow0 + (k * (PB / 2) + ltb) / (NPIECE / 2) <= Yend + 2,
                                                    k * (PB / 2) + ltb, stage + (k * (PB / 2) + wr * 64) * 4);
                }
                const int rowbase = Y0 + 2 * j - 8;
                f32x4 acc[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int gi = wr + 4 * i;
                    const int rr = gi >= 5 ? 1 : 0, cg = gi - rr * 5;
                    const int row = rowbase + rr;
                    acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (gi < 10 && cg * 16 < wlim && row >= row_lo && row <= row_hi) acc[i] = conv_group(row, cg);       // (wave-uniform)
                }
                DMVS_DMA_BARRIER();     // the staged rows have landed; everyone is done reading the ring rows phase 2 overwrites
                // ---- phase 2: the stores (4 consecutive pixels of one (row, channel): 16 bytes, W % 4 == 0; behind the barrier, so that its
                // vector-memory wait never waits for a store), then the staged rows as bf16 triples into the input ring, once per element
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int gi = wr + 4 * i;
                    const int rr = gi >= 5 ? 1 : 0, cg = gi - rr * 5;
                    const int row = rowbase + rr;
                    const int x0 = cg * 16 + 4 * kq, col = X0 + x0;
                    if (gi < 10 && row >= row_lo && row <= row_hi && x0 < US && col < W) {
                        f32x4 v;
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[i][r] * sc + sh, 0.0f);
                        *reinterpret_cast<f32x4*>(yb + (m * iplane + row * W + col)) = v;
                    }
                }
                auto convert_item = [&](bool need, int li, int lc, int lq) {
                    const int lrow = lrow0 + li;
                    if (need && lrow <= Yend + 2) {
                        const float* sp = stage + (li * 16 + lc * 8) * SW + lq + 2;
                        float v[8];
#pragma unroll
                        for (int c8 = 0; c8 < 8; ++c8) v[c8] = sp[c8 * SW];
                        bf16x8 h8, m8, l8;
                        dmvs_split3_bf16x8(v, h8, m8, l8);
                        u32x4s* const d = in_q + Ring::index(lrow, lc, lq);
                        d[0] = __builtin_bit_cast(u32x4s, h8);
                        d[PLQ] = __builtin_bit_cast(u32x4s, m8);
                        d[2 * PLQ] = __builtin_bit_cast(u32x4s, l8);
                    }
                };
                // item 0 = lane tb (all 256 lanes), item 1 = 256 + tb = (row 1, chunk 1, position tb + 4) (lanes tb < 80)
                DMVS_OPAQUE(ltb);
                const int li0 = ltb / (2 * NP), lrem = ltb - li0 * (2 * NP);
                const int lc0 = lrem / NP;
                convert_item(true, li0, lc0, lrem - lc0 * NP);
                convert_item(ltb + PB / 2 < NLOAD, 1, 1, ltb + PB / 2 - 3 * NP);
                DMVS_LDS_BARRIER();     // both rings hold the next step's rows, the staging buffer is free (ds accesses only)
            }
        } else {
            for (int j = 0; j < nsteps; ++j) {
                // ---- phase 1: mid rows Y0 + 2j - 5, - 4 into accumulators
                DMVS_OPAQUE(lm);
                const int rowbase = Y0 + 2 * j - 5;
                f32x4 acc[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int gi = wr * 3 + i;
                    const int rr = gi >= 6 ? 1 : 0, cg = gi - rr * 6;
                    const int row = rowbase + rr;
                    acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (cg * 16 < wlim && row >= row_lo && row <= row_hi) acc[i] = conv_group(row, cg);       // (wave-uniform)
                }
                DMVS_DMA_BARRIER();     // (the same barrier as the conv1.2 waves': these waves have no vector-memory operation in flight)
                // ---- phase 2: BN + ReLU, zero outside the image, as bf16 triples into the mid ring
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int gi = wr * 3 + i;
                    const int rr = gi >= 6 ? 1 : 0, cg = gi - rr * 6;
                    const int row = rowbase + rr;
                    if (row >= Y0 - 1 && row <= Yend + 1 && cg * 16 < wlim) {
                        const int p0 = cg * 16 + 4 * kq;
                        const bool rin = row >= 0 && row < H;
                        float v[8];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int col = X0 - 1 + p0 + r;
                            const bool inside = rin && col >= 0 && col < W;
                            v[r] = inside ? fmaxf(acc[i][r] * sc + sh, 0.0f) : 0.0f;
                            v[4 + r] = 0.0f;
                        }
                        bf16x8 h8, m8, l8;
                        dmvs_split3_bf16x8(v, h8, m8, l8);
                        uint16_t* const d = mid_h + Ring::index(row, m >> 3, p0) * 8 + (m & 7);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (p0 + r < US + 2) {
                                d[r * 8] = (uint16_t)h8[r];
                                d[PLQ * 8 + r * 8] = (uint16_t)m8[r];
                                d[2 * PLQ * 8 + r * 8] = (uint16_t)l8[r];
                            }
                        }
                    }
                }
                DMVS_LDS_BARRIER();
            }
        }
    }
}

}  // namespace

extern "C" int dmvs_featurenet_conv1_pair_f32(const float* x, const void* wsplit1, const float* scale1, const float* shift1, const void* wsplit2,
                                              const float* scale2, const float* shift2, float* y, int32_t N, int32_t H, int32_t W, int32_t tune,
                                              void* stream) {
    if (!x || !wsplit1 || !wsplit2 || !y || N <= 0 || H <= 0 || W <= 0) return DMVS_EINVAL;
    if ((long)16 * H * W >= (1L << 31)) return DMVS_EINVAL;
    // rows of whole 16-byte pieces on 16-byte aligned tensors (the output's 16-byte stores, the weights' 16-byte loads)
    if ((W & 3) || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)wsplit1 | (uintptr_t)wsplit2) & 15)) return DMVS_EINVAL;
    const int nsx = (W + US - 1) / US, nsy = (H + UR - 1) / UR;
    const long nunits = (long)nsx * nsy * N;
    if (nunits >= (1L << 31)) return DMVS_EINVAL;
    // persistent workgroups: as many as are resident at once; tune & 0xffff forces the grid (tests: results do not depend on it)
    static const int resident = dmvs_resident_workgroups(reinterpret_cast<const void*>(featurenet_conv1_pair_kernel), PB);
    hipLaunchKernelGGL(featurenet_conv1_pair_kernel, dim3(dmvs_persistent_grid(tune, resident, nunits)), dim3(PB), 0, (hipStream_t)stream, x,
                       reinterpret_cast<const u32x4s*>(wsplit1), scale1, shift1, reinterpret_cast<const u32x4s*>(wsplit2), scale2, shift2, y, N, H, W,
                       nsx, nsy);
    return dmvs_launch_status();
}
