// Pieces shared by the fused FeatureNet kernels (stem.hip, stem3.hip, conv1_pair.hip, fpn_tail.hip): persistent workgroups that take
// (image, strip, segment) work units round-robin and march down a unit's rows over LDS rings of bf16 triples, in split-bf16 arithmetic
// (dmvs_bf16.h: the order of the six partial products, the epilogue's triple store).  Everything is forced inline.  A helper is used in a kernel
// only where the kernel's registers, scratch, occupancy and LDS (hipcc -Rpass-analysis=kernel-resource-usage) stay what they were.  Kept local:
//   * conv1_pair.hip's conv_group interleaves its operand reads with the six matrix instructions (128 VGPRs, 68 bytes of scratch: no slack);
//   * fpn_tail.hip's c3 stager (one row per call): through dmvs_stage_piece the kernel spills 16 instead of 10 SGPRs;
//   * the 3x3 kernels pack their three tap slots into one register themselves (a packing FUNCTION cost conv1_pair 20 bytes of scratch);
//   * the "4 pixels of one (row, channel)" store of stem.hip / stem3.hip: as a function it cost stem.hip two VGPRs;
//   * conv1_pair.hip's mid-ring writer stores 2-byte elements of transposed accumulators, not 8-byte halves: no dmvs_store_split4.
#pragma once
#include "dmvs_bf16.h"

// Work unit `unit` of nsx strips x nsy segments x N images, strips fastest: a strip is US columns, a segment UR rows of the H-row image
// the unit is counted in.  The unit covers columns X0 .. X0 + US - 1 (the last strip may be partial) and rows Y0 .. Yend.
struct dmvs_unit {
    int sx, sy, n, X0, Y0, Yend;
    __device__ __forceinline__ dmvs_unit(int unit, int nsx, int nsy, int US, int UR, int H) {
        sx = unit % nsx;
        const int uq = unit / nsx;
        sy = uq % nsy;
        n = uq / nsy;
        X0 = US * sx;
        Y0 = UR * sy;
        Yend = min(Y0 + UR, H) - 1;
    }
};

// The tap of a lane's k-slots in tap group g of a KH x KW kernel, as ky | kx << SH (a field of SH bits per coordinate): a bf16 MFMA step spans
// 4 taps x 8 channels, lane quarter kq = lane >> 4 holds tap slot 4g + kq.  Slots beyond the kernel read the LAST tap's operand against zero weights.
template <int KH, int KW, int SH = 4> __device__ __forceinline__ int dmvs_tap_slot(int g, int kq) {
    const int t = min(4 * g + kq, KH * KW - 1);
    return (t / KW) | ((t % KW) << SH);
}

// A ring of bf16 triples [plane hi / mid / lo][4 row slots][NCH chunks of 8 channels][NP positions][8 channels], in 16-byte entries (the 8
// channels of one position: a lane's k-slots of one MFMA step).  Image row r lives in slot (r + 4) & 3 (rows from -4 on): the ring holds
// exactly the four rows that two output rows of a 3x3 layer read.
template <int NCH, int NP> struct dmvs_ring {
    static constexpr int SLOTS = 4;
    static constexpr int PLQ = SLOTS * NCH * NP;        // entries of one plane
    static constexpr int RINGQ = 3 * PLQ;               // entries of the ring
    static __device__ __forceinline__ int slot(int row) { return (row + 4) & 3; }
    static __device__ __forceinline__ int index(int row, int chunk, int pos) { return (slot(row) * NCH + chunk) * NP + pos; }
    // the operand entry of step s = (chunk s / 3, tap group s % 3) of a 3x3 layer for output (row, pos): source row row - 1 + ky, position
    // pos + kx (positions count from the column left of the output's first); taps = dmvs_tap_slot<3, 3, 2>(g, kq) of group g in bits 4g .. 4g + 3
    static __device__ __forceinline__ int operand(int s, int taps, int row, int pos) {
        const int c = s / 3, g = s - c * 3;
        const int tg = taps >> (4 * g);
        const int sl = (row + 3 + (tg & 3)) & 3;        // slot(row - 1 + ky)
        return (sl * NCH + c) * NP + pos + ((tg >> 2) & 3);
    }
};

// Rows of an NCHW fp32 tensor into an LDS buffer [ROWS][C][RW] by 16-byte LDS-DMA: piece e = (row, channel, 4 columns) of rows row0 .. row0 +
// ROWS - 1, columns col0 .. col0 + RW - 1 of the H x W image at `img` (W % 4 == 0 and col0 % 4 == 0: a piece lies wholly inside or outside).  A piece
// outside the image, or one the caller rules out (!wanted), reads the zero source.  The 64 pieces of a wave are contiguous in the buffer: dstp = the
// wave's first piece (wave-uniform); the caller issues pieces k T + lane for k = 0, 1, ... and skips the waves beyond the last piece.
template <int ROWS, int C, int RW>
__device__ __forceinline__ void dmvs_stage_piece(const float* img, int plane, int H, int W, int row0, int col0, bool wanted, int e, float* dstp) {
    constexpr int PER_ROW = C * RW / 4;
    const int li = ROWS == 1 ? 0 : e / PER_ROW, rem = e - li * PER_ROW;
    const int ch = rem / (RW / 4), pc = rem - ch * (RW / 4);
    const int row = row0 + li, col = col0 + 4 * pc;
    const bool ok = wanted && row >= 0 && row < H && col >= 0 && col < W;
    const float* srcp = ok ? img + (ch * plane + row * W + col) : dmvs_zero16;
    __builtin_amdgcn_global_load_lds(srcp, DMVS_LDS_PTR(dstp), 16, 0, 0);
}

// conv0.1 of the stem (8 -> 8, 3x3) on ROW PAIRS: cout = 8 would leave half of the 16 matrix rows empty, so row m = (output row of the pair
// m >> 3, cout m & 7) and K = 8 input channels x 12 (input row j = 0..3, kx) slots = 3 bf16 MFMA steps; rows 0-7 take tap row ky = j, rows 8-15
// ky = j - 1, the rest zero weights.  The lane's paired weights of slot 4g + kq (dmvs_tap_slot<4, 3>) as bf16 triples.
__device__ __forceinline__ void dmvs_conv01_paired_weights(const float* w1, int m, int kq, bf16x8 (&wh)[3], bf16x8 (&wm)[3], bf16x8 (&wl)[3]) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int sl = 4 * g + kq;
        const int j = sl / 3, kx = sl - j * 3;
        const int ky = m < 8 ? j : j - 1;
        float wv[8];
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) wv[ci] = (ky >= 0 && ky <= 2) ? w1[(ci * 9 + ky * 3 + kx) * 8 + (m & 7)] : 0.0f;
        dmvs_split3_bf16x8(wv, wh[g], wm[g], wl[g]);
    }
}
