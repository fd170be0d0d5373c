// attn_fwd_wq's LDS image of one 64-key K or V tile (round 18): where a (key row, byte column) lives, which LDS-DMA
// piece and lane bring it there, and the lane bases and immediates of the fragment reads. Plain C++17 constexpr with no
// HIP in it, so a host compiler alone builds and tests it (tests/host/attn_wq_image_main.cpp); attn_wide.hip takes
// every offset from here.
//
// attn_fwd_m16's image pads every 256-B row to 288 B, so that row r starts 32 (r & 7) bytes into the 256-B bank window
// and the ds_read_b128 K reads and the ds_read_b64_tr_b16 V reads are conflict-free. A 1-KiB DMA piece of that image
// is 3.55 rows, an eighth of it padding no read touches, and a tile is 18 pieces. Here the padding sits between PIECES
// instead: a piece is four whole 256-B rows, pieces are 1056 = 1024 + 32 bytes apart, and piece p of a 32-row group
// holds the rows p, p + 8, p + 16, p + 24 of the group (a DMA lane has its own source address, and rows of a tile are a
// whole token apart in the fused QKV buffer anyway). Row r again starts 32 (r & 7) bytes into the bank window, a tile
// is 16 pieces with no padding lanes, and the image is 16 896 B instead of 18 432.
#pragma once

namespace cp25attn {
namespace wqimg {

constexpr int kRows = 64;              // keys of a tile
constexpr int kRowBytes = 256;         // head dim 128 x bf16
constexpr int kPieceBytes = 1024;      // one wave-instruction of the LDS-DMA: 64 lanes x 16 B
constexpr int kPieceStride = 1056;     // 1024 + 32: the next piece starts one 32-B step further into the bank window
constexpr int kPieces = 16;            // per image
constexpr int kGroupStride = 8 * kPieceStride;  // 8448: a 32-row group is 8 pieces
constexpr int kImage = 2 * kGroupStride;        // 16 896
constexpr int kWaves = 4;              // wave w moves the pieces w + 4 j
constexpr int kWaveStep = kWaves * kPieceStride;  // 4224: from a wave's piece j to its piece j + 1

// LDS byte of (key row, byte column) of a tile, relative to the image
constexpr int off(int row, int col) {
  return kGroupStride * (row >> 5) + kPieceStride * (row & 7) + kRowBytes * ((row & 31) >> 3) + col;
}

// ---- the DMA: piece P = 0..15 goes to image byte piece_dst(P); lane l brings 16 B of row piece_row(P, l) ----
constexpr int piece_dst(int P) { return kPieceStride * P; }
constexpr int piece_row(int P, int lane) { return 32 * (P >> 3) + (P & 7) + 8 * (lane >> 4); }
constexpr int piece_col(int lane) { return 16 * (lane & 15); }
// piece j = 0..3 of wave w
constexpr int wave_piece(int wave, int j) { return wave + kWaves * j; }
// and back: the piece and the lane that bring (row, 16-B chunk)
constexpr int piece_of(int row) { return 8 * (row >> 5) + (row & 7); }
constexpr int lane_of(int row, int chunk) { return 16 * ((row & 31) >> 3) + chunk; }

// ---- the fragment reads: one base per lane, everything else an immediate ----
// K fragment (ds_read_b128) of key block kb (rows 16 kb .. + 15), d step s: lane (c16, g) reads row 16 kb + c16,
// bytes 64 s + 16 g .. + 15
constexpr int k_lane_base(int lane) { return off(lane & 15, 16 * (lane >> 4)); }
constexpr int k_imm(int kb, int s) { return kGroupStride * (kb >> 1) + 2 * kRowBytes * (kb & 1) + 64 * s; }
// V^T fragment (two ds_read_b64_tr_b16) of key step ks (rows 32 ks .. + 31), half hf (16 rows), column block f
// (32 B): lane (c16, g) reads row 32 ks + 16 hf + 4 g + (c16 >> 2), bytes 32 f + 8 (c16 & 3) .. + 7
constexpr int v_lane_row(int lane) { return 4 * (lane >> 4) + ((lane & 15) >> 2); }
constexpr int v_lane_base(int lane) { return off(v_lane_row(lane), 8 * (lane & 3)); }
constexpr int v_imm(int ks, int hf, int f) { return kGroupStride * ks + 2 * kRowBytes * hf + 32 * f; }

// every immediate above is lane-uniform: base + immediate is the address of the row and column the lane wants
constexpr bool reads_consistent() {
  for (int lane = 0; lane < 64; ++lane) {
    for (int kb = 0; kb < 4; ++kb)
      for (int s = 0; s < 4; ++s)
        if (k_lane_base(lane) + k_imm(kb, s) != off(16 * kb + (lane & 15), 64 * s + 16 * (lane >> 4))) return false;
    for (int ks = 0; ks < 2; ++ks)
      for (int hf = 0; hf < 2; ++hf)
        for (int f = 0; f < 8; ++f)
          if (v_lane_base(lane) + v_imm(ks, hf, f) !=
              off(32 * ks + 16 * hf + v_lane_row(lane), 32 * f + 8 * (lane & 3)))
            return false;
  }
  return true;
}
// every piece lands inside the image, and lane l of piece P writes the 16 B the image wants at its row and column
constexpr bool pieces_consistent() {
  for (int P = 0; P < kPieces; ++P) {
    if (piece_dst(P) + kPieceBytes > kImage) return false;
    for (int lane = 0; lane < 64; ++lane) {
      const int row = piece_row(P, lane), col = piece_col(lane);
      if (row < 0 || row >= kRows || piece_of(row) != P || lane_of(row, col / 16) != lane) return false;
      if (off(row, col) != piece_dst(P) + 16 * lane) return false;
    }
  }
  return true;
}
static_assert(reads_consistent(), "the fragment reads' immediates are lane-uniform");
static_assert(pieces_consistent(), "16 pieces of 64 chunks tile the image");

}  // namespace wqimg
}  // namespace cp25attn
