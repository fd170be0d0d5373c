// Prints attn_fwd_wq's LDS image (csrc/attn_wq_image.h) as tables for tests/test_attn_wq_image_cpu.py, which checks
// them with a bank model of its own. A host program: the header has no HIP in it.
#include <cstdio>

#include "attn_wq_image.h"

int main() {
  using namespace cp25attn::wqimg;
  std::printf("image %d pieces %d piece_bytes %d rows %d row_bytes %d\n", kImage, kPieces, kPieceBytes, kRows,
              kRowBytes);
  for (int row = 0; row < kRows; ++row)
    for (int chunk = 0; chunk < kRowBytes / 16; ++chunk)
      std::printf("off %d %d %d %d %d\n", row, chunk, off(row, 16 * chunk), piece_of(row), lane_of(row, chunk));
  for (int P = 0; P < kPieces; ++P)
    for (int lane = 0; lane < 64; ++lane)
      std::printf("piece %d %d %d %d %d\n", P, lane, piece_row(P, lane), piece_col(lane), piece_dst(P) + 16 * lane);
  for (int w = 0; w < kWaves; ++w)
    for (int j = 0; j < 4; ++j) std::printf("wave %d %d %d %d\n", w, j, wave_piece(w, j), kPieceStride * w + kWaveStep * j);
  for (int lane = 0; lane < 64; ++lane) std::printf("base %d %d %d\n", lane, k_lane_base(lane), v_lane_base(lane));
  for (int kb = 0; kb < 4; ++kb)
    for (int s = 0; s < 4; ++s) std::printf("kimm %d %d %d\n", kb, s, k_imm(kb, s));
  for (int ks = 0; ks < 2; ++ks)
    for (int hf = 0; hf < 2; ++hf)
      for (int f = 0; f < 8; ++f) std::printf("vimm %d %d %d %d\n", ks, hf, f, v_imm(ks, hf, f));
  return 0;
}
