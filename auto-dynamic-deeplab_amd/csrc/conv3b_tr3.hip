// conv3b_tr3.hip — instantiations of conv3b_kernel with TWO-ROW tiles for the 3x3 convolutions at dilation <= 2 (conv3b.h; chosen by conv3.hip c3_layout).
#include "conv3b.h"

// (waves across channels, pixels per tile row): 64-pixel rows for the full-width launches, 32 for the half-width ones of 3-wave blocks
C3Variant c3b_variant_tr3(int wc, int rpx, int mode, int np) {
  if (wc == 2 && rpx == 64) return c3b_tile_variant<2, 3, false, 64, 2>(mode, np);
  if (wc == 3 && rpx == 64) return c3b_tile_variant<3, 3, false, 64, 2>(mode, np);
  if (wc == 4 && rpx == 64) return c3b_tile_variant<4, 3, false, 64, 2>(mode, np);
  if (wc == 5 && rpx == 64) return c3b_tile_variant<5, 3, false, 64, 2>(mode, np);
  if (wc == 3 && rpx == 32) return c3b_tile_variant<3, 3, false, 32, 2>(mode, np);
  return {};
}
C3B_DIAG_READER(c3b_diag_tr3)
