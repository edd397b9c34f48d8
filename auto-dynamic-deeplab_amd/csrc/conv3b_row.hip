// conv3b_row.hip — instantiations of conv3b_kernel with ONE-ROW tiles (conv3b.h; chosen by conv3.hip c3_layout): the wide dilations of ASPP
// (3x3, d = 6 / 12 / 18: the rows of a tile pair share nothing), half- and quarter-width tiles of small maps, and the pointwise GEMM form (KS = 1).
#include "conv3b.h"

C3Variant c3b_variant_row(int wc, int ks, int bigd, int bpx, int mode, int np) {
  if (ks == 3 && bigd) {            // 3x3 at dilation > 2
    if (wc == 2 && bpx == C3_BP) return c3b_tile_variant<2, 3, true, C3_BP, 1>(mode, np);
    if (wc == 3 && bpx == C3_BP) return c3b_tile_variant<3, 3, true, C3_BP, 1>(mode, np);
    if (wc == 4 && bpx == C3_BP) return c3b_tile_variant<4, 3, true, C3_BP, 1>(mode, np);
    if (wc == 5 && bpx == C3_BP) return c3b_tile_variant<5, 3, true, C3_BP, 1>(mode, np);
    if (wc == 4 && bpx == 64) return c3b_tile_variant<4, 3, true, 64, 1>(mode, np);
  } else if (!bigd) {               // what the two-row tiles leave: half width on 4 waves, quarter width on 3; the 1x1
    if (wc == 4 && ks == 3 && bpx == 64) return c3b_tile_variant<4, 3, false, 64, 1>(mode, np);
    if (wc == 3 && ks == 3 && bpx == 32) return c3b_tile_variant<3, 3, false, 32, 1>(mode, np);
    if (wc == 3 && ks == 5 && bpx == 32) return c3b_tile_variant<3, 5, false, 32, 1>(mode, np);
    if (wc == 3 && ks == 1 && bpx == C3_BP) return c3b_tile_variant<3, 1, false, C3_BP, 1>(mode, np);
    if (wc == 4 && ks == 1 && bpx == C3_BP) return c3b_tile_variant<4, 1, false, C3_BP, 1>(mode, np);
    if (wc == 5 && ks == 1 && bpx == C3_BP) return c3b_tile_variant<5, 1, false, C3_BP, 1>(mode, np);
    if (wc == 4 && ks == 1 && bpx == 64) return c3b_tile_variant<4, 1, false, 64, 1>(mode, np);
  }
  return {};
}
C3B_DIAG_READER(c3b_diag_row)
