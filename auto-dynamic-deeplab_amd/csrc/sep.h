// The tile choice of one fused SepConv half, shared by the forward (sepf.hip) and the backward (sepb.hip).  sep_choose makes it from the shape alone; the
// launch, the rows queries, the batch key and prepare and addk_sep_*_config read it.  The planner pairs a fused forward with a fused backward (the forward
// writes the depthwise output the backward's weight gradient reads): one choice keeps the two on the same tiles.  Plain host C++ on include/addk.h alone.
#pragma once
#include <stdint.h>
#include "addk.h"

// the (KS, KG, KP, R) instantiations both kernels are built for: kernel size, 16-channel groups, pixel stride in LDS (floats), rows per wave
#define ADDK_SEP_VARIANTS(X) \
  X(3, 3, 40, 1) X(3, 3, 40, 2) X(5, 3, 40, 1) X(5, 3, 40, 2) \
  X(3, 3, 56, 1) X(3, 3, 56, 2) X(5, 3, 56, 1) X(5, 3, 56, 2) \
  X(3, 5, 72, 1) X(5, 5, 72, 1) X(3, 5, 88, 1) X(5, 5, 88, 1)

struct SepChoice {
  int ks, kg, kp, r;             // the variant
  int tiles_x, tiles_y, gx;      // (4r) x 16 pixel tiles, one workgroup each; gx is also the number of slab / workspace rows
};
inline bool sep_is(const SepChoice& c, int ks, int kg, int kp, int r) { return c.ks == ks && c.kg == kg && c.kp == kp && c.r == r; }
// batch key <-> variant (the key names the variant only: tiles are per launch)
inline int sep_key(const SepChoice& c) { return (c.ks << 16) | (c.kg << 12) | (c.kp << 4) | c.r; }
inline SepChoice sep_from_key(int key) { return SepChoice{(key >> 16) & 15, (key >> 12) & 15, (key >> 4) & 255, key & 15, 0, 0, 0}; }

// false: the fused kernels do not take this shape (K in {3, 5}, C == Cout a multiple of 4 in (32, 48] or (64, 80])
inline bool sep_choose(int N, int H, int W, int C, int Cout, int K, SepChoice& c) {
  if (!(K == 3 || K == 5) || N <= 0 || H <= 0 || W <= 0 || Cout != C || C % 4) return false;
  const int kg = (C + 15) / 16, tx = (W + 15) / 16;
  if (!(kg == 3 || kg == 5)) return false;
  int kp = C; while (kp % 16 != 8) kp += 4;
  // 80-channel tiles need 100-127 KB of LDS: one workgroup per CU.  That is fine while the launch has at most two rounds of them
  // (config 2: 256 workgroups at 64x128) and LOSES to the separate depthwise / pointwise launches beyond (F = 40, 80 channels at
  // 128x256 = 1024 workgroups: step 72.2 ms fused vs 66.5 ms unfused) — those shapes stay on the unfused kernels
  if (kg == 5 && (long)N * ((H + 3) / 4) * tx > 512) return false;
  // two rows per wave where that still gives the chip >= 1.5 workgroups per CU (the LDS patch of a KG = 5 tile is 56 KB at R = 1)
  const long blocks2 = (long)N * ((H + 7) / 8) * tx;
  const int r = (kg == 3 && blocks2 >= 384) ? 2 : 1, ty = (H + 4 * r - 1) / (4 * r);
  const SepChoice v{K, kg, kp, r, tx, ty, N * ty * tx};
  bool built = false;
#define ADDK_SEP_BUILT(KS_, KG_, KP_, R_) built = built || sep_is(v, KS_, KG_, KP_, R_);
  ADDK_SEP_VARIANTS(ADDK_SEP_BUILT)
#undef ADDK_SEP_BUILT
  if (built) c = v;
  return built;
}

// a source or sum term as both kernels read it: (a, b) both or neither (they load b wherever a is set), rows that hold their channels, and no resampled
// map (src.rs_hw is honoured by addk_conv_fwd alone: here the map would be read as a plain one of the wrong size)
inline bool sep_src_ok(const addk_src& s) { return (s.a == nullptr) == (s.b == nullptr) && s.ld >= s.C && s.rs_hw == 0; }

// the fast-path mask gates what the library RECOMMENDS (supported, addk_sep_bwd_rows, batch keys, cfg[0]), never a direct launch: include/addk.h
inline bool sep_recommended() { return (addk_get_fast_paths() & ADDK_FAST_PW) != 0; }

// cfg[8] of addk_sep_fwd_config / addk_sep_bwd_config (c: all zero for a shape the kernels do not take)
inline int sep_config(const SepChoice& c, bool fused, int key, int32_t* cfg) {
  cfg[0] = fused; cfg[1] = c.ks; cfg[2] = c.kg; cfg[3] = c.kp; cfg[4] = c.r; cfg[5] = cfg[6] = c.gx; cfg[7] = key;
  return ADDK_OK;
}
