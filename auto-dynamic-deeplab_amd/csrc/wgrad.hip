// Weight gradient of the dense convolution for one source:
//     dW[co][tap][c] = sum_p dy[p, co] * Z[p @ tap, c],   Z = relu?(a*x+b) recomputed on the fly.
// GEMM with M = output channels, N = input channels of one tap and the reduction over pixels.
// A block owns one tile of output x input channels (and one or all taps) and one slice of the pixel range; the per-slice tiles go to a
// workspace that the reduce kernels here sum deterministically into dW.  This file: those reduce kernels and the host side — which kernel
// a convolution gets (wg_choose), its descriptor (wg_fill), the dispatch over the kernel families (wg_variant; the kernels themselves:
// wgrad_pix.hip, wgrad_h3.hip, wgrad_hk.hip, wgrad_rs.hip; shared device code: wgrad.h) and the C entry points.
#include <vector>
#include "wgrad.h"

namespace {

__global__ void wgrad_reduce_kernel(const float* ws, int splits, int Cout, int taps, int C, float* dw, int ldw,
                                    int cin_total, int w_choff, int accumulate) {
  long n = (long)Cout * taps * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;      // four independent chains keep the loads in flight
    int k = 0;
    for (; k + 3 < splits; k += 4) {
      s0 += ws[(long)k * n + i]; s1 += ws[(long)(k + 1) * n + i]; s2 += ws[(long)(k + 2) * n + i]; s3 += ws[(long)(k + 3) * n + i];
    }
    for (; k < splits; ++k) s0 += ws[(long)k * n + i];
    float s = (s0 + s1) + (s2 + s3);
    int c = (int)(i % C); long r = i / C; int tap = (int)(r % taps); int co = (int)(r / taps);
    float* d = dw + (long)co * ldw + (long)tap * cin_total + w_choff + c;
    *d = accumulate ? *d + s : s;
  }
}

// many slices, few elements: one wave per element, lanes stride over the slices, fixed-order butterfly
__global__ void __launch_bounds__(256) wgrad_reduce_wave_kernel(const float* ws, int splits, int Cout, int taps, int C, float* dw, int ldw,
                                                                int cin_total, int w_choff, int accumulate) {
  const long n = (long)Cout * taps * C;
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  float s = 0.f;
  for (int k = lane; k < splits; k += 64) s += ws[(long)k * n + i];
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0) {
    int c = (int)(i % C); long r = i / C; int tap = (int)(r % taps); int co = (int)(r / taps);
    float* d = dw + (long)co * ldw + (long)tap * cin_total + w_choff + c;
    *d = accumulate ? *d + s : s;
  }
}

// batched reduce: rwork[b] = (op, first element, mode): mode 1 = many slices, few elements: 64 consecutive elements x 4 slice
// groups per block (every load a coalesced 256-byte segment; fixed-order combine in LDS), 0 = thread per element
__global__ void __launch_bounds__(256) wgrad_reduce_batch_kernel(const WgK* __restrict__ ops, const int4* __restrict__ rwork) {
  __shared__ float part[4][64];
  const int4 wk = rwork[blockIdx.x];
  const WgK p = wg_desc<true>(ops[0], ops, __builtin_amdgcn_readfirstlane(wk.x));
  const int C = p.src.C;
  const gfloat* ws = (const gfloat*)p.ws;
  const long n = (long)p.Cout * p.taps * C;
  long i; float s;
  bool writer;
  if (wk.z) {
    const int e = threadIdx.x & 63, rg = threadIdx.x >> 6;
    i = (long)wk.y + e;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < n) {
      int k = rg;
      for (; k + 12 < p.splits; k += 16) {
        s0 += ws[(long)k * n + i]; s1 += ws[(long)(k + 4) * n + i]; s2 += ws[(long)(k + 8) * n + i]; s3 += ws[(long)(k + 12) * n + i];
      }
      for (; k < p.splits; k += 4) s0 += ws[(long)k * n + i];
    }
    part[rg][e] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    s = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
    writer = rg == 0 && i < n;
  } else {
    i = (long)wk.y + threadIdx.x;
    if (i >= n) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 3 < p.splits; k += 4) {
      s0 += ws[(long)k * n + i]; s1 += ws[(long)(k + 1) * n + i]; s2 += ws[(long)(k + 2) * n + i]; s3 += ws[(long)(k + 3) * n + i];
    }
    for (; k < p.splits; ++k) s0 += ws[(long)k * n + i];
    s = (s0 + s1) + (s2 + s3);
    writer = true;
  }
  if (writer) {
    int c = (int)(i % C); long r = i / C; int tap = (int)(r % p.taps); int co = (int)(r / p.taps);
    gfloat* d = (gfloat*)p.dw + (long)co * p.ldw + (long)tap * p.cin_total + p.w_choff + c;
    *d = p.accumulate ? *d + s : s;
  }
}

int pick_cty(int Cout) {
  const int cands[5] = {8, 5, 4, 3, 2};
  int best = 2; long bc = -1;
  for (int k = 0; k < 5; ++k) { long cols = (long)cdiv(Cout, 16 * cands[k]) * 16 * cands[k]; if (bc < 0 || cols < bc) { bc = cols; best = cands[k]; } }
  return best;
}
int pick_ctz(int C) {
  const int cands[4] = {5, 4, 3, 1};
  int best = 1; long bc = -1;
  for (int k = 0; k < 4; ++k) { long cols = (long)cdiv(C, 16 * cands[k]) * 16 * cands[k]; if (bc < 0 || cols < bc) { bc = cols; best = cands[k]; } }
  return best;
}
// The weight-gradient kernels.  The numbers are what addk_conv_wgrad_config returns in cfg[0] and a batch in meta[0].
enum WgKind : int {
  WG_PIX = 0,         // pixel-split kernel (wgrad_kernel)
  WG_OS_128x64 = 1,   // output-split 128x64 (wide heads)
  WG_OS_96x96 = 2,    // output-split 96x96 (80-channel cells)
  WG_OS_64x64 = 3,    // output-split 64x64 (64-channel stem)
  WG_H3 = 5,          // halo-patch kernel (3x3, stride 1, 'same' padding, wide): (64*NT co) x (16*NG c) tiles, the nine taps in the block
  WG_RS = 6,          // register-streaming kernel for the narrow cell convolutions
  WG_HK = 7,          // halo-patch kernel with the taps split across waves (the cells' dilated 3x3 / 5x5 convolutions)
  WG_ST = 8,          // few input channels (stem0): all taps x channels in two column tiles of one workgroup
  WG_H1 = 9,          // the split-precision halo-patch arithmetic for the wide 1x1 heads (wgrad_h1b_kernel)
};
int os_kind(int Cout, int C) {
  if (Cout >= 128 && Cout % 128 == 0 && C >= 48) return WG_OS_128x64;
  if (Cout > 64 && Cout <= 96 && C > 64 && C <= 96) return WG_OS_96x96;
  if (Cout > 48 && Cout <= 64 && C > 48 && C <= 64) return WG_OS_64x64;
  return WG_PIX;
}
void pick_tiles(int Cout, int C, int* cty, int* ctz) {
  *cty = pick_cty(Cout); *ctz = pick_ctz(C);
  if (*cty == 8 && *ctz == 5) *ctz = 4;   // 8x5 accumulator tiles would not leave room for the staging registers
  switch (os_kind(Cout, C)) {
    case WG_OS_128x64: *cty = 8; *ctz = 4; break;
    case WG_OS_96x96: *cty = 6; *ctz = 6; break;
    case WG_OS_64x64: *cty = 4; *ctz = 4; break;
    default: break;
  }
}
// blocks of one pixel slice of the pixel-split geometry (kinds 0-3)
inline int pix_tiles(int Cout, int C, int taps) { int cty, ctz; pick_tiles(Cout, C, &cty, &ctz); return cdiv(Cout, 16 * cty) * taps * cdiv(C, 16 * ctz); }
// terms of the split-precision weight-gradient kernels in precision mode `mode` for cty output-channel tiles per workgroup (0: the fp32
// kernels); tail_x3 (mode 3): the 128-channel blocks are the exit heads (decoder, ASPP) -> three terms; stem1's 64-channel blocks and the
// cells' convs keep six
inline int wg_np_of(int cty, int mode) { return mode == 2 ? 3 : mode == 1 ? 2 : mode == 3 ? (cty == 8 ? 2 : 3) : 0; }
bool h3_ok(const addk_conv_wgrad_args* a) {
  return (addk_get_fast_paths() & ADDK_FAST_WGRAD3) && a->KH == 3 && a->KW == 3 && a->stride == 1 && a->pad == a->dil && a->dil >= 1 && a->dil <= 18 &&
         a->OH == a->H && a->OW == a->W && a->W >= 64 && a->Cout % 64 == 0 && a->src.C >= 16 &&
         aligned16(a->dy) && a->lddy % 4 == 0 && src_vec_ok(a->src) && (long)a->N * a->H * a->W >= 8192;
}
// kind 9 runs in the split-precision modes only
bool h1_ok(const addk_conv_wgrad_args* a, int mode) {
  return (addk_get_fast_paths() & ADDK_FAST_WGRAD3) && a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad == 0 && a->OH == a->H && a->OW == a->W &&
         a->W >= 64 && a->Cout % 128 == 0 && a->src.C >= 64 && a->src.C % 4 == 0 && aligned16(a->dy) && a->lddy % 4 == 0 && src_vec_ok(a->src) &&
         (!a->src.a || (aligned16(a->src.a) && aligned16(a->src.b))) && (long)a->N * a->H * a->W >= 8192 && wg_np_of(8, mode);
}
bool rs_ok(const addk_conv_wgrad_args* a) {
  return (addk_get_fast_paths() & ADDK_FAST_WGRAD_RS) && a->Cout <= 160 && a->Cout >= 16 && a->src.C >= 16 && a->KH * a->KW <= 25 &&
         aligned16(a->dy) && a->lddy % 4 == 0 && a->Cout % 4 == 0 && src_vec_ok(a->src) && (long)a->N * a->OH * a->OW >= 4096;
}
// tile stride of an operand: 40-channel tiles (3-component layout) when the channel count is a multiple of 40 or fits 48,
// else up to 64 channels (4-component layout)
inline int rs_tile(int Cn) {
  if (Cn <= 48) return Cn;
  if (Cn % 40 == 0) return 40;
  if (Cn % 48 == 0) return 48;
  const int nt = cdiv(Cn, RS_T); return cdiv(cdiv(Cn, nt), 4) * 4;
}
inline int rs_lay(int tile) { return tile <= 48 ? 3 : 4; }
// output-channel tiles per block of kind 7: 3 for the 5x5 (7 taps per wave -> 21 accumulator tiles), up to 5 for the 3x3 (3 taps per wave)
inline int hk_ct(int Cout, int ks) { return (ks == 5 || Cout <= 48) ? 3 : 5; }
inline int hk_tiles(int Cout, int C, int ks) { return cdiv(Cout, 16 * hk_ct(Cout, ks)) * cdiv(C, 16); }
bool hk_ok(const addk_conv_wgrad_args* a) {
  return (addk_get_fast_paths() & ADDK_FAST_WGRAD_RS) && a->KH == a->KW && (a->KH == 3 || a->KH == 5) && a->stride == 1 &&
         a->dil >= 1 && a->dil <= 2 && a->pad == a->dil * (a->KH / 2) && a->OH == a->H && a->OW == a->W &&
         a->Cout >= 32 && a->Cout <= 160 && a->Cout % 4 == 0 && a->src.C >= 16 && a->OW >= 32 &&
         aligned16(a->dy) && a->lddy % 4 == 0 && src_vec_ok(a->src) && (long)a->N * a->H * a->W >= 4096;
}
bool st_ok(const addk_conv_wgrad_args* a) {
  return (addk_get_fast_paths() & ADDK_FAST_WGRAD_RS) && a->src.C <= 4 && a->KH * a->KW * a->src.C <= 32 && a->Cout <= 64 && a->Cout % 4 == 0 &&
         aligned16(a->dy) && a->lddy % 4 == 0 && (long)a->N * a->OH * a->OW >= 65536;
}
constexpr int ST_MAX_SPLITS = 1024;      // kind 8 slices the pixels only, into at most this many 1024-pixel slices
// input-channel tiles per workgroup of kind 5: 2 (512 threads sharing one staged dy tile) on the split-precision kernel when the channels fill
// whole pairs of tiles (a half-empty pair costs what the shared dy saves: 304 and 400 channels measured equal, 256 -7 %, stem1's 64 -> 64 -14 %)
inline int h3_ng(int Cout, int C, int mode) {
  // (re-measured with the split-fp16 arithmetic: the shared dy tile still wins, 2.2 vs 2.38 ms per step: profiles/r05_wgrad_h3b_f16_pipelined.txt)
  return (C % 32 == 0 && wg_np_of(Cout % 128 == 0 ? 8 : 4, mode)) ? 2 : 1;
}
inline int h3_tiles(int Cout, int C) { const int nt = Cout % 128 == 0 ? 2 : 1; return (Cout / (64 * nt)) * cdiv(C, 16); }
// at most 32 workspace slices, or as many as it takes for the op alone to offer one block per slot (few-tile convs: stem1)
inline int h3_max_splits(int tiles) { const int s = cdiv(768, tiles); return s > 32 ? s : 32; }
// `budget` = workgroups this conv should contribute.  A lone launch needs ~1536 of them to fill the chip even if that
// leaves a block a single 64-pixel step; inside a batch the other convs provide the parallelism, so each block gets
// >= 8 steps and the per-block epilogue (cross-wave combine + partial tile written to the workspace) is amortised.
int pick_splits(long P, int tiles, int budget = 1536, int min_steps = 1) {
  long maxs = cdiv(P, (long)min_steps * KP);
  long want = cdiv(budget, tiles);
  long s = want < maxs ? want : maxs;
  if (s < 1) s = 1;
  if (s > 1024) s = 1024;
  return (int)s;
}

// Everything decided for one weight gradient: the kernel, its geometry and how its pixel range is cut into slices.
struct WgChoice {
  int kind;             // WgKind
  int cty, ctz;         // with kind and the precision mode, the variant (wg_variant): kinds 0-3: 16-channel output / input tiles per block;
                        // 5: 4*NT and NG; 6: the lane layouts of dy and the activation; 7: CT and KS; 8: 4, 2; 9: 8, 4
  int nyt, nzt, tiles;  // output- / input-channel tiles and the blocks of one slice (times the taps for kinds 0-3 and 6)
  int vecY, vecZ;       // the descriptor's 16-byte load flags; kind 6: the operands' tile strides
  long nseg;            // kinds 5, 7, 9: the pixels are cut as 64-pixel row segments, a step count per block for the batch (h3_pick_steps)
  int slots;            //   resident blocks of the launch the step count is picked for
  int px_chunk;         // kinds 6, 8: the pixels are cut into slices of about this many (kinds 0-3: pick_splits' budget)
  int cap;              // kinds 5-9: the most slices, what addk_conv_wgrad_ws has sized the workspace for
};
// Halo-patch scheduling.  A block runs `steps` row segments; blocks are dispatched in grid order as CU slots free up
// (2 resident blocks per CU at NT=2, 3 at NT=1), so what matters is that the LAST round of blocks is nearly full:
// pick the segment count per block that minimises  ceil(blocks / slots) * (steps + start-up)  over the whole launch.
inline int h3_splits(long nseg, int steps, int tiles) {
  int sp = cdiv(nseg, steps);
  const int cap = h3_max_splits(tiles);
  if (sp > cap) sp = cap;
  return cdiv(nseg, cdiv(nseg, sp));
}
int h3_pick_steps(const WgChoice* ops, int n) {
  const long slots = ops[0].slots;
  int best = 64; double best_cost = -1.0;
  for (int steps = 8; steps <= 256; ++steps) {
    long blocks = 0; long longest = 0;
    for (int i = 0; i < n; ++i) {
      const int sp = h3_splits(ops[i].nseg, steps, ops[i].tiles);
      blocks += (long)ops[i].tiles * sp;
      const long ch = cdiv(ops[i].nseg, sp);
      if (ch > longest) longest = ch;
    }
    const double cost = (double)cdiv(blocks, slots) * ((double)longest + 1.5);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = steps; }
  }
  return best;
}

int wg_choose(const addk_conv_wgrad_args* a, int mode, WgChoice& c) {
  ADDK_REQUIRE(a && a->dy && a->src.x && a->dw, "conv_wgrad: null pointer");
  ADDK_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0 && a->Cout > 0 && a->src.C > 0, "conv_wgrad: empty shape");
  ADDK_REQUIRE(a->lddy >= a->Cout && a->src.ld >= a->src.C, "conv_wgrad: short stride");
  ADDK_REQUIRE(a->w_choff + a->src.C <= a->cin_total && a->ldw >= a->KH * a->KW * a->cin_total, "conv_wgrad: weight layout");
  ADDK_REQUIRE((a->src.a == nullptr) == (a->src.b == nullptr), "conv_wgrad: a/b must come together");
  ADDK_REQUIRE((long)a->N * a->OH * a->OW < (1L << 30) && (long)a->N * a->H * a->W < (1L << 30), "conv_wgrad: tensor too large for 32-bit pixel indexing");
  const int Cout = a->Cout, C = a->src.C, taps = a->KH * a->KW;
  const long P = (long)a->N * a->OH * a->OW, nseg = (long)a->N * a->OH * cdiv(a->OW, H3_KP);
  c = WgChoice{};
  c.kind = os_kind(Cout, C);
  pick_tiles(Cout, C, &c.cty, &c.ctz);
  c.nyt = cdiv(Cout, 16 * c.cty); c.nzt = cdiv(C, 16 * c.ctz); c.tiles = c.nyt * taps * c.nzt;
  c.vecY = aligned16(a->dy) && a->lddy % 4 == 0 && Cout % 4 == 0; c.vecZ = src_vec_ok(a->src);
  const int pix_cap = pick_splits(P, c.tiles);      // the slices of a lone pixel-split launch: every workspace holds them
  if (st_ok(a)) {
    c.kind = WG_ST; c.cty = 4; c.ctz = 2; c.nyt = c.nzt = c.tiles = 1;
    c.px_chunk = 1024; c.cap = ST_MAX_SPLITS;
  } else if (h3_ok(a)) {
    const int nt = Cout % 128 == 0 ? 2 : 1, ng = h3_ng(Cout, C, mode);
    c.kind = WG_H3; c.cty = 4 * nt; c.ctz = ng; c.nyt = Cout / (64 * nt); c.nzt = cdiv(C, 16 * ng);
    c.nseg = nseg; c.slots = ng == 2 ? 256 : nt == 2 ? 512 : 768; c.cap = h3_max_splits(h3_tiles(Cout, C));
  } else if (h1_ok(a, mode)) {      // 128 output x 64 input channels per workgroup
    c.kind = WG_H1; c.cty = 8; c.ctz = 4; c.nyt = Cout / 128; c.nzt = cdiv(C, 16 * H1_TP);
    c.nseg = nseg; c.slots = 512; c.cap = pix_cap;
  } else if (hk_ok(a)) {
    const int ct = hk_ct(Cout, a->KH);
    c.kind = WG_HK; c.cty = ct; c.ctz = a->KH; c.nyt = cdiv(Cout, 16 * ct); c.nzt = cdiv(C, 16);
    c.nseg = nseg; c.slots = ct == 3 ? 768 : 512; c.cap = h3_max_splits(c.nyt * c.nzt);
  } else if (rs_ok(a)) {      // <= 64-channel tiles, 2048-pixel slices (128 k-steps per wave)
    c.kind = WG_RS; c.vecY = rs_tile(Cout); c.vecZ = rs_tile(C); c.cty = rs_lay(c.vecY); c.ctz = rs_lay(c.vecZ);
    c.nyt = cdiv(Cout, c.vecY); c.nzt = cdiv(C, c.vecZ); c.tiles = c.nyt * taps * c.nzt;
    c.px_chunk = 2048; c.cap = pix_cap;
  }
  if (c.nseg) c.tiles = c.nyt * c.nzt;
  return 0;
}

// The kernel of a launch key (kind, cty, ctz) in precision mode `mode`.
// In the split-precision modes kinds 5, 7 and 9 run the split kernels (wgrad_h3b / hkb / h1b).  A batch is
// replayed in the mode current at run time: the geometries only the split kernels have (kind 9, kind 5 with NG = 2) fail in fp32.
int wg_variant(bool batch, int kind, int cty, int ctz, int mode, WgVariant& v) {
  const int np = wg_np_of(cty, mode);
  v = {nullptr, 256, 0};
  if ((kind == WG_H1 || (kind == WG_H3 && ctz == 2)) && !np) {
    addk_set_error("conv_wgrad: launch prepared for the split-precision kernel, but the precision mode changed since");
    return ADDK_ERR_INVALID;
  }
  switch (kind) {
    case WG_PIX: v = wg_variant_pix(batch, cty, ctz); break;
    case WG_OS_128x64: v = wg_variant_os(batch, 4); break;
    case WG_OS_96x96: v = wg_variant_os(batch, 3); break;
    case WG_OS_64x64: v = wg_variant_os(batch, 2); break;
    case WG_H3: v = wg_variant_h3(batch, cty, ctz, np); break;
    case WG_RS: v = wg_variant_rs(batch, cty, ctz, mode); break;
    case WG_HK: v = wg_variant_hk(batch, cty, ctz, np); break;
    case WG_ST: v = wg_variant_st(batch); break;
    case WG_H1: v = wg_variant_h1(batch, np); break;
    default: break;
  }
  if (!v.fn) { addk_set_error("conv_wgrad: no tile config"); return ADDK_ERR_UNSUPPORTED; }
  return 0;
}

// the workspace slices of a conv are summed by one wave per 64 weights when there are many of them, else by one block per 256
inline bool wg_wave_reduce(int splits, long n) { return splits > 16 && n <= 65536; }
}  // namespace

// The workspace bound, from the P / Cout / C / taps of a conv: the most slices of any kind its shape may get (the kinds' predicates
// need the full arguments; these are the shape parts of them, widened).  Plans size their buffers with it.
extern "C" int64_t addk_conv_wgrad_ws(int64_t P, int32_t Cout, int32_t C, int32_t taps) {
  int splits = pick_splits(P, pix_tiles(Cout, C, taps));      // kinds 0-3, and the cap of kinds 6 and 9
  auto at_least = [&](int s) { if (s > splits) splits = s; };
  if ((taps == 9 || taps == 25) && Cout >= 32 && Cout <= 160 && C >= 16) at_least(h3_max_splits(hk_tiles(Cout, C, taps == 9 ? 3 : 5)));   // kind 7
  if (taps == 9 && Cout % 64 == 0 && C >= 16) at_least(h3_max_splits(h3_tiles(Cout, C)));                                              // kind 5
  if (C <= 4 && taps * C <= 32 && Cout <= 64) at_least(ST_MAX_SPLITS);                                                                // kind 8
  return (int64_t)splits * Cout * taps * C;
}

// The descriptor of a weight gradient from its choice, with the pixel range cut into slices.  In a batch, `budget` and `min_steps` (kinds
// 0-3) and `h3_steps` (kinds 5, 7, 9: one step count for the whole batch) come from the batch.
static int wg_fill(const addk_conv_wgrad_args* a, const WgChoice& c, WgK& k, bool check_ws, int budget = 1536, int min_steps = 1, int h3_steps = 0) {
  k.dy = a->dy; k.lddy = a->lddy; k.Cout = a->Cout;
  k.N = a->N; k.H = a->H; k.W = a->W; k.OH = a->OH; k.OW = a->OW;
  k.KH = a->KH; k.KW = a->KW; k.stride = a->stride; k.pad = a->pad; k.dil = a->dil;
  k.src = a->src; k.ws = a->ws;
  k.taps = a->KH * a->KW; k.nyt = c.nyt; k.nzt = c.nzt;
  k.P = a->N * a->OH * a->OW;
  k.vecY = c.vecY; k.vecZ = c.vecZ;
  if (c.nseg) {      // 64-pixel row segments, h3_steps of them per block
    if (h3_steps <= 0) h3_steps = h3_pick_steps(&c, 1);
    int sp = cdiv(c.nseg, h3_steps); if (sp > c.cap) sp = c.cap;
    k.chunkP = cdiv(c.nseg, sp);
    k.splits = cdiv(c.nseg, k.chunkP);
  } else if (c.px_chunk) {      // slices of about px_chunk pixels, a multiple of 4
    int sp = cdiv(k.P, c.px_chunk); if (sp > c.cap) sp = c.cap;
    k.chunkP = cdiv(cdiv(k.P, sp), 4) * 4;
    k.splits = cdiv(k.P, k.chunkP);
  } else {      // `budget` blocks, slices of whole 64-pixel steps
    k.splits = pick_splits(k.P, c.tiles, budget, min_steps);
    k.chunkP = cdiv(cdiv(k.P, k.splits), KP) * KP;
  }
  ADDK_REQUIRE(!check_ws || a->ws, "conv_wgrad: null pointer");
  ADDK_REQUIRE(!check_ws || a->ws_floats >= (int64_t)k.splits * a->Cout * k.taps * a->src.C, "conv_wgrad: workspace too small");
  k.dw = a->dw; k.ldw = a->ldw; k.cin_total = a->cin_total; k.w_choff = a->w_choff; k.accumulate = a->accumulate;
  return 0;
}

static int wg_launch(int kind, int cty, int ctz, dim3 grid, hipStream_t st, const WgK& k, const WgK* ops, const int4* work) {
  WgVariant v;
  const int rc = wg_variant(ops != nullptr, kind, cty, ctz, addk_get_conv_precision(), v);
  if (rc) return rc;
  hipLaunchKernelGGL(v.fn, grid, dim3(v.threads), v.lds, st, k, ops, work);
  return addk_check_launch("conv_wgrad");
}
// The reduction of the workspace slices into dW: of the batch `ops` (rblocks entries of rwork), or of the lone conv `k`.
static int wg_reduce_launch(hipStream_t st, const WgK& k, const WgK* ops, const int4* rwork, unsigned rblocks) {
  if (ops) {
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(rblocks), dim3(256), 0, st, ops, rwork);
    return addk_check_launch("conv_wgrad_batch_reduce");
  }
  const long n = (long)k.Cout * k.taps * k.src.C;
  const bool wave = wg_wave_reduce(k.splits, n);
  int rb = cdiv(n, 256); if (rb > 2048) rb = 2048;
  hipLaunchKernelGGL(wave ? wgrad_reduce_wave_kernel : wgrad_reduce_kernel, dim3(wave ? cdiv(n, 4) : rb), dim3(256), 0, st, k.ws, k.splits, k.Cout, k.taps, k.src.C,
                     k.dw, k.ldw, k.cin_total, k.w_choff, k.accumulate);
  return addk_check_launch("conv_wgrad_reduce");
}

extern "C" int addk_conv_wgrad(const addk_conv_wgrad_args* a, void* stream) {
  WgChoice c; WgK k;
  int rc = wg_choose(a, addk_get_conv_precision(), c);
  if (!rc) rc = wg_fill(a, c, k, true);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = wg_launch(c.kind, c.cty, c.ctz, dim3(c.tiles, k.splits), st, k, nullptr, nullptr);
  if (rc) return rc;
  return wg_reduce_launch(st, k, nullptr, nullptr, 0);
}

// ---- batched weight gradients -------------------------------------------------------------------------------------
extern "C" int addk_conv_wgrad_config(const addk_conv_wgrad_args* a, int32_t* cfg) {
  WgChoice c; WgK k;
  int rc = wg_choose(a, addk_get_conv_precision(), c);
  if (!rc) rc = wg_fill(a, c, k, false);
  if (rc) return rc;
  cfg[0] = c.kind; cfg[1] = c.cty; cfg[2] = c.ctz; cfg[3] = c.tiles * k.splits;
  return 0;
}

extern "C" int64_t addk_conv_wgrad_batch_prepare(const addk_conv_wgrad_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta) {
  if (!a || n <= 0 || !meta) { addk_set_error("wgrad_batch_prepare: bad args"); return ADDK_ERR_INVALID; }
  const int mode = addk_get_conv_precision();
  std::vector<WgChoice> ch(n);
  for (int i = 0; i < n; ++i) {
    const int rc = wg_choose(&a[i], mode, ch[i]);
    if (rc) return rc;
    if (ch[i].kind != ch[0].kind || ch[i].cty != ch[0].cty || ch[i].ctz != ch[0].ctz) { addk_set_error("wgrad_batch_prepare: mixed tile configurations"); return ADDK_ERR_INVALID; }
  }
  int budget = 8192 / n; if (budget < 32) budget = 32; if (budget > 1536) budget = 1536;
  const int min_steps = n >= 4 ? 8 : 1;
  const int h3_steps = ch[0].nseg ? h3_pick_steps(ch.data(), n) : 0;
  std::vector<WgK> ops(n);
  long nblocks = 0, nrblocks = 0;
  for (int i = 0; i < n; ++i) {
    const int rc = wg_fill(&a[i], ch[i], ops[i], host_blob != nullptr, budget, min_steps, h3_steps);
    if (rc) return rc;
    nblocks += (long)ch[i].tiles * ops[i].splits;
    const long ne = (long)a[i].Cout * ops[i].taps * a[i].src.C;
    nrblocks += wg_wave_reduce(ops[i].splits, ne) ? cdiv(ne, 64) : cdiv(ne, 256);
  }
  const int64_t off_work = ((int64_t)n * sizeof(WgK) + 15) / 16 * 16;
  const int64_t off_rwork = off_work + nblocks * (int64_t)sizeof(int4);
  const int64_t total = off_rwork + nrblocks * (int64_t)sizeof(int4);
  meta[0] = ch[0].kind; meta[1] = ch[0].cty; meta[2] = ch[0].ctz; meta[3] = n; meta[4] = off_work; meta[5] = nblocks; meta[6] = off_rwork; meta[7] = nrblocks;
  if (!host_blob) return total;
  if (blob_bytes < total) { addk_set_error("wgrad_batch_prepare: blob too small"); return ADDK_ERR_INVALID; }
  memcpy(host_blob, ops.data(), (size_t)n * sizeof(WgK));
  int4* work = reinterpret_cast<int4*>(reinterpret_cast<char*>(host_blob) + off_work);
  int4* rwork = reinterpret_cast<int4*>(reinterpret_cast<char*>(host_blob) + off_rwork);
  long b = 0, rb = 0;
  for (int i = 0; i < n; ++i) {
    const int tiles = ch[i].tiles, sp = ops[i].splits;
    if (ch[i].kind == WG_RS) {
      // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs, so within a group of 8 pixel chunks the tiles
      // (taps x channel blocks) of one chunk are placed 8 apart: they share an XCD and its L2 serves the 9/25 re-reads
      // of that chunk's dy / activation rows.
      for (int g0 = 0; g0 < sp; g0 += 8) {
        const int gn = sp - g0 < 8 ? sp - g0 : 8;
        for (int x = 0; x < tiles; ++x)
          for (int yy = 0; yy < gn; ++yy) work[b++] = make_int4(i, x, g0 + yy, 0);
      }
    } else
    for (int y = 0; y < sp; ++y)
      for (int x = 0; x < tiles; ++x) work[b++] = make_int4(i, x, y, 0);
    const long ne = (long)a[i].Cout * ops[i].taps * a[i].src.C;
    if (wg_wave_reduce(sp, ne)) { for (long e = 0; e < ne; e += 64) rwork[rb++] = make_int4(i, (int)e, 1, 0); }
    else { for (long e = 0; e < ne; e += 256) rwork[rb++] = make_int4(i, (int)e, 0, 0); }
  }
  return total;
}

extern "C" int addk_conv_wgrad_batch_run(const void* dev_blob, const int64_t* meta, void* stream) {
  ADDK_REQUIRE(dev_blob && meta && meta[3] > 0 && meta[5] > 0 && meta[7] > 0, "wgrad_batch_run: bad args");
  const WgK* ops = reinterpret_cast<const WgK*>(dev_blob);
  const int4* work = reinterpret_cast<const int4*>(reinterpret_cast<const char*>(dev_blob) + meta[4]);
  const int4* rwork = reinterpret_cast<const int4*>(reinterpret_cast<const char*>(dev_blob) + meta[6]);
  hipStream_t st = (hipStream_t)stream;
  WgK dummy{};
  int rc = wg_launch((int)meta[0], (int)meta[1], (int)meta[2], dim3((unsigned)meta[5], 1), st, dummy, ops, work);
  if (rc) return rc;
  return wg_reduce_launch(st, dummy, ops, rwork, (unsigned)meta[7]);
}
