// Fused BACKWARD of a SepConv half (reference modeling/operations.py:51-53 / :55-57, autograd of  y = pw(dw(relu(a x + b)))):
//   dt = W_pw^T dy                      (data gradient of the pointwise 1x1: fp32 matrix cores)
//   dz = dw_flipped * dt                (data gradient of the depthwise KS x KS)
//   dW_dw[c][tap] = sum_p dt[o(p, tap)] z[p],   (dA, dB) = sum_p (m dz x, m dz),   dx (+)= a m dz      (m = ReLU mask)
// in ONE launch over the same 2-D tiles as the forward kernel (sepf.hip).  Round 2 ran two launches (pw data gradient 23-60 us,
// depthwise backward 25-38 us per level batch) with the 10 MB gradient dt written and re-read in between: 6.5 ms of the 37 ms
// step.  Here dt never leaves the chip:
//   * stage 1: the workgroup computes dt on its haloed patch [(4R+KS-1)][16+KS-1] — every wave walks 16-pixel groups of the
//     patch, loads dy straight into the MFMA B fragment (lane (li, kq): pixel li, channels 16g + 4kq .. +3), the transposed
//     pointwise weights wait in LDS as ready A fragments — and drops the result into the LDS patch [pixel][KP] whose stride
//     KP = 8 (mod 16) makes the tap reads of stage 2 conflict-free (sepf.hip);
//   * stage 2: lane (li, kq) owns R input pixels x 4 channels of group g: per kernel row it reads KS shifted dt quads, feeds dz
//     and the KS weight-gradient products, and reduces the latter over the 16 pixel lanes with four DPP row adds per value, all 4 * KS
//     values of the kernel row in one interleaved block (fixed order: bit-reproducible); the fp64 (dA, dB) sums of an item take the same
//     tree by DPP moves; the four row bands' partials meet in LDS, one row [C][KS*KS] of the weight-gradient workspace and one row
//     [C][2] of the (dA, dB) slab per workgroup.
// The pointwise WEIGHT gradient stays with the batched register-streaming kernel (wgrad.hip), which reads dy and the stored
// depthwise output.
#include <stdlib.h>
#include "common.h"
#include "sep.h"

namespace {

struct SepbK {
  const float* dy; int lddy;
  addk_src src; int N, H, W, C;
  const float* dww; const float* pww; int ldw;
  float* g; int ldg; int accumulate;
  double* dab; float* ws;
  int tiles_x, tiles_y, gx;
};

__device__ __forceinline__ float4 fma4b(float4 w, float4 v, float4 a) {
  return make_float4(fmaf(w.x, v.x, a.x), fmaf(w.y, v.y, a.y), fmaf(w.z, v.z, a.z), fmaf(w.w, v.w, a.w));
}
// the same four FMAs as two explicit 2-vectors: the weight-gradient products end in the scalar operands of the reduction block below,
// which the SLP vectoriser takes as a reason to leave their FMAs scalar; written as vectors they stay v_pk_fma_f32
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct F4pk { f32x2 lo, hi; };
__device__ __forceinline__ F4pk fma4pk(float4 w, float4 v, F4pk a) {
  a.lo = __builtin_elementwise_fma((f32x2){w.x, w.y}, (f32x2){v.x, v.y}, a.lo);
  a.hi = __builtin_elementwise_fma((f32x2){w.z, w.w}, (f32x2){v.z, v.w}, a.hi);
  return a;
}
// Sums over the 16 lanes of a DPP row (= the 16 pixel lanes li of one channel quad) of all 4 * KS products of a kernel row at once, the same
// value in every lane, in the fixed tree (((x0+x1)+(x2+x3)) + ((x4+x5)+(x6+x7))) + (((x8+x9)+(x10+x11)) + ((x12+x13)+(x14+x15))): four levels
// (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror), each ONE v_add_f32_dpp per value.  Written per component with
// __builtin_amdgcn_update_dpp, the SLP vectoriser pairs the adds into v_pk_add_f32, which cannot carry the DPP control: every level then
// costs v_mov_b32_dpp x2 + v_pk_add_f32 + hazard no-ops, 6 VALU per value per tree where 4 suffice.
// Hazards: a DPP read of a VGPR that the VALU wrote needs two wait states and the compiler's hazard recogniser does not look inside inline
// assembly, so the spacing holds by construction: ONE asm statement, level by level over the 12 or 20 independent chains, so an add reads
// what the instruction 12 / 20 places before it wrote; the only no-op inside is the `s_nop 1` that opens the block, for the FMA that may
// have written the first operands just before it (in front of an asm statement the compiler may add its own fixed one-state pad, an
// `s_nop 0`: two no-ops per kernel row at the most, where the per-component form had 10-22).  volatile: the block is cross-lane and must
// stay where every lane of the row is active.
// an empty statement that the values pass through: what computes them stays above it, so the patch quads die before the reduction block
__device__ __forceinline__ void pin4(F4pk& v) { asm volatile("" : "+v"(v.lo), "+v"(v.hi)); }
#define SEPB_DPP(i, ctl) "v_add_f32_dpp %" #i ", %" #i ", %" #i " " ctl " row_mask:0xf bank_mask:0xf\n\t"
#define SEPB_LVL12(ctl) SEPB_DPP(0, ctl) SEPB_DPP(1, ctl) SEPB_DPP(2, ctl) SEPB_DPP(3, ctl) SEPB_DPP(4, ctl) SEPB_DPP(5, ctl) \
  SEPB_DPP(6, ctl) SEPB_DPP(7, ctl) SEPB_DPP(8, ctl) SEPB_DPP(9, ctl) SEPB_DPP(10, ctl) SEPB_DPP(11, ctl)
#define SEPB_LVL20(ctl) SEPB_LVL12(ctl) SEPB_DPP(12, ctl) SEPB_DPP(13, ctl) SEPB_DPP(14, ctl) SEPB_DPP(15, ctl) SEPB_DPP(16, ctl) \
  SEPB_DPP(17, ctl) SEPB_DPP(18, ctl) SEPB_DPP(19, ctl)
#define SEPB_TREE(LVL) "s_nop 1\n\t" LVL("quad_perm:[1,0,3,2]") LVL("quad_perm:[2,3,0,1]") LVL("row_half_mirror") LVL("row_mirror")
#define SEPB_V4(d) "+v"((d).x), "+v"((d).y), "+v"((d).z), "+v"((d).w)
__device__ __forceinline__ void row_sum16_taps(float4 (&d)[3]) {
  asm volatile(SEPB_TREE(SEPB_LVL12) : SEPB_V4(d[0]), SEPB_V4(d[1]), SEPB_V4(d[2]));
}
__device__ __forceinline__ void row_sum16_taps(float4 (&d)[5]) {
  asm volatile(SEPB_TREE(SEPB_LVL20) : SEPB_V4(d[0]), SEPB_V4(d[1]), SEPB_V4(d[2]), SEPB_V4(d[3]), SEPB_V4(d[4]));
}
#undef SEPB_V4
#undef SEPB_TREE
#undef SEPB_LVL20
#undef SEPB_LVL12
#undef SEPB_DPP

// One level of the same tree for the fp64 (dA, dB) sums: v + (v of the partner lane), the partner's two halves fetched by DPP moves (DPP on
// 64-bit arithmetic is limited to row_newbcast on this ISA); no LDS round trip, unlike __shfl_xor on a double.  Plain builtins: the compiler
// keeps the hazard spacing of these itself.
template <int CTL>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTL, 0xF, 0xF, true);
  return v + __hiloint2double(hi, lo);
}
template <int N>
__device__ __forceinline__ void row_sum16_f64(double (&s)[N]) {      // all N chains level by level: N independent adds in flight
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = dpp_add_f64<0xB1>(s[i]);         // quad_perm [1,0,3,2]
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = dpp_add_f64<0x4E>(s[i]);         // quad_perm [2,3,0,1]
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = dpp_add_f64<0x141>(s[i]);        // row_half_mirror
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = dpp_add_f64<0x140>(s[i]);        // row_mirror
}

// waves per workgroup.  Stage 1 hands the 16-pixel tiles of the patch and stage 2 the 4 * KG (row band, channel group) items round-robin to
// NW waves; the arithmetic of a tile / an item does not depend on which wave runs it.  A tile is one workgroup and the grid is one or two
// workgroups per CU (sep.h), so NW sets the waves per SIMD: 16 waves for the 80-channel tiles (one workgroup per CU), 8 for the 40-channel
// tiles config 2 runs (two per CU), all 4 waves per SIMD within 128 VGPRs; the 40-channel 5x5 at R = 1 (not run by config 2, not
// measured) stays at 4 waves.
template <int KS, int KG, int R>
struct SepbWaves { static constexpr int NW = KG == 5 ? 16 : (KS == 3 || R == 2) ? 8 : 4, WPS = NW == 4 ? 2 : 4; };

template <int KS, int KG, int KP, int R>
struct SepbGeo {
  static constexpr int NW = SepbWaves<KS, KG, R>::NW, NTHR = 64 * NW, WPS = SepbWaves<KS, KG, R>::WPS;   // waves, threads, waves per SIMD the launch bounds ask for
  static constexpr int CT = KG, PH = 4 * R + KS - 1, PW = 16 + KS - 1, NPIX = PH * PW, KQ = KP / 4, NT16 = (NPIX + 15) / 16;
  static constexpr int PATCH = NT16 * 16 * KP + 8;
  static constexpr int DWL = KS * KS * KG * 16, PWL = KG * CT * 64 * 4;
  static constexpr int DWS = 4 * KS * KS * KG * 16;                // per-row-band weight-gradient partials [4][KS*KS][KG*16]
  static constexpr int RED = 4 * KG * 16 * 2 * 2;                  // floats: [4][KG*16][2] doubles
  static constexpr size_t LDS = (size_t)(PATCH + DWL + PWL + DWS + RED) * 4;
};

template <int KS, int KG, int KP, int R>
__device__ __forceinline__ void sepb_body(const SepbK& p, float* sm) {
  typedef SepbGeo<KS, KG, KP, R> G;
  constexpr int CT = G::CT, PW = G::PW, NPIX = G::NPIX, KQ = G::KQ, HK = KS / 2, NT = KS * KS;
  float* patch = sm;
  float* dwl = patch + G::PATCH;                 // [NT][KG*16] tap weights, FLIPPED: dwl[f] = w[NT-1-f]
  float* pwl = dwl + G::DWL;                     // [KG][CT][64] float4: A fragments of W^T
  float* dws = pwl + G::PWL;                     // [4][NT][KG*16]
  double* red = reinterpret_cast<double*>(dws + G::DWS);
  constexpr int NW = G::NW, NTHR = G::NTHR;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), li = lane & 15, kq = lane >> 4;
  const int C = p.C;
  int b = blockIdx.x;
  const int tx = b % p.tiles_x; b /= p.tiles_x;
  const int ty = b % p.tiles_y; const int n = b / p.tiles_y;
  const int ih0 = ty * (4 * R), iw0 = tx * 16;

  // ---- [r4] the first stage-1 tile's dy quads are requested before anything else: they travel while the weights are staged ----
  auto dy_geom = [&](int j, const float*& dp, bool& ok) {
    const int pix = 16 * j + li;
    const int pr = pix / PW, pc = pix - pr * PW;
    const int oh = ih0 - HK + pr, ow = iw0 - HK + pc;
    ok = j < G::NT16 && pix < NPIX && (unsigned)oh < (unsigned)p.H && (unsigned)ow < (unsigned)p.W;
    dp = p.dy + (ok ? ((long)(n * p.H + oh) * p.W + ow) * p.lddy : 0);
  };
  auto dy_load = [&](int j, float4 (&d)[KG]) {
    const float* dp; bool ok;
    dy_geom(j, dp, ok);
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      const int k = 16 * g + 4 * kq;
      d[g] = ld4(dp + ((ok && k < C) ? k : 0));
    }
  };
  float4 dcur[KG], dnxt[KG];
  dy_load(wave, dcur);
  __builtin_amdgcn_sched_barrier(0);
  // ---- weights -> LDS (the tap table's channels beyond C are zeroed by threads that write no weight there: no barrier in between) ----
  for (int i = t; i < NT * (KG * 16 - C); i += NTHR) {
    const int tp = i / (KG * 16 - C), c = C + i - tp * (KG * 16 - C);
    dwl[tp * (KG * 16) + c] = 0.f;
  }
  for (int i = t; i < C * NT; i += NTHR) {
    const int c = i / NT, tp = i - c * NT;
    dwl[(NT - 1 - tp) * (KG * 16) + c] = ((const gfloat*)p.dww)[i];
  }
  for (int s = t; s < KG * CT * 64; s += NTHR) {          // A[row = ci = 16 i + (ln & 15)][k = co = 16 g + 4 (ln >> 4) + e] = W[co][ci]
    const int g = s / (CT * 64), rem = s - g * (CT * 64), i = rem >> 6, ln = rem & 63;
    const int ci = i * 16 + (ln & 15), co = 16 * g + 4 * (ln >> 4);
    const bool ok = ci < C && co < C;
    const gfloat* wp = (const gfloat*)(p.pww + (ok ? (long)co * p.ldw + ci : 0));
    const long st = ok ? p.ldw : 0;
    float4 v = make_float4(wp[0], wp[st], wp[2 * st], wp[3 * st]);
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
    lds_st4(pwl + s * 4, v);
  }
  if (KQ > C / 4) {                                      // zero the padding quads of every patch pixel (never written by stage 1)
    for (int i = t; i < G::NT16 * 16 * (KQ - C / 4); i += NTHR) {
      const int px = i / (KQ - C / 4), q = C / 4 + i - px * (KQ - C / 4);
      lds_st4(patch + px * KP + 4 * q, zero4());
    }
  }
  if (t < 8) patch[G::NT16 * 16 * KP + t] = 0.f;
  __syncthreads();

  // ---- stage 1: dt = W^T dy on the haloed patch, 16 pixels at a time ----
  for (int j = wave; j < G::NT16; j += NW) {
    const int pix = 16 * j + li;
    const float* dp; bool ok;
    dy_geom(j, dp, ok);
    dy_load(j + NW, dnxt);                                  // the next tile of this wave: in flight under this tile's matrix work (masked beyond the patch)
    float4 d[KG];
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      const int k = 16 * g + 4 * kq;
      const bool okk = ok && k < C;
      float4 v = dcur[g];
      v.x = okk ? v.x : 0.f; v.y = okk ? v.y : 0.f; v.z = okk ? v.z : 0.f; v.w = okk ? v.w : 0.f;
      d[g] = v;
      dcur[g] = dnxt[g];
    }
    f32x4 acc[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      float4 wf[CT];
#pragma unroll
      for (int i = 0; i < CT; ++i) wf[i] = lds_ld4(pwl + ((g * CT + i) * 64 + lane) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < CT; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(get4(wf[i], e), get4(d[g], e), acc[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < CT; ++i) {
      const int q = 4 * i + kq;                          // lane holds channels 16 i + 4 kq + {0..3} of pixel `pix`
      if (q < KQ) lds_st4(patch + pix * KP + 4 * q, make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
    }
  }
  __syncthreads();

  // ---- stage 2: depthwise backward; a work item is (row band rb: input rows [rb*R, rb*R + R) x 16 pixels, channel group g), item 4 g + rb
  // goes to wave (4 g + rb) % NW: NW is a multiple of 4, so a wave keeps ONE band and walks the groups g = wave / 4, + NW / 4, ... ----
  const int rb = wave & 3;
  int pp[R]; bool pin[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int ih = ih0 + rb * R + r, iw = iw0 + li;
    pin[r] = ih < p.H && iw < p.W;
    pp[r] = (n * p.H + ih) * p.W + iw;
  }
  const bool relu = p.src.relu != 0;
  float* mydws = dws + rb * (NT * KG * 16);
  double (*rd)[KG * 16][2] = reinterpret_cast<double (*)[KG * 16][2]>(red);
  // real loops over the channel group and the kernel row: fully unrolled, hipcc hoists every LDS read of the 15 (group, row)
  // bodies to the top (234-256 VGPRs and scratch spills for KS = 5); one body at a time needs ~100
  // [r4] the input values of this wave's NEXT item and the gradient THIS item accumulates into are requested at the top of an item's body and
  // arrive under its LDS / VALU work: the loop used to open with a dependent round trip per group and close with another.  (The accumulate
  // operand is not read until the item's end, so it need not be asked for an item earlier: R quads fewer live across the kernel-row loop.)
  float4 xn[R];
  auto pre = [&](int g) {
    const int q = 4 * g + kq;
    const bool cok = g < KG && 4 * q < C;
#pragma unroll
    for (int r = 0; r < R; ++r) xn[r] = ld4(p.src.x + ((pin[r] && cok) ? (long)pp[r] * p.src.ld + 4 * q : 0));
  };
  pre(wave >> 2);
#pragma unroll 1
  for (int g = wave >> 2; g < KG; g += NW / 4) {       // a wave with no item (left) falls through to the barrier
    const int q = 4 * g + kq;
    const int qr = q < KQ ? q : q - 2;
    const bool cok = 4 * q < C;
    float4 av = make_float4(1.f, 1.f, 1.f, 1.f), bv = zero4();
    if (p.src.a && cok) { av = ld4(p.src.a + 4 * q); bv = ld4(p.src.b + 4 * q); }
    float4 x[R], z[R], oacc[R]; F4pk dz[R]; bool m[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      x[r] = xn[r];
      oacc[r] = zero4();
      if (p.g && p.accumulate) oacc[r] = ld4(p.g + ((pin[r] && cok) ? (long)pp[r] * p.ldg + 4 * q : 0));
    }
    pre(g + NW / 4);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool okx = pin[r] && cok;
      const float4 zp = fma4b(av, x[r], bv);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[r][e] = okx && (!relu || get4(zp, e) > 0.f);
      z[r] = make_float4(m[r][0] ? zp.x : 0.f, m[r][1] ? zp.y : 0.f, m[r][2] ? zp.z : 0.f, m[r][3] ? zp.w : 0.f);
      if (!relu) z[r] = make_float4(okx ? zp.x : 0.f, okx ? zp.y : 0.f, okx ? zp.z : 0.f, okx ? zp.w : 0.f);
      dz[r].lo = dz[r].hi = (f32x2){0.f, 0.f};
    }
    const float* pb = patch + ((rb * R) * PW + li) * KP + 4 * qr;
#pragma unroll 1
    for (int fr = 0; fr < KS; ++fr) {                    // flipped kernel row: patch row i = fr + r feeds input row r
      float4 wr[KS], dwa[KS]; F4pk dwp[KS];
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) { wr[dx] = lds_ld4(dwl + (fr * KS + dx) * (KG * 16) + 4 * q); dwp[dx].lo = dwp[dx].hi = (f32x2){0.f, 0.f}; }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
          const float4 v = lds_ld4(pb + ((fr + r) * PW + dx) * KP);
          dz[r] = fma4pk(wr[dx], v, dz[r]);
          dwp[dx] = fma4pk(v, z[r], dwp[dx]);
        }
#pragma unroll
      for (int r = 0; r < R; ++r) pin4(dz[r]);
#pragma unroll
      for (int dx = 0; dx < KS; ++dx) dwa[dx] = make_float4(dwp[dx].lo.x, dwp[dx].lo.y, dwp[dx].hi.x, dwp[dx].hi.y);
      row_sum16_taps(dwa);
      if (li == 0) {
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) lds_st4(mydws + (fr * KS + dx) * (KG * 16) + 4 * q, dwa[dx]);     // flipped tap index f = fr*KS + dx
      }
    }
    double sAB[8];                                       // sA[e] = sAB[2 e], sB[e] = sAB[2 e + 1]
#pragma unroll
    for (int e = 0; e < 8; ++e) sAB[e] = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 dzr = make_float4(dz[r].lo.x, dz[r].lo.y, dz[r].hi.x, dz[r].hi.y);
      float4 gm;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = m[r][e] ? get4(dzr, e) : 0.f;
        set4(gm, e, d);
        sAB[2 * e] += (double)d * (double)get4(x[r], e); sAB[2 * e + 1] += (double)d;
      }
      if (p.g && pin[r] && cok) {
        float4 gv = make_float4(gm.x * av.x, gm.y * av.y, gm.z * av.z, gm.w * av.w);
        float* gp = p.g + (long)pp[r] * p.ldg + 4 * q;
        if (p.accumulate) { const float4 o = oacc[r]; gv.x += o.x; gv.y += o.y; gv.z += o.z; gv.w += o.w; }
        st4(gp, gv);
      }
    }
    if (p.dab) {
      row_sum16_f64(sAB);
      if (li == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { rd[rb][4 * q + e][0] = sAB[2 * e]; rd[rb][4 * q + e][1] = sAB[2 * e + 1]; }
      }
    }
  }
  __syncthreads();
  // ---- one workspace row per workgroup: the four row bands in fixed order; the flipped tap index goes back to [c][tap] ----
  for (int i = t; i < C * NT; i += NTHR) {
    const int c = i / NT, tp = i - c * NT;
    const int o = (NT - 1 - tp) * (KG * 16) + c;
    const float s = (dws[o] + dws[NT * KG * 16 + o]) + (dws[2 * NT * KG * 16 + o] + dws[3 * NT * KG * 16 + o]);
    ((gfloat*)p.ws)[((long)blockIdx.x * C + c) * NT + tp] = s;
  }
  if (p.dab && t < C) {
    gdouble* o = (gdouble*)p.dab + ((long)blockIdx.x * C + t) * 2;
    o[0] = (rd[0][t][0] + rd[1][t][0]) + (rd[2][t][0] + rd[3][t][0]);
    o[1] = (rd[0][t][1] + rd[1][t][1]) + (rd[2][t][1] + rd[3][t][1]);
  }
}

template <int KS, int KG, int KP, int R>
__global__ void __launch_bounds__((SepbGeo<KS, KG, KP, R>::NTHR), (SepbGeo<KS, KG, KP, R>::WPS)) sepb_kernel(const SepbK p) {
  extern __shared__ __attribute__((aligned(16))) float sepb_sm[];
  sepb_body<KS, KG, KP, R>(p, sepb_sm);
}
template <int KS, int KG, int KP, int R>
__global__ void __launch_bounds__((SepbGeo<KS, KG, KP, R>::NTHR), (SepbGeo<KS, KG, KP, R>::WPS)) sepb_batch_kernel(const SepbK* __restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) float sepb_sm[];
  const SepbK p = tab[blockIdx.z];
  if ((int)blockIdx.x >= p.gx) return;
  sepb_body<KS, KG, KP, R>(p, sepb_sm);
}

// shapes the backward takes: sep_choose's, within 32-bit pixel indexing
bool sepb_choose(const addk_sep_bwd_args* a, SepChoice& c) {
  return a && sep_choose(a->N, a->H, a->W, a->src.C, a->Cout, a->K, c) && (long)a->N * a->H * a->W < (1L << 30);
}
// the arguments of a launch on the fused kernel; fills the choice
bool sepb_args_ok(const addk_sep_bwd_args* a, SepChoice& c) {
  if (!sepb_choose(a, c)) return false;
  const addk_src& s = a->src;
  if (!s.x || !src_vec_ok(s) || !sep_src_ok(s) || !a->dw_w || !a->pw_w || !a->dy || !a->ws) return false;
  if (!aligned16(a->dy) || a->lddy % 4 || a->lddy < a->Cout || a->ldw < s.C) return false;
  return !a->g || (aligned16(a->g) && a->ldg % 4 == 0 && a->ldg >= s.C);
}
// the kernel descriptor of checked arguments
SepbK sepb_desc(const addk_sep_bwd_args* a, const SepChoice& c) {
  SepbK k{};
  k.dy = a->dy; k.lddy = a->lddy; k.src = a->src; k.N = a->N; k.H = a->H; k.W = a->W; k.C = a->src.C;
  k.dww = a->dw_w; k.pww = a->pw_w; k.ldw = a->ldw; k.g = a->g; k.ldg = a->ldg; k.accumulate = a->accumulate;
  k.dab = (double*)a->dab; k.ws = a->ws;
  k.tiles_x = c.tiles_x; k.tiles_y = c.tiles_y; k.gx = c.gx;
  return k;
}

template <int KS, int KG, int KP, int R>
int sepb_go(bool batch, dim3 grid, hipStream_t st, const SepbK* one, const SepbK* tab) {
  typedef SepbGeo<KS, KG, KP, R> G;
  addk_dyn_lds<sepb_kernel<KS, KG, KP, R>>((int)G::LDS);
  addk_dyn_lds<sepb_batch_kernel<KS, KG, KP, R>>((int)G::LDS);
  if (batch) hipLaunchKernelGGL((sepb_batch_kernel<KS, KG, KP, R>), grid, dim3(G::NTHR), G::LDS, st, tab);
  else hipLaunchKernelGGL((sepb_kernel<KS, KG, KP, R>), grid, dim3(G::NTHR), G::LDS, st, *one);
  return addk_check_launch("sep_bwd");
}

int sepb_dispatch(const SepChoice& c, bool batch, dim3 grid, hipStream_t st, const SepbK* one, const SepbK* tab) {
#define ADDK_SEPB(KS_, KG_, KP_, R_) if (sep_is(c, KS_, KG_, KP_, R_)) return sepb_go<KS_, KG_, KP_, R_>(batch, grid, st, one, tab);
  ADDK_SEP_VARIANTS(ADDK_SEPB)
#undef ADDK_SEPB
  addk_set_error("sep_bwd: no instantiation");
  return ADDK_ERR_UNSUPPORTED;
}

}  // namespace

// rows of `ws` ([rows][C][K*K] floats) and `dab` ([rows][C][2] fp64) the launch writes: one per workgroup; 0: the library does not
// recommend the fused kernel for this shape.  Shape and mask only: the query comes before dy and the workspace exist.
extern "C" int addk_sep_bwd_rows(const addk_sep_bwd_args* a) { SepChoice c; return sep_recommended() && sepb_choose(a, c) ? c.gx : 0; }
extern "C" int addk_sep_bwd_batch_key(const addk_sep_bwd_args* a) { SepChoice c; return sep_recommended() && sepb_args_ok(a, c) ? sep_key(c) : -1; }
extern "C" int addk_sep_bwd_config(const addk_sep_bwd_args* a, int32_t* cfg) {
  ADDK_REQUIRE(a && cfg, "sep_bwd_config: null argument");
  SepChoice c{};
  sepb_choose(a, c);
  return sep_config(c, addk_sep_bwd_rows(a) > 0, addk_sep_bwd_batch_key(a), cfg);
}
extern "C" int addk_sep_bwd(const addk_sep_bwd_args* a, void* stream) {
  SepChoice c;
  ADDK_REQUIRE(sepb_args_ok(a, c), "sep_bwd: shape not covered (K in {3,5}, C == Cout in (32,48] or (64,80], aligned)");
  const SepbK k = sepb_desc(a, c);
  return sepb_dispatch(c, false, dim3(k.gx), (hipStream_t)stream, &k, nullptr);
}
extern "C" int64_t addk_sep_bwd_batch_prepare(const addk_sep_bwd_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta) {
  return batch_prepare<SepbK>("sep_bwd_batch_prepare", a, n, host_blob, blob_bytes, meta, [](const addk_sep_bwd_args* x, SepbK& k, BatchItem& b) {
    SepChoice c;
    if (!sepb_args_ok(x, c)) return false;
    k = sepb_desc(x, c); b = BatchItem{sep_key(c), c.gx, 1, 0};
    return true;
  });
}
extern "C" int addk_sep_bwd_batch_run(const void* dev_blob, const int64_t* meta, void* stream) {
  ADDK_REQUIRE(dev_blob && meta && meta[1] > 0 && meta[2] > 0, "sep_bwd_batch_run: bad args");
  return sepb_dispatch(sep_from_key((int)meta[0]), true, dim3((unsigned)meta[2], 1, (unsigned)meta[1]), (hipStream_t)stream, nullptr,
                       reinterpret_cast<const SepbK*>(dev_blob));
}
