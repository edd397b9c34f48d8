// wgrad_rs.hip — the register-streaming weight-gradient kernel of the narrow cell convolutions, fp32 and split-fp16 (wgrad.h; choice and
// launch: wgrad.hip).
#include "wgrad.h"

namespace {

// Register-streaming weight gradient for the narrow cell convolutions (Cout, C <= 160; 1x1, dilated k x k, strided):
// no LDS staging and no barrier in the main loop.  A wave walks its own pixel range four pixels per MFMA k-step; lane
// (li, kq) loads its slice of dy (pixel kq) and of the activation (tap-shifted pixel kq) straight from global memory and
// uses the COMPONENTS of those vector loads as MFMA operands.  Two lane layouts per operand:
//   LAY 4: one float4 at channel 4*li        -> 4 operand tiles, tile e holds channels {4r+e}           (<= 64 channels)
//   LAY 3: one float2 at channel 2*li + one float at channel 32+li -> 3 tiles {2r}, {2r+1}, {32+r}      (<= 48 channels)
// so a 40-channel conv issues 3x3 MFMAs per k-step (83 % useful rows) instead of 4x4 (62 %).  Every load is unconditional
// (masked lanes read a safe address and are zeroed) and RS_U k-steps are in flight per wave.  The LDS-staged kernels
// above ran these launches at 23 TF/s, bound by their barrier/latency chains.
// the same fragment from lane offsets the caller has clamped already (l0: the vector element, l1: the lone third element of LAY 3), unmasked
template <int LAY>
__device__ __forceinline__ RsFrag<LAY> rs_load_at(const float* b, int l0, int l1) {
  RsFrag<LAY> f;
  if (LAY == 4) { const float4 x = ld4(b + l0); f.v[0] = x.x; f.v[1] = x.y; f.v[2] = x.z; f.v[3 % LAY] = x.w; }
  else {
    typedef float rs_f32x2 __attribute__((ext_vector_type(2)));
    const rs_f32x2 x = *(const __attribute__((address_space(1))) rs_f32x2*)(b + l0);
    f.v[0] = x.x; f.v[1] = x.y; f.v[2] = ((const gfloat*)b)[l1];
  }
  return f;
}
// channel (relative to the tile origin) held by component e, row/column index R of the MFMA tile
template <int LAY> __device__ __forceinline__ int rs_chan(int e, int R) { return LAY == 4 ? 4 * R + e : (e < 2 ? 2 * R + e : 32 + R); }

// [r5] F16 = the split-fp16 arithmetic (common.h) in the same register-streaming form: a batch of RS_U = 4 k-steps (16 pixels per wave) becomes ONE k-step of
// v_mfma_f32_16x16x16_f16 — the lane that loaded pixel 4 u + kq in k-step u supplies it as k-slot 4 kq + u of both operands (any bijection of the contraction
// index serves as long as the two operands agree) — so the loads are exactly the fp32 form's and 36 fp32 matrix instructions (1152 pipe cycles per 16 pixels)
// become 27 fp16 ones (432).  Every WAVE keeps its own running scales for dy and for the activation (it owns its accumulators until the fixed-order combine at
// the end): per batch the wave's largest magnitudes by four DPP steps and readlanes, the accumulators rescaled when a scale drops, unscaled before the combine.
typedef _Float16 wg_f16x4 __attribute__((ext_vector_type(4)));
template <int LA, int LB, bool BATCH, bool F16 = false>
__global__ void __launch_bounds__(256, 2) wgrad_rs_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  static_assert(!F16 || RS_U == 4, "one fp16 k-step = four pixel quads");
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  __shared__ float tile[RS_T][RS_T + 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  int bx = blk_x;
  const int zt = bx % p.nzt; bx /= p.nzt;
  const int tap = bx % p.taps; const int yt = bx / p.taps;
  const int kh = tap / p.KW, kw = tap - kh * p.KW;
  const int tsy = p.vecY, tsz = p.vecZ;        // tile strides in channels (multiples of 4), set by the host for this kind
  const int co0 = yt * tsy, c0 = zt * tsz;
  const int ncy = min(tsy, p.Cout - co0), ncz = min(tsz, p.src.C - c0);
  const bool y4 = 4 * li < ncy, y2 = 2 * li < min(ncy, 32), y1 = 32 + li < ncy;
  const bool z4 = 4 * li < ncz, z2 = 2 * li < min(ncz, 32), z1 = 32 + li < ncz;
  const int C = p.src.C;
  const int pbeg = blk_y * p.chunkP;
  int pend = pbeg + p.chunkP; if (pend > p.P) pend = p.P;
  const int span = (pend - pbeg + 3) / 4;                  // k-steps of the block
  const int per_wave = (span + 3) / 4;
  const int s_beg = wave * per_wave, s_end = min(span, s_beg + per_wave);
  RsFrag<LB> za, zb;
#pragma unroll
  for (int f = 0; f < LB; ++f) { za.v[f] = 1.f; zb.v[f] = 0.f; }
  if (p.src.a) { za = rs_load<LB>(p.src.a + c0, li, z4, z2, z1); zb = rs_load<LB>(p.src.b + c0, li, z4, z2, z1); }
  const bool zrelu = p.src.relu != 0;
  const int ohw = p.OH * p.OW;
  const float* ybase = p.dy + co0;
  const float* zbase = p.src.x + c0;
  const bool same = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0;      // 1x1: the activation pixel is the dy pixel
  f32x4 acc[LA][LB];
#pragma unroll
  for (int e = 0; e < LA; ++e)
#pragma unroll
    for (int f = 0; f < LB; ++f) acc[e][f] = (f32x4){0.f, 0.f, 0.f, 0.f};

  {
    // [r4] The loop used to spend 6-11 vector instructions per MFMA (r03 counters: 6892 VALU / 1148 MFMA per wave, 66-70 % issue stall; 52 of
    // the 84 VALU of the compute block were v_cndmask, the load blocks re-derived (n, oh, ow) by integer division for every k-step): with
    // 24 issue cycles free per 32-cycle fp32 MFMA the kernel was bound by VALU issue, not by HBM.  Now
    //   * this lane's pixel walks incrementally (4 pixels per k-step: offsets by addition, (n, oh, ow) by carries, no division);
    //   * channel-validity selects are gone: an operand element of a channel beyond the tile only feeds accumulator rows / columns that
    //     are never stored (the combine below masks them), and its load address is clamped as before;
    //   * pixel validity (tail of the range, zero padding) is applied to ONE operand only, the activation: 0 * dy adds nothing, and dy of a
    //     masked pixel is read from a valid address.
    // Same products, same summation order: results are bit-identical to the previous form for finite gradients.
    int pp = pbeg + 4 * s_beg + kq;
    int n_ = 0, oh_ = 0, ow_ = 0;
    if (!same) { n_ = pp / ohw; const int rem = pp - n_ * ohw; oh_ = rem / p.OW; ow_ = rem - oh_ * p.OW; }
    const int ylane = LA == 4 ? (y4 ? 4 * li : 0) : (y2 ? 2 * li : 0), ylane1 = (LA == 3 && y1) ? 32 + li : 0;
    const int zlane = LB == 4 ? (z4 ? 4 * li : 0) : (z2 ? 2 * li : 0), zlane1 = (LB == 3 && z1) ? 32 + li : 0;
    WgScale fsc = {0, 0};
    for (int s0 = s_beg; s0 < s_end; s0 += RS_U) {
      RsFrag<LA> dy4[RS_U]; RsFrag<LB> z4v[RS_U];
      bool zv[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const bool pv_ = (s0 + u) < s_end && pp < pend;
        dy4[u] = rs_load_at<LA>(ybase + (pv_ ? (long)pp * p.lddy : 0), ylane, ylane1);
        long zoff = 0; bool okz = pv_;
        if (same) zoff = (long)pp * p.src.ld;
        else {
          const int ih = oh_ * p.stride - p.pad + kh * p.dil, iw = ow_ * p.stride - p.pad + kw * p.dil;
          okz = okz && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
          zoff = ((long)(n_ * p.H + ih) * p.W + iw) * p.src.ld;
          ow_ += 4;                                          // the lane's next pixel: 4 further along the flattened (n, oh, ow) order
          while (ow_ >= p.OW) { ow_ -= p.OW; if (++oh_ >= p.OH) { oh_ = 0; ++n_; } }
        }
        z4v[u] = rs_load_at<LB>(zbase + (okz ? zoff : 0), zlane, zlane1);
        zv[u] = okz;
        pp += 4;
      }
      if constexpr (F16) {
        float my = 0.f, mz = 0.f;
#pragma unroll
        for (int u = 0; u < RS_U; ++u) {
          const bool ok = zv[u];
#pragma unroll
          for (int f = 0; f < LB; ++f) {
            float x = fmaf(za.v[f], z4v[u].v[f], zb.v[f]);
            if (zrelu) x = fmaxf(x, 0.f);
            x = ok ? x : 0.f;
            z4v[u].v[f] = x;
            mz = fmaxf(mz, fabsf(x));
          }
#pragma unroll
          for (int e = 0; e < LA; ++e) my = fmaxf(my, fabsf(dy4[u].v[e]));
        }
        const int wy = f16_scale_field(wave_umax(__float_as_uint(my))), wz = f16_scale_field(wave_umax(__float_as_uint(mz)));
        int sh = 0;
        if (fsc.kfy == 0) fsc.kfy = wy; else if (wy < fsc.kfy) { sh += wy - fsc.kfy; fsc.kfy = wy; }
        if (fsc.kfz == 0) fsc.kfz = wz; else if (wz < fsc.kfz) { sh += wz - fsc.kfz; fsc.kfz = wz; }
        if (sh != 0) {                          // (wave-uniform) a larger batch: the sums move to the coarser scale, exactly
          const int rf = 127 + sh;
          const float r = rf > 0 ? wg_pow2(rf) : 0.f;
#pragma unroll
          for (int e = 0; e < LA; ++e)
#pragma unroll
            for (int f = 0; f < LB; ++f) acc[e][f] *= r;
        }
        const float sy = wg_pow2(fsc.kfy), sz = wg_pow2(fsc.kfz);
        wg_f16x4 yh[LA], yl[LA], zh[LB], zl[LB];
#pragma unroll
        for (int e = 0; e < LA; ++e) {
          uint2 pl[2];
          split4h(make_float4(dy4[0].v[e] * sy, dy4[1].v[e] * sy, dy4[2].v[e] * sy, dy4[3].v[e] * sy), pl);
          yh[e] = __builtin_bit_cast(wg_f16x4, pl[0]); yl[e] = __builtin_bit_cast(wg_f16x4, pl[1]);
        }
#pragma unroll
        for (int f = 0; f < LB; ++f) {
          uint2 pl[2];
          split4h(make_float4(z4v[0].v[f] * sz, z4v[1].v[f] * sz, z4v[2].v[f] * sz, z4v[3].v[f] * sz), pl);
          zh[f] = __builtin_bit_cast(wg_f16x4, pl[0]); zl[f] = __builtin_bit_cast(wg_f16x4, pl[1]);
        }
#pragma unroll
        for (int e = 0; e < LA; ++e)
#pragma unroll
          for (int f = 0; f < LB; ++f) {
            acc[e][f] = __builtin_amdgcn_mfma_f32_16x16x16f16(yl[e], zh[f], acc[e][f], 0, 0, 0);
            acc[e][f] = __builtin_amdgcn_mfma_f32_16x16x16f16(yh[e], zl[f], acc[e][f], 0, 0, 0);
            acc[e][f] = __builtin_amdgcn_mfma_f32_16x16x16f16(yh[e], zh[f], acc[e][f], 0, 0, 0);
          }
      } else {
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        RsFrag<LB> v = z4v[u];
        const bool ok = zv[u];
#pragma unroll
        for (int f = 0; f < LB; ++f) {
          float x = fmaf(za.v[f], v.v[f], zb.v[f]);
          if (zrelu) x = fmaxf(x, 0.f);
          v.v[f] = ok ? x : 0.f;
        }
#pragma unroll
        for (int e = 0; e < LA; ++e)
#pragma unroll
          for (int f = 0; f < LB; ++f)
            acc[e][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(dy4[u].v[e], v.v[f], acc[e][f], 0, 0, 0);
      }
      }
    }
    if (F16) {                                  // this wave's two scales leave its sums
      const float iy = wg_pow2(254 - fsc.kfy), iz = wg_pow2(254 - fsc.kfz);
#pragma unroll
      for (int e = 0; e < LA; ++e)
#pragma unroll
        for (int f = 0; f < LB; ++f) acc[e][f] = acc[e][f] * iy * iz;
    }
  }
  // combine the four waves in a fixed order; acc[e][f][r] = dW[co0 + chanA(e, 4*kq + r)][c0 + chanB(f, li)]
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int e = 0; e < LA; ++e)
#pragma unroll
        for (int f = 0; f < LB; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* d = &tile[rs_chan<LA>(e, 4 * kq + r)][rs_chan<LB>(f, li)];
            *d = (w == 0) ? acc[e][f][r] : *d + acc[e][f][r];
          }
    }
    __syncthreads();
  }
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * p.taps * C;
  for (int idx = t; idx < RS_T * RS_T; idx += 256) {
    const int r = idx / RS_T, cc = idx - r * RS_T;
    if (r < ncy && cc < ncz) wsb[((long)(co0 + r) * p.taps + tap) * C + c0 + cc] = tile[r][cc];
  }
}

// f16x3 (mode 1): the narrow cell convs' weight gradients on the fp16 matrix pipe too (ABAB: step 29.57 -> 29.2 ms)
template <int LA, int LB, bool B> WgFn wg_rs(int mode) { return mode == 1 ? wgrad_rs_kernel<LA, LB, B, true> : wgrad_rs_kernel<LA, LB, B>; }
}  // namespace

template <bool B> static WgVariant wg_rs_any(int cty, int ctz, int mode) {
  WgFn fn = nullptr;
  if ((cty == 3 || cty == 4) && (ctz == 3 || ctz == 4))
    fn = cty == 3 ? (ctz == 3 ? wg_rs<3, 3, B>(mode) : wg_rs<3, 4, B>(mode)) : (ctz == 3 ? wg_rs<4, 3, B>(mode) : wg_rs<4, 4, B>(mode));
  return {fn, 256, 0};
}
WgVariant wg_variant_rs(bool batch, int cty, int ctz, int mode) { return batch ? wg_rs_any<true>(cty, ctz, mode) : wg_rs_any<false>(cty, ctz, mode); }
