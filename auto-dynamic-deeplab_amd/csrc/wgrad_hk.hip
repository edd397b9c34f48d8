// wgrad_hk.hip — the halo-patch weight-gradient kernels of the cells' dense dilated convolutions, the taps split across the waves:
// wgrad_hk_kernel (fp32) and its split-precision form wgrad_hkb_kernel (wgrad.h; choice and launch: wgrad.hip).
#include "wgrad.h"

namespace {

// Halo-patch weight gradient of the cells' dense dilated convolutions (dil_conv_3x3 / dil_conv_5x5: 40/80/160 channels,
// dilation <= 2).  Same staging as wgrad_h3_kernel — per 64-pixel row segment dy [64][16*CT] and the KS activation rows
// [KS][64+(KS-1)d][16] go to LDS once and every tap reads its shifted window — but the accumulators are split the other
// way round: all four waves use every output-channel tile and each owns a QUARTER OF THE TAPS (7 of 25, 3 of 9), so a
// 40-channel conv keeps 3x7 = 21 accumulator tiles per wave with 83 % useful rows.  On the per-tap kernels these launches
// re-read dy and the activation once per tap (25x) and were bound by L2 bandwidth.

template <int KS, int CT, bool BATCH>
__global__ void __launch_bounds__(256, 2) wgrad_hk_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  constexpr int TAPS = KS * KS, TPW = (TAPS + 3) / 4, HK = KS / 2;
  constexpr int BCO = 16 * CT, LY = BCO, YQ = BCO / 4;            // 48 and 80 are = 16 mod 32: conflict-free fragment reads
  constexpr int NYJ = (H3_KP * YQ + 255) / 256;
  constexpr int NZJ = (KS * HK_ZW * 4 + 255) / 256;
  __shared__ __attribute__((aligned(16))) float Ys[H3_KP * LY];
  __shared__ __attribute__((aligned(16))) float Zs[KS * HK_ZW * 16];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int zt = blk_x % p.nzt, yt = blk_x / p.nzt;
  const int co0 = yt * BCO, c0 = zt * 16;
  const int d = p.dil, ZW = H3_KP + (KS - 1) * d;
  const int spr = (p.OW + H3_KP - 1) / H3_KP;
  const int nseg = p.N * p.OH * spr;
  const int sbeg = blk_y * p.chunkP;
  int send = sbeg + p.chunkP; if (send > nseg) send = nseg;

  int yrow[NYJ], yqv[NYJ];
#pragma unroll
  for (int k = 0; k < NYJ; ++k) { const int slot = t + 256 * k; yrow[k] = slot / YQ; yqv[k] = slot - yrow[k] * YQ; }   // yrow >= 64: outside
  const int zq = t & 3, zc = c0 + 4 * zq, nremz = p.src.C - zc;
  int zr[NZJ], zj[NZJ];
#pragma unroll
  for (int k = 0; k < NZJ; ++k) {
    const int pix = (t + 256 * k) >> 2;
    zr[k] = pix / ZW; zj[k] = pix - zr[k] * ZW;         // zr >= KS marks a slot outside the patch
  }
  float4 za = make_float4(1.f, 1.f, 1.f, 1.f), zb = zero4();
  if (p.src.a && nremz > 0) { za = ld4(p.src.a + zc); zb = ld4(p.src.b + zc); }
  const bool zrelu = p.src.relu != 0;
  int zbase[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    int tap = wave * TPW + j; if (tap > TAPS - 1) tap = TAPS - 1;      // surplus slots of the last wave recompute the last tap (discarded)
    zbase[j] = (((tap / KS) * HK_ZW) + kq + (tap % KS) * d) * 16 + li;
  }

  f32x4 acc[CT][TPW];
#pragma unroll
  for (int i = 0; i < CT; ++i)
#pragma unroll
    for (int j = 0; j < TPW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float4 ry[NYJ], rz[NZJ];
  unsigned ymask = 0, zmask = 0;
  auto load_step = [&](int seg) {
    const int rowid = seg / spr, sx = seg - rowid * spr;
    const int n = rowid / p.OH, oh = rowid - n * p.OH;
    const int ow0 = sx * H3_KP;
    const long pp0 = (long)rowid * p.OW + ow0;
    ymask = 0; zmask = 0;
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      const int co = co0 + 4 * yqv[k];
      const bool ok = yrow[k] < H3_KP && co < p.Cout && ow0 + yrow[k] < p.OW;
      ry[k] = ld4(ok ? p.dy + (pp0 + yrow[k]) * p.lddy + co : p.dy);
      ymask |= (ok ? 1u : 0u) << k;
    }
#pragma unroll
    for (int k = 0; k < NZJ; ++k) {
      const int ih = oh + (zr[k] - HK) * d, iw = ow0 - HK * d + zj[k];
      const bool ok = zr[k] < KS && nremz > 0 && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      rz[k] = ld4(ok ? p.src.x + ((long)(n * p.H + ih) * p.W + iw) * p.src.ld + zc : p.src.x);
      zmask |= (ok ? 1u : 0u) << k;
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      float4 v = ry[k];
      const bool ok = (ymask >> k) & 1u;
      v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
      if (yrow[k] < H3_KP) lds_st4(&Ys[yrow[k] * LY + 4 * yqv[k]], v);
    }
#pragma unroll
    for (int k = 0; k < NZJ; ++k) {
      float4 v = rz[k];
      v.x = fmaf(za.x, v.x, zb.x); v.y = fmaf(za.y, v.y, zb.y); v.z = fmaf(za.z, v.z, zb.z); v.w = fmaf(za.w, v.w, zb.w);
      if (zrelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      const bool ok = (zmask >> k) & 1u;
      v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
      if (zr[k] < KS) lds_st4(&Zs[(zr[k] * HK_ZW + zj[k]) * 16 + 4 * zq], v);
    }
  };

  if (sbeg < send) {
    load_step(sbeg);
    store_step();
    __syncthreads();
    const float* yw = &Ys[kq * LY + li];
    for (int seg = sbeg; seg < send; ++seg) {
      const bool more = seg + 1 < send;
      if (more) load_step(seg + 1);
      float yfA[CT], zfA[TPW], yfB[CT], zfB[TPW];
      auto rd = [&](int s4, float* yf, float* zf) {
#pragma unroll
        for (int i = 0; i < CT; ++i) yf[i] = yw[s4 * 4 * LY + i * 16];
#pragma unroll
        for (int j = 0; j < TPW; ++j) zf[j] = Zs[zbase[j] + s4 * 64];
      };
      auto mma = [&](const float* yf, const float* zf) {
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
          for (int j = 0; j < TPW; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(yf[i], zf[j], acc[i][j], 0, 0, 0);
      };
      rd(0, yfA, zfA);
#pragma unroll
      for (int s4 = 0; s4 < H3_KP / 4; s4 += 2) {
        rd(s4 + 1, yfB, zfB);
        __builtin_amdgcn_sched_barrier(0);
        mma(yfA, zfA);
        __builtin_amdgcn_sched_barrier(0);
        if (s4 + 2 < H3_KP / 4) rd(s4 + 2, yfA, zfA);
        __builtin_amdgcn_sched_barrier(0);
        mma(yfB, zfB);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
      if (more) { store_step(); __syncthreads(); }
    }
  }
  const int C = p.src.C;
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * TAPS * C;
  const int c = c0 + li;
#pragma unroll
  for (int i = 0; i < CT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cow = co0 + i * 16 + kq * 4 + r;
      if (cow < p.Cout && c < C) {
        gfloat* o = wsb + (long)cow * TAPS * C + c;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          const int tap = wave * TPW + j;
          if (tap < TAPS) o[tap * C] = acc[i][j][r];
        }
      }
    }
}


// Split-bf16 form of wgrad_hk_kernel (same work decomposition, partial-tile layout and epilogue; arithmetic, LDS images and
// transposed fragment reads as in wgrad_h3b_kernel): every wave uses all CT output-channel tiles and owns a quarter of the taps.
template <int KS, int CT, bool BATCH, int NP>
__global__ void __launch_bounds__(256, 2) wgrad_hkb_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  constexpr int TAPS = KS * KS, TPW = (TAPS + 3) / 4, HK = KS / 2;
  constexpr int BCO = 16 * CT, YQ = BCO / 4;
  constexpr int NYJ = (H3_KP * YQ + 255) / 256;
  constexpr int NZJ = (KS * HK_ZW * 4 + 255) / 256;
  constexpr int YIMG = H3_KP * 32 + 32, ZROW = HKB_ZWP * 32;       // bytes per dy tile image / per patch row (one plane)
  constexpr int YPL = CT * YIMG, ZPL = KS * ZROW;
  extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];
  unsigned char* Yb = wsm;                                        // [NP][CT][64 px][16 co]
  unsigned char* Zb = wsm + NP * YPL;                             // [NP][KS rows][HKB_ZWP px][16 ci]
  unsigned* wmx = reinterpret_cast<unsigned*>(wsm + NP * (YPL + ZPL));      // NP = 2: [2][4] the waves' largest magnitudes of the segment being staged (wgrad_h3b_kernel)
  WgScale fsc = {0, 0};

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int zt = blk_x % p.nzt, yt = blk_x / p.nzt;
  const int co0 = yt * BCO, c0 = zt * 16;
  const int d = p.dil, ZW = H3_KP + (KS - 1) * d;
  const int spr = (p.OW + H3_KP - 1) / H3_KP;
  const int nseg = p.N * p.OH * spr;
  const int sbeg = blk_y * p.chunkP;
  int send = sbeg + p.chunkP; if (send > nseg) send = nseg;

  int yrow[NYJ], yqv[NYJ];
#pragma unroll
  for (int k = 0; k < NYJ; ++k) { const int slot = t + 256 * k; yrow[k] = slot / YQ; yqv[k] = slot - yrow[k] * YQ; }   // yrow >= 64: outside
  const int zq = t & 3, zc = c0 + 4 * zq, nremz = p.src.C - zc;
  int zr[NZJ], zj[NZJ];
#pragma unroll
  for (int k = 0; k < NZJ; ++k) {
    const int pix = (t + 256 * k) >> 2;
    zr[k] = pix / ZW; zj[k] = pix - zr[k] * ZW;         // zr >= KS marks a slot outside the patch
  }
  float4 za = make_float4(1.f, 1.f, 1.f, 1.f), zb = zero4();
  if (p.src.a && nremz > 0) { za = ld4(p.src.a + zc); zb = ld4(p.src.b + zc); }
  const bool zrelu = p.src.relu != 0;
  const int tq = li >> 2, tp = li & 3;
  const int lrow = 8 * kq + tq;
  int zrow_off[TPW], zshift[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    int tap = wave * TPW + j; if (tap > TAPS - 1) tap = TAPS - 1;      // surplus slots of the last wave recompute the last tap (discarded)
    zrow_off[j] = (tap / KS) * ZROW; zshift[j] = (tap % KS) * d;
  }

  f32x4 acc[CT][TPW];
#pragma unroll
  for (int i = 0; i < CT; ++i)
#pragma unroll
    for (int j = 0; j < TPW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float4 ry[NYJ], rz[NZJ];
  unsigned ymask = 0, zmask = 0;
  auto load_step = [&](int seg) {
    const int rowid = seg / spr, sx = seg - rowid * spr;
    const int n = rowid / p.OH, oh = rowid - n * p.OH;
    const int ow0 = sx * H3_KP;
    const long pp0 = (long)rowid * p.OW + ow0;
    ymask = 0; zmask = 0;
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      const int co = co0 + 4 * yqv[k];
      const bool ok = yrow[k] < H3_KP && co < p.Cout && ow0 + yrow[k] < p.OW;
      ry[k] = ld4(ok ? p.dy + (pp0 + yrow[k]) * p.lddy + co : p.dy);
      ymask |= (ok ? 1u : 0u) << k;
    }
#pragma unroll
    for (int k = 0; k < NZJ; ++k) {
      const int ih = oh + (zr[k] - HK) * d, iw = ow0 - HK * d + zj[k];
      const bool ok = zr[k] < KS && nremz > 0 && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      rz[k] = ld4(ok ? p.src.x + ((long)(n * p.H + ih) * p.W + iw) * p.src.ld + zc : p.src.x);
      zmask |= (ok ? 1u : 0u) << k;
    }
  };
  auto ypro = [&](int k) {
    float4 v = ry[k];
    const bool ok = (ymask >> k) & 1u;
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
    return v;
  };
  auto zpro = [&](int k) {
    float4 v = rz[k];
    v.x = fmaf(za.x, v.x, zb.x); v.y = fmaf(za.y, v.y, zb.y); v.z = fmaf(za.z, v.z, zb.z); v.w = fmaf(za.w, v.w, zb.w);
    if (zrelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    const bool ok = (zmask >> k) & 1u;
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
    return v;
  };
  auto prep2 = [&]() {                                               // NP = 2: masks and prologue in place, the wave's maxima to LDS (in front of the barrier)
    unsigned my = 0, mz = 0;
#pragma unroll
    for (int k = 0; k < NYJ; ++k) { ry[k] = ypro(k); const unsigned b = absbits4(ry[k]); my = b > my ? b : my; }
#pragma unroll
    for (int k = 0; k < NZJ; ++k) { rz[k] = zpro(k); const unsigned b = absbits4(rz[k]); mz = b > mz ? b : mz; }
    wg_publish_max(wmx, 4, wave, lane, my, mz);
  };
  auto rescale2 = [&]() { wg_acc_rescale(acc, wg_rescale(wmx, 4, fsc)); };
  auto store_step = [&]() {
    const float sy = NP == 2 ? wg_pow2(fsc.kfy) : 1.f, sz = NP == 2 ? wg_pow2(fsc.kfz) : 1.f;
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      const float4 v = NP == 2 ? wg_mul4(ry[k], sy) : ypro(k);
      if (yrow[k] < H3_KP) {
        uint2 pl[NP];
        wg_split4<NP>(v, pl);
        const int off = (yqv[k] >> 2) * YIMG + wg_prow(yrow[k]) + 8 * (yqv[k] & 3);
#pragma unroll
        for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(Yb + m * YPL + off) = pl[m];
      }
    }
#pragma unroll
    for (int k = 0; k < NZJ; ++k) {
      const float4 v = NP == 2 ? wg_mul4(rz[k], sz) : zpro(k);
      if (zr[k] < KS) {
        uint2 pl[NP];
        wg_split4<NP>(v, pl);
        const int off = zr[k] * ZROW + wg_prow(zj[k]) + 8 * zq;
#pragma unroll
        for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(Zb + m * ZPL + off) = pl[m];
      }
    }
  };

  if (sbeg < send) {
    load_step(sbeg);
    if (NP == 2) { prep2(); __syncthreads(); rescale2(); }
    store_step();
    __syncthreads();
    for (int seg = sbeg; seg < send; ++seg) {
      const bool more = seg + 1 < send;
      if (more) load_step(seg + 1);
#pragma unroll
      for (int ks = 0; ks < H3_KP / 32; ++ks) {
        wg_bf16x8 yf[CT][NP];
#pragma unroll
        for (int i = 0; i < CT; ++i) wg_tr_read<NP>(Yb + i * YIMG, YPL, ks * 32, lrow, tp, yf[i]);
        wg_bf16x8 zf[2][NP];
        wg_tr_read<NP>(Zb + zrow_off[0], ZPL, ks * 32 + zshift[0], lrow, tp, zf[0]);
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if (j + 1 < TPW) wg_tr_read<NP>(Zb + zrow_off[j + 1], ZPL, ks * 32 + zshift[j + 1], lrow, tp, zf[(j + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
          wg_terms<NP>(acc, j, yf, zf[j & 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (NP == 2 && more) prep2();
      __syncthreads();
      if (more) { if (NP == 2) rescale2(); store_step(); __syncthreads(); }
    }
  }
  const int C = p.src.C;
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * TAPS * C;
  if (NP == 2) {
    const float iy = wg_pow2(254 - fsc.kfy), iz = wg_pow2(254 - fsc.kfz);
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
      for (int j = 0; j < TPW; ++j) acc[i][j] = acc[i][j] * iy * iz;
  }
  const int c = c0 + li;
#pragma unroll
  for (int i = 0; i < CT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cow = co0 + i * 16 + kq * 4 + r;
      if (cow < p.Cout && c < C) {
        gfloat* o = wsb + (long)cow * TAPS * C + c;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          const int tap = wave * TPW + j;
          if (tap < TAPS) o[tap * C] = acc[i][j][r];
        }
      }
    }
}

template <int KS, int CT, bool B> WgVariant wg_hk(int np) {
  if (!np) return {wgrad_hk_kernel<KS, CT, B>, 256, 0};
  return np == 3 ? wg_dyn_lds<wgrad_hkb_kernel<KS, CT, B, 3>>(256, wg_hkb_lds(KS, CT, 3))
                 : wg_dyn_lds<wgrad_hkb_kernel<KS, CT, B, 2>>(256, wg_hkb_lds(KS, CT, 2));
}
}  // namespace

template <bool B> static WgVariant wg_hk_any(int cty, int ctz, int np) {
  if (ctz == 3 && cty == 3) return wg_hk<3, 3, B>(np);
  if (ctz == 3 && cty == 5) return wg_hk<3, 5, B>(np);
  if (ctz == 5 && cty == 3) return wg_hk<5, 3, B>(np);
  return {nullptr, 256, 0};
}
WgVariant wg_variant_hk(bool batch, int cty, int ctz, int np) { return batch ? wg_hk_any<true>(cty, ctz, np) : wg_hk_any<false>(cty, ctz, np); }
