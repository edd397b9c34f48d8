// wgrad_pix.hip — the fp32 weight-gradient kernels that stage [pixel][channel] tiles of both operands per tap (wgrad.h; choice and launch: wgrad.hip):
// GEMM with M = output channels (tile 16*CTY), N = input channels of one tap (tile 16*CTZ) and the
// reduction over pixels.  A block owns one (co tile, tap, c tile) and one slice of the pixel range;
// its four waves each take 16 of the 64 pixels staged per step (both tiles are staged in their memory
// order [pixel][channel]; MFMA fragments are read with ds_read_b32, rows padded so that the two pixel
// rows a 32-lane group touches fall on disjoint banks).  Wave partials are combined through LDS in a
// fixed order and the per-slice tiles go to a workspace that addk reduces deterministically into dW.
#include "wgrad.h"

namespace {

template <int CTY, int CTZ, bool BATCH>
__global__ void __launch_bounds__(256) wgrad_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  constexpr int BCY = 16 * CTY, BCZ = 16 * CTZ;
  constexpr int LY = ldpad(BCY), LZ = ldpad(BCZ);
  constexpr int NYJ = (KP * BCY / 4 + 255) / 256;
  constexpr int NZJ = (KP * BCZ / 4 + 255) / 256;
  constexpr int STAGE = KP * LY + KP * LZ;
  constexpr int TILE = BCY * BCZ;
  constexpr int LDSF = STAGE > TILE ? STAGE : TILE;
  __shared__ __attribute__((aligned(16))) float lds[LDSF];
  float* Ys = lds;
  float* Zs = lds + KP * LY;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  int bx = blk_x;
  const int zt = bx % p.nzt; bx /= p.nzt;
  const int tap = bx % p.taps; const int yt = bx / p.taps;
  const int kh = tap / p.KW, kw = tap - kh * p.KW;
  const int co0 = yt * BCY, c0 = zt * BCZ;
  const int ohw = p.OH * p.OW;
  const int pbeg = blk_y * p.chunkP;
  int pend = pbeg + p.chunkP; if (pend > p.P) pend = p.P;
  // lazy-BN scale/shift of this thread's channel quads (fixed across pixel steps)
  float4 za[NZJ], zb[NZJ];
#pragma unroll
  for (int j = 0; j < NZJ; ++j) {
    int slot = t + 256 * j, row = slot / (BCZ / 4), q = slot - row * (BCZ / 4);
    int c = c0 + 4 * q;
    za[j] = make_float4(1.f, 1.f, 1.f, 1.f); zb[j] = zero4();
    if (p.src.a && row < KP && c < p.src.C) { za[j] = ld4g(p.src.a + c, p.src.C - c, p.vecZ); zb[j] = ld4g(p.src.b + c, p.src.C - c, p.vecZ); }
  }
  const bool zrelu = p.src.relu != 0;

  f32x4 acc[CTY][CTZ];
#pragma unroll
  for (int i = 0; i < CTY; ++i)
#pragma unroll
    for (int j = 0; j < CTZ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float4 ry[NYJ], rz[NZJ];
  unsigned zmask = 0;
  auto load_step = [&](int p0) {
    zmask = 0;
#pragma unroll
    for (int j = 0; j < NYJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCY / 4), q = slot - row * (BCY / 4);
      int pp = p0 + row; int co = co0 + 4 * q;
      float4 v = zero4();
      if (row < KP && pp < pend && co < p.Cout) v = ld4g(p.dy + (long)pp * p.lddy + co, p.Cout - co, p.vecY);
      ry[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NZJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCZ / 4), q = slot - row * (BCZ / 4);
      int pp = p0 + row; int c = c0 + 4 * q;
      float4 v = zero4();
      if (row < KP && pp < pend && c < p.src.C) {
        int n = pp / ohw; int rem = pp - n * ohw;
        int oh = rem / p.OW, ow = rem - oh * p.OW;
        int ih = oh * p.stride - p.pad + kh * p.dil, iw = ow * p.stride - p.pad + kw * p.dil;
        if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) {
          const float* xp = p.src.x + ((long)(n * p.H + ih) * p.W + iw) * p.src.ld + c;
          const int nrem = p.src.C - c;
          v = ld4g(xp, nrem, p.vecZ);
          zmask |= 1u << j;
        }
      }
      rz[j] = v;
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int j = 0; j < NYJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCY / 4), q = slot - row * (BCY / 4);
      if (row < KP) lds_st4(&Ys[row * LY + 4 * q], ry[j]);
    }
#pragma unroll
    for (int j = 0; j < NZJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCZ / 4), q = slot - row * (BCZ / 4);
      float4 v = rz[j];
      if (zmask & (1u << j)) {      // lazy prologue, applied after the MFMAs of the previous step
        const int nrem = p.src.C - (c0 + 4 * q);
        v.x = fmaf(za[j].x, v.x, zb[j].x); v.y = fmaf(za[j].y, v.y, zb[j].y);
        v.z = fmaf(za[j].z, v.z, zb[j].z); v.w = fmaf(za[j].w, v.w, zb[j].w);
        if (zrelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        if (nrem < 4) { if (nrem < 2) v.y = 0.f; if (nrem < 3) v.z = 0.f; v.w = 0.f; }
      }
      if (row < KP) lds_st4(&Zs[row * LZ + 4 * q], v);
    }
  };

  if (pbeg < pend) {
    load_step(pbeg);
    store_step();
    __syncthreads();
    for (int p0 = pbeg; p0 < pend; p0 += KP) {
      const bool more = p0 + KP < pend;
      if (more) load_step(p0 + KP);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int px = wave * 16 + ks * 4 + kq;
        float yf[CTY], zf[CTZ];
#pragma unroll
        for (int i = 0; i < CTY; ++i) yf[i] = Ys[px * LY + i * 16 + li];
#pragma unroll
        for (int j = 0; j < CTZ; ++j) zf[j] = Zs[px * LZ + j * 16 + li];
#pragma unroll
        for (int i = 0; i < CTY; ++i)
#pragma unroll
          for (int j = 0; j < CTZ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(yf[i], zf[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
      if (more) { store_step(); __syncthreads(); }
    }
  }

  // combine the four waves in a fixed order (deterministic), tile layout [co][c]
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < CTY; ++i)
#pragma unroll
        for (int j = 0; j < CTZ; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int idx = (i * 16 + kq * 4 + r) * BCZ + j * 16 + li;
            lds[idx] = (w == 0) ? acc[i][j][r] : lds[idx] + acc[i][j][r];
          }
    }
    __syncthreads();
  }
  // workspace layout: [split][co][tap][c] over the real (unpadded) extents
  const int C = p.src.C;
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * p.taps * C;
  for (int idx = t; idx < TILE; idx += 256) {
    int r = idx / BCZ, cc = idx - r * BCZ;
    int co = co0 + r, c = c0 + cc;
    if (co < p.Cout && c < C) wsb[((long)co * p.taps + tap) * C + c] = lds[idx];
  }
}

// Output-split variant for the 256-wide heads (ASPP / decoder): the four waves form a 2x2 grid over a
// (32*TY) x (32*TZ) output tile, every wave walks ALL staged pixels and owns a TYxTZ block of 16x16 accumulators
// (32-64 VGPRs instead of the 128 of the pixel-split form), so 2-3 blocks fit a CU and staging overlaps the MFMAs;
// no cross-wave reduction is needed.
template <int TY, int TZ, bool BATCH>
__global__ void __launch_bounds__(256) wgrad_os_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  constexpr int BCY = 32 * TY, BCZ = 32 * TZ;
  constexpr int LY = ldpad(BCY), LZ = ldpad(BCZ);
  constexpr int NYJ = (KP * BCY / 4 + 255) / 256;
  constexpr int NZJ = (KP * BCZ / 4 + 255) / 256;
  __shared__ __attribute__((aligned(16))) float lds[KP * LY + KP * LZ];
  float* Ys = lds;
  float* Zs = lds + KP * LY;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int wy = wave >> 1, wz = wave & 1;
  int bx = blk_x;
  const int zt = bx % p.nzt; bx /= p.nzt;
  const int tap = bx % p.taps; const int yt = bx / p.taps;
  const int kh = tap / p.KW, kw = tap - kh * p.KW;
  const int co0 = yt * BCY, c0 = zt * BCZ;
  const int ohw = p.OH * p.OW;
  const int pbeg = blk_y * p.chunkP;
  int pend = pbeg + p.chunkP; if (pend > p.P) pend = p.P;
  float4 za[NZJ], zb[NZJ];
#pragma unroll
  for (int j = 0; j < NZJ; ++j) {
    int slot = t + 256 * j, row = slot / (BCZ / 4), q = slot - row * (BCZ / 4);
    int c = c0 + 4 * q;
    za[j] = make_float4(1.f, 1.f, 1.f, 1.f); zb[j] = zero4();
    if (p.src.a && row < KP && c < p.src.C) { za[j] = ld4g(p.src.a + c, p.src.C - c, p.vecZ); zb[j] = ld4g(p.src.b + c, p.src.C - c, p.vecZ); }
  }
  const bool zrelu = p.src.relu != 0;

  f32x4 acc[TY][TZ];
#pragma unroll
  for (int i = 0; i < TY; ++i)
#pragma unroll
    for (int j = 0; j < TZ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float4 ry[NYJ], rz[NZJ];
  unsigned zmask = 0;
  auto load_step = [&](int p0) {
    zmask = 0;
#pragma unroll
    for (int j = 0; j < NYJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCY / 4), q = slot - row * (BCY / 4);
      int pp = p0 + row; int co = co0 + 4 * q;
      float4 v = zero4();
      if (row < KP && pp < pend && co < p.Cout) v = ld4g(p.dy + (long)pp * p.lddy + co, p.Cout - co, p.vecY);
      ry[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NZJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCZ / 4), q = slot - row * (BCZ / 4);
      int pp = p0 + row; int c = c0 + 4 * q;
      float4 v = zero4();
      if (row < KP && pp < pend && c < p.src.C) {
        int n = pp / ohw; int rem = pp - n * ohw;
        int oh = rem / p.OW, ow = rem - oh * p.OW;
        int ih = oh * p.stride - p.pad + kh * p.dil, iw = ow * p.stride - p.pad + kw * p.dil;
        if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) {
          v = ld4g(p.src.x + ((long)(n * p.H + ih) * p.W + iw) * p.src.ld + c, p.src.C - c, p.vecZ);
          zmask |= 1u << j;
        }
      }
      rz[j] = v;
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int j = 0; j < NYJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCY / 4), q = slot - row * (BCY / 4);
      if (row < KP) lds_st4(&Ys[row * LY + 4 * q], ry[j]);
    }
#pragma unroll
    for (int j = 0; j < NZJ; ++j) {
      int slot = t + 256 * j, row = slot / (BCZ / 4), q = slot - row * (BCZ / 4);
      float4 v = rz[j];
      if (zmask & (1u << j)) {
        const int nrem = p.src.C - (c0 + 4 * q);
        v.x = fmaf(za[j].x, v.x, zb[j].x); v.y = fmaf(za[j].y, v.y, zb[j].y);
        v.z = fmaf(za[j].z, v.z, zb[j].z); v.w = fmaf(za[j].w, v.w, zb[j].w);
        if (zrelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        if (nrem < 4) { if (nrem < 2) v.y = 0.f; if (nrem < 3) v.z = 0.f; v.w = 0.f; }
      }
      if (row < KP) lds_st4(&Zs[row * LZ + 4 * q], v);
    }
  };

  if (pbeg < pend) {
    load_step(pbeg);
    store_step();
    __syncthreads();
    for (int p0 = pbeg; p0 < pend; p0 += KP) {
      const bool more = p0 + KP < pend;
      if (more) load_step(p0 + KP);
#pragma unroll 4
      for (int ks = 0; ks < KP / 4; ++ks) {
        const int px = ks * 4 + kq;
        float yf[TY], zf[TZ];
#pragma unroll
        for (int i = 0; i < TY; ++i) yf[i] = Ys[px * LY + (wy * TY + i) * 16 + li];
#pragma unroll
        for (int j = 0; j < TZ; ++j) zf[j] = Zs[px * LZ + (wz * TZ + j) * 16 + li];
#pragma unroll
        for (int i = 0; i < TY; ++i)
#pragma unroll
          for (int j = 0; j < TZ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(yf[i], zf[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
      if (more) { store_step(); __syncthreads(); }
    }
  }
  const int C = p.src.C;
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * p.taps * C;
#pragma unroll
  for (int i = 0; i < TY; ++i)
#pragma unroll
    for (int j = 0; j < TZ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int co = co0 + (wy * TY + i) * 16 + kq * 4 + r, c = c0 + (wz * TZ + j) * 16 + li;
        if (co < p.Cout && c < C) wsb[((long)co * p.taps + tap) * C + c] = acc[i][j][r];
      }
}

// Weight gradient of a k x k conv with a HANDFUL of input channels (stem0: 3 -> 64, 3x3, stride 2; ADD.py:153-157): KH*KW*C <= 32 patch
// values per output pixel.  On the generic kernel this launch re-read dy once per tap (0.37 ms, 0.9 TB/s).  Here it is ONE pass in the
// register-streaming form of wgrad_rs_kernel: lane (li, kq) of a k-step = 4 pixels loads dy of pixel kq as one float4 at channel 4 li
// (component e = A operand of output-channel tile {4r + e}) and GATHERS patch values e0 = li and 16 + li of that pixel (tap e / C,
// channel e % C, prologue and zero padding applied) as the B operands of the two column tiles: 8 MFMAs per 4 pixels, dy read once.
template <bool BATCH>
__global__ void __launch_bounds__(256, 2) wgrad_st_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  __shared__ float tile[RS_T][33];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int C = p.src.C, NE = p.taps * C;                   // patch values per pixel (<= 32)
  const bool y4 = 4 * li < p.Cout;
  const int pbeg = blk_y * p.chunkP;
  int pend = pbeg + p.chunkP; if (pend > p.P) pend = p.P;
  const int span = (pend - pbeg + 3) / 4, per_wave = (span + 3) / 4;
  const int s_beg = wave * per_wave, s_end = min(span, s_beg + per_wave);
  // this lane's two patch elements: tap and channel, prologue coefficients
  int ekh[2], ekw[2], ec[2]; bool eok[2]; float ea[2], eb[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int e = 16 * f + li;
    eok[f] = e < NE;
    const int tap = eok[f] ? e / C : 0;
    ec[f] = eok[f] ? e - tap * C : 0;
    ekh[f] = (tap / p.KW) * p.dil - p.pad; ekw[f] = (tap % p.KW) * p.dil - p.pad;
    ea[f] = 1.f; eb[f] = 0.f;
    if (p.src.a && eok[f]) { ea[f] = ((const gfloat*)p.src.a)[ec[f]]; eb[f] = ((const gfloat*)p.src.b)[ec[f]]; }
  }
  const bool zrelu = p.src.relu != 0;
  const int ohw = p.OH * p.OW;
  f32x4 acc[4][2];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[e][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int s0 = s_beg; s0 < s_end; s0 += RS_U) {
    RsFrag<4> dy4[RS_U]; float zv[RS_U][2];
#pragma unroll
    for (int u = 0; u < RS_U; ++u) {
      const int pp = pbeg + 4 * (s0 + u) + kq;
      const bool pv_ = (s0 + u) < s_end && pp < pend;
      dy4[u] = rs_load<4>(p.dy + (pv_ ? (long)pp * p.lddy : 0), li, pv_ && y4, false, false);
      const int n = pp / ohw, rem = pp - n * ohw, oh = rem / p.OW, ow = rem - oh * p.OW;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int ih = oh * p.stride + ekh[f], iw = ow * p.stride + ekw[f];
        const bool ok = pv_ && eok[f] && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        float x = ((const gfloat*)p.src.x)[ok ? ((long)(n * p.H + ih) * p.W + iw) * p.src.ld + ec[f] : 0];
        x = fmaf(ea[f], x, eb[f]);
        if (zrelu) x = fmaxf(x, 0.f);
        zv[u][f] = ok ? x : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < RS_U; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 2; ++f)
          acc[e][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(dy4[u].v[e], zv[u][f], acc[e][f], 0, 0, 0);
  }
  // combine the four waves in a fixed order; acc[e][f][r] = dW[4 (4 kq + r) + e][16 f + li]
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* d = &tile[4 * (4 * kq + r) + e][16 * f + li];
            *d = (w == 0) ? acc[e][f][r] : *d + acc[e][f][r];
          }
    }
    __syncthreads();
  }
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * NE;
  for (int idx = t; idx < RS_T * 32; idx += 256) {
    const int r = idx >> 5, cc = idx & 31;
    if (r < p.Cout && cc < NE) wsb[(long)r * NE + cc] = tile[r][cc];
  }
}

template <int Y, bool B> WgFn wg_pix(int ctz) {
  switch (ctz) {
    case 1: return wgrad_kernel<Y, 1, B>;
    case 3: return wgrad_kernel<Y, 3, B>;
    case 4: return wgrad_kernel<Y, 4, B>;
    case 5: if constexpr (Y != 8) return wgrad_kernel<Y, 5, B>; else return nullptr;
    default: return nullptr;
  }
}
}  // namespace

template <bool B> static WgFn wg_pix_any(int cty, int ctz) {
  return cty == 2 ? wg_pix<2, B>(ctz) : cty == 3 ? wg_pix<3, B>(ctz) : cty == 4 ? wg_pix<4, B>(ctz) : cty == 5 ? wg_pix<5, B>(ctz) : cty == 8 ? wg_pix<8, B>(ctz) : nullptr;
}
template <bool B> static WgFn wg_os_any(int ty) { return ty == 4 ? wgrad_os_kernel<4, 2, B> : ty == 3 ? wgrad_os_kernel<3, 3, B> : ty == 2 ? wgrad_os_kernel<2, 2, B> : nullptr; }
WgVariant wg_variant_pix(bool batch, int cty, int ctz) { return {batch ? wg_pix_any<true>(cty, ctz) : wg_pix_any<false>(cty, ctz), 256, 0}; }
WgVariant wg_variant_os(bool batch, int ty) { return {batch ? wg_os_any<true>(ty) : wg_os_any<false>(ty), 256, 0}; }
WgVariant wg_variant_st(bool batch) { return {batch ? wgrad_st_kernel<true> : wgrad_st_kernel<false>, 256, 0}; }
