// wgrad_h3.hip — the halo-patch weight-gradient kernels of the wide convolutions: wgrad_h3_kernel (3x3, fp32), its split-precision form
// wgrad_h3b_kernel and the same arithmetic for the wide 1x1 heads, wgrad_h1b_kernel (wgrad.h; choice and launch: wgrad.hip).
#include "wgrad.h"

#ifdef ADDK_WG_DIAG
// diagnostic build (scripts/wgrad_phases.sh): every wave of wgrad_h3b_kernel adds its lifetime in shader-clock ticks (s_memtime) and in 100 MHz reference ticks
// (s_memrealtime) — their ratio is the clock the CUs ran at inside the kernel — and the shader ticks it spent in each phase of the segment loop:
// [0] life (shader) [1] life (reference) [2] waves [3] preparing the next segment's addresses [4] matrix phase (fragment reads + MFMA + the next segment's loads) [5] the split into registers
// (including the wait for the loads) [6] waiting at the barrier behind it [7] LDS stores and the barrier behind them
__device__ unsigned long long g_wg_diag[64][8];
#ifdef ADDK_WG_DIAG2
__device__ unsigned long long g_wg_diag2[64][2];
#endif
#define WG_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
// the eight counters summed over the waves since the last call; resets them
extern "C" int addk_wg_diag(unsigned long long* out8) {
  unsigned long long h[64][8];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_wg_diag), sizeof h) != hipSuccess) return ADDK_ERR_INVALID;
  for (int k = 0; k < 8; ++k) { out8[k] = 0; for (int i = 0; i < 64; ++i) out8[k] += h[i][k]; }
#ifdef ADDK_WG_DIAG2
  { unsigned long long h2[64][2]; (void)hipMemcpyFromSymbol(h2, HIP_SYMBOL(g_wg_diag2), sizeof h2); unsigned long long a = 0, b = 0;
    for (int i = 0; i < 64; ++i) { a += h2[i][0]; b += h2[i][1]; h2[i][0] = h2[i][1] = 0; }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wg_diag2), h2, sizeof h2);
    fprintf(stderr, "      inside split + LDS stores: waiting for the loads %.1f %% of wave life, dy part %.1f %%\n", 100.0 * a / out8[0], 100.0 * b / out8[0]); }
#endif
  for (int i = 0; i < 64; ++i) for (int k = 0; k < 8; ++k) h[i][k] = 0;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_wg_diag), h, sizeof h) == hipSuccess ? ADDK_OK : ADDK_ERR_INVALID;
}
#endif

namespace {

// Halo-patch variant for the wide 3x3 stride-1 convolutions (decoder, ASPP dilated branches, stem1): a block owns
// (64*NT output channels) x (16 input channels) x ALL NINE taps and walks its pixel range one 64-pixel row segment at a
// time.  Per segment it stages dy[64 px][64*NT] once and the three activation rows oh-d, oh, oh+d of the 16 channels
// ([3][64+2d px][16], BatchNorm/ReLU applied on the way in, zero padding after it) once, and every tap reads its
// shifted window of that patch from LDS: 64*NT + 48 floats fetched per pixel for 9*16*64*NT MACs, against 64*NT+64 per
// pixel PER TAP for the per-tap kernels above (2.5x the arithmetic intensity at NT=2, 1/9 of the global load
// instructions).  Wave w keeps co tiles [w*NT, w*NT+NT) x 9 taps = 9*NT 16x16 accumulators.
template <int NT, bool BATCH>
__global__ void __launch_bounds__(256, 2) wgrad_h3_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  constexpr int BCO = 64 * NT, LY = BCO + 16, YQ = BCO / 4, YRS = 256 / YQ;
  constexpr int NYJ = H3_KP / YRS;
  constexpr int NZJ = (3 * H3_ZW * 4 + 255) / 256;
  __shared__ __attribute__((aligned(16))) float Ys[H3_KP * LY];
  __shared__ __attribute__((aligned(16))) float Zs[3 * H3_ZW * 16];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int zt = blk_x % p.nzt, yt = blk_x / p.nzt;
  const int co0 = yt * BCO, c0 = zt * 16;
  const int d = p.dil, ZW = H3_KP + 2 * d;
  const int spr = (p.OW + H3_KP - 1) / H3_KP;          // segments per image row
  const int nseg = p.N * p.OH * spr;
  const int sbeg = blk_y * p.chunkP;
  int send = sbeg + p.chunkP; if (send > nseg) send = nseg;

  // fixed slot geometry
  const int yq = t & (YQ - 1), yrow0 = t / YQ;
  const int co = co0 + 4 * yq;
  const bool co_ok = co < p.Cout;
  const int zq = t & 3, zc = c0 + 4 * zq, nremz = p.src.C - zc;
  int zr[NZJ], zj[NZJ];
#pragma unroll
  for (int k = 0; k < NZJ; ++k) {
    const int pix = (t + 256 * k) >> 2;
    zr[k] = pix / ZW; zj[k] = pix - zr[k] * ZW;         // zr >= 3 marks a slot outside the patch
  }
  float4 za = make_float4(1.f, 1.f, 1.f, 1.f), zb = zero4();
  if (p.src.a && nremz > 0) { za = ld4g(p.src.a + zc, nremz, p.vecZ); zb = ld4g(p.src.b + zc, nremz, p.vecZ); }
  const bool zrelu = p.src.relu != 0;
  int zbase[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) zbase[tap] = (((tap / 3) * H3_ZW) + kq + (tap % 3) * d) * 16 + li;

  f32x4 acc[NT][9];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Branch-free staging: every slot always issues its 16-byte load (from a safe address when it is masked) so the
  // loads of a step go out back to back; masked slots are zeroed when they are written to LDS.
  float4 ry[NYJ], rz[NZJ];
  unsigned ymask = 0, zmask = 0;
  auto load_step = [&](int seg) {
    const int rowid = seg / spr, sx = seg - rowid * spr;
    const int n = rowid / p.OH, oh = rowid - n * p.OH;
    const int ow0 = sx * H3_KP;
    const long pp0 = (long)rowid * p.OW + ow0;
    const float* yb = p.dy + pp0 * p.lddy + co;
    ymask = 0; zmask = 0;
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      const int row = yrow0 + k * YRS;
      const bool ok = co_ok && ow0 + row < p.OW;
      ry[k] = ld4(ok ? yb + (long)row * p.lddy : p.dy);
      ymask |= (ok ? 1u : 0u) << k;
    }
#pragma unroll
    for (int k = 0; k < NZJ; ++k) {
      const int ih = oh + (zr[k] - 1) * d, iw = ow0 - d + zj[k];
      const bool ok = zr[k] < 3 && nremz > 0 && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
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
      lds_st4(&Ys[(yrow0 + k * YRS) * LY + 4 * yq], v);
    }
#pragma unroll
    for (int k = 0; k < NZJ; ++k) {
      float4 v = rz[k];
      v.x = fmaf(za.x, v.x, zb.x); v.y = fmaf(za.y, v.y, zb.y); v.z = fmaf(za.z, v.z, zb.z); v.w = fmaf(za.w, v.w, zb.w);
      if (zrelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      const bool ok = (zmask >> k) & 1u;
      v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
      if (zr[k] < 3) lds_st4(&Zs[(zr[k] * H3_ZW + zj[k]) * 16 + 4 * zq], v);
    }
  };

  if (sbeg < send) {
    load_step(sbeg);
    store_step();
    __syncthreads();
    const float* yw = &Ys[kq * LY + wave * NT * 16 + li];
    for (int seg = sbeg; seg < send; ++seg) {
      const bool more = seg + 1 < send;
      if (more) load_step(seg + 1);
      // software-pipelined fragment reads: the LDS reads of k-step s+1 are in flight while the 9*NT MFMAs of k-step s issue
      float yfA[NT], zfA[9], yfB[NT], zfB[9];
      auto rd = [&](int s4, float* yf, float* zf) {
#pragma unroll
        for (int i = 0; i < NT; ++i) yf[i] = yw[s4 * 4 * LY + i * 16];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) zf[tap] = Zs[zbase[tap] + s4 * 64];
      };
      auto mma = [&](const float* yf, const float* zf) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
          for (int tap = 0; tap < 9; ++tap)
            acc[i][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(yf[i], zf[tap], acc[i][tap], 0, 0, 0);
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
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * 9 * C;
  const int c = c0 + li;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cow = co0 + (wave * NT + i) * 16 + kq * 4 + r;
      if (cow < p.Cout && c < C) {
        gfloat* o = wsb + (long)cow * 9 * C + c;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) o[tap * C] = acc[i][tap][r];
      }
    }
}

// Split-bf16 form of wgrad_h3_kernel (same work decomposition, same partial-tile layout, same epilogue): dy and the
// activations are written as h + m + l in bf16 (exact) and a product is the sum of its six largest bf16 x bf16 terms on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation (conv3.hip: as accurate as the fp32 MFMA chain at 2.5x its rate).
// The staged LDS images and the transposed fragment reads: wgrad.h (wg_prow, wg_tr_read).
// NG = 2: a 512-thread workgroup of two wave groups, one per 16-channel input tile, which SHARE the staged dy tile (two 256-thread workgroups of
// neighbouring input tiles — which sit on one CU and run their phases together anyway: scripts/wgrad_phases.sh — split and store the same dy twice)
template <int NT, bool BATCH, int NP, int NG>
__global__ void __launch_bounds__(256 * NG, 2) wgrad_h3b_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  constexpr int NTHR = 256 * NG, BCO = 64 * NT, YT = BCO / 16, YQ = BCO / 4, YRS = NTHR / YQ;
  constexpr int NYJ = H3_KP / YRS;
  constexpr int ZWP = 104;                                        // patch row pitch in pixels (>= 64 + 2*18, multiple of 8: the swizzle works on 8-pixel blocks)
  // bytes per dy tile image / per activation patch row (one plane).  The tile images are 32 bytes apart from a multiple of
  // the 256-byte bank period: the 8 tiles x 4 channel quads a half-wave stores for one pixel row then cover all 64 banks once
  constexpr int YIMG = H3_KP * 32 + 32, ZROW = ZWP * 32;
  // one input-channel tile of the patch (one plane); with two tiles, 64 bytes off the 256-byte bank period: the two 32-byte halves a pixel's eight
  // channel quads store then hit different banks (SQ_LDS_BANK_CONFLICT 9.5 % of the LDS cycles without)
  constexpr int ZTILE = 3 * ZROW + (NG > 1 ? 64 : 0);
  constexpr int YPL = YT * YIMG, ZPL = NG * ZTILE;                // bytes per plane
  extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];
  unsigned char* Yb = wsm;                                        // [NP][YT][64 px][16 co]
  unsigned char* Zb = wsm + NP * YPL;                             // [NP][NG tiles][3 rows][ZWP px][16 ci]
  unsigned* wmx = reinterpret_cast<unsigned*>(wsm + NP * (YPL + ZPL));      // NP = 2: [2][4 NG] the waves' largest dy / activation magnitudes of the segment being staged
  WgScale fsc = {0, 0};

  const int t = threadIdx.x, lane = t & 63, li = lane & 15, kq = lane >> 4;
  const int wave8 = __builtin_amdgcn_readfirstlane(t >> 6), wave = wave8 & 3, grp = wave8 >> 2;      // output-channel tiles of this wave; its input-channel tile
  const int zt = blk_x % p.nzt, yt = blk_x / p.nzt;
  const int co0 = yt * BCO, c0 = zt * 16 * NG;
  const int d = p.dil, ZW = H3_KP + 2 * d;
  const int spr = (p.OW + H3_KP - 1) / H3_KP;
  const int nseg = p.N * p.OH * spr;
  const int sbeg = blk_y * p.chunkP;
  int send = sbeg + p.chunkP; if (send > nseg) send = nseg;

  // Staging geometry.  Everything a thread needs per segment is a THREAD CONSTANT (a byte offset from a segment-uniform base pointer, an LDS
  // offset) plus segment scalars: no per-slot divisions, address arithmetic or validity bits in vector registers.
  //   dy: thread (yq, yrow0) owns channel quad yq of rows yrow0 + k YRS of the 64-pixel segment;
  //   patch: thread (zq, zj0) owns channel quad zq of patch columns zj0 and 64 + zj0 (the latter only below 2 d) of each of the 3 rows.
  // The NEXT segment's global loads are issued one per tap INSIDE the matrix phase (they are branch-free: a lane without a valid element
  // reads element 0 of a valid row and is masked when the patch is stored): measured with the in-kernel phase clock (scripts/wgrad_phases.sh),
  // issuing 14 KB of loads per wave in one burst held every wave for 11 % of its life at the CU's 64 B/clk address path.
  constexpr int NIT = NYJ + 6;                                      // load items per segment: NYJ dy rows, 3 patch rows x 2 halves
  static_assert(NIT <= 18, "one load item per (k-step, tap)");
  const int yq = t & (YQ - 1), yrow0 = t / YQ;
  const int co = co0 + 4 * yq;                                      // < Cout: BCO divides Cout (wg_fill)
  const unsigned yoff = ((unsigned)yrow0 * (unsigned)p.lddy + (unsigned)co) * 4u;
  const long ystep = (long)YRS * p.lddy;
  // LDS offset of row yrow0 + k YRS = (k even ? ysw0 : ysw1) + k YRS 32: the swizzle bit (bit 3 of the row) alternates with k when YRS = 8
  const int ytile = (yq >> 2) * YIMG + 8 * (yq & 3);
  const int ysw0 = ytile + wg_prow(yrow0), ysw1 = ytile + wg_prow(yrow0 + YRS) - (YRS << 5);
  constexpr int ZQ = 4 * NG;                                        // channel quads per patch pixel
  const int zq = t & (ZQ - 1), zj0 = t / ZQ, zc = c0 + 4 * zq, nremz = p.src.C - zc;
  const unsigned zldb = (unsigned)p.src.ld * 4u;
  const unsigned zoff = (unsigned)zj0 * zldb + (unsigned)zc * 4u;     // byte offset of (patch column zj0, channel zc) from the patch row's column 0
  const int zsw = (zq >> 2) * ZTILE + wg_prow(zj0) + 8 * (zq & 3);  // second half: + 64 * 32 (bit 3 of 64 + zj0 is bit 3 of zj0)
  const bool zhalf1 = zj0 < 2 * d;                                  // this thread has a column in the second half (64 + zj0 < ZW)
  float4 za = make_float4(1.f, 1.f, 1.f, 1.f), zb = zero4();
  if (p.src.a && nremz > 0) { za = ld4g(p.src.a + zc, nremz, p.vecZ); zb = ld4g(p.src.b + zc, nremz, p.vecZ); }
  const bool zrelu = p.src.relu != 0, zaff = p.src.a != nullptr;
  // transposed-read lane geometry: lane 16g + 4q + pp supplies (pixel row q of the block, channels 4pp..4pp+3)
  const int tq = li >> 2, tp = li & 3;
  const int lrow = 8 * kq + tq;                                   // this lane's pixel row inside a 32-pixel k-step (first read; second +4)

  f32x4 acc[NT][9];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float4 ry[NYJ], rz[6];
  // l_*: the segment load_prep turns to next; c_*: the one it prepared last (scalars, advanced incrementally)
  int l_sx, l_oh, l_n, c_sx, c_oh, c_n;
  { const int rowid = sbeg / spr; l_sx = sbeg - rowid * spr; l_n = rowid / p.OH; l_oh = rowid - l_n * p.OH; c_sx = l_sx; c_oh = l_oh; c_n = l_n; }
  // what the load items of the prepared segment need, and the validity the store of that segment needs
  const float* yseg = p.dy; const float* zrowp[3] = {p.src.x, p.src.x, p.src.x};
  unsigned zo0 = 0, zo1 = 0;                                        // this lane's byte offsets in a patch row's image row (0: no valid element)
  int st_skip = 0;                                                  // leading pixels of the segment that belong to its left neighbour
  unsigned zrows = 0;                                               // bit r: patch row r lies inside the image
  unsigned long long zcm0 = 0, zcm1 = 0;                            // lane masks: this lane's first / second column lies inside the image (and its channels exist)
#ifdef ADDK_WG_DIAG2
  unsigned long long dsub[2] = {0, 0};        // shader ticks inside store_step: waiting for the loads, the dy part (split + LDS stores, drained)
#endif
  auto load_prep = [&](bool next) {                                 // next == false: prepare the last segment again (a harmless reload behind the block's final matrix phase)
    if (next) { c_sx = l_sx; c_oh = l_oh; c_n = l_n; if (++l_sx == spr) { l_sx = 0; if (++l_oh == p.OH) { l_oh = 0; ++l_n; } } }
    // the last segment of an image row is moved left to end at the row's end (OW >= 64: h3_ok); the st_skip pixels it then shares with its
    // neighbour get dy = 0 in store_step — every segment is a full one
    int ow0 = c_sx * H3_KP;
    st_skip = ow0 + H3_KP - p.OW; if (st_skip < 0) st_skip = 0;
    ow0 -= st_skip;
    const long rowid = (long)c_n * p.OH + c_oh;
    yseg = p.dy + (rowid * p.OW + ow0) * p.lddy;
    const int iw0 = ow0 - d;                                        // image column of patch column 0
    const bool c0ok = nremz > 0 && (unsigned)(iw0 + zj0) < (unsigned)p.W;
    const bool c1ok = nremz > 0 && zhalf1 && (unsigned)(iw0 + H3_KP + zj0) < (unsigned)p.W;
    zcm0 = __ballot(c0ok); zcm1 = __ballot(c1ok);
    const unsigned zbase = (unsigned)iw0 * zldb;                    // (wraps for iw0 < 0; a valid lane's sum does not)
    zo0 = c0ok ? zbase + zoff : 0u;
    zo1 = c1ok ? zbase + H3_KP * zldb + zoff : 0u;
    zrows = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ih = c_oh + (r - 1) * d;
      const bool rok = (unsigned)ih < (unsigned)p.H;
      zrows |= (rok ? 1u : 0u) << r;
      zrowp[r] = rok ? p.src.x + (((long)c_n * p.H + ih) * p.W) * p.src.ld : p.src.x;
    }
  };
  auto load_item = [&](int i) {
    if (i < NYJ) ry[i] = ld4so(yseg + i * ystep, yoff);
    else if (i < NIT) rz[i - NYJ] = ld4so(zrowp[(i - NYJ) >> 1], ((i - NYJ) & 1) ? zo1 : zo0);
  };
  // The split runs BEFORE the barrier that ends the matrix phase, into registers (the SIMD's arbiter serves the older of its two waves first: the wave that
  // leaves the matrix phase early splits under the other one's MFMAs instead of waiting at the barrier), the LDS stores behind it.
  constexpr bool PRE_Z = NP != 2 && !(NT == 2 && (NP == 3 || NG == 1));      // (the two-tile six-term forms have no registers for the patch's planes: only dy is split early,
  constexpr bool PRE_Y = NP != 2 && !(NT == 2 && NP == 3 && NG == 1);      //  and nothing at all in the 256-thread form, whose threads hold eight dy rows)
  // (NP = 2, split-fp16: the conversion needs the segment's scale, which exists behind that barrier only — prep2 in front of it, rescale2 + write_step behind)
  uint2 py[NYJ][NP], pz[6][NP];
  auto split_z = [&]() {
    const bool c0ok = __builtin_amdgcn_inverse_ballot_w64(zcm0), c1ok = __builtin_amdgcn_inverse_ballot_w64(zcm1);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const bool rok = (zrows >> r) & 1u;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 1 && !zhalf1) continue;
        wg_split4<NP>(wg_zpro(rz[2 * r + h], za, zb, zaff, zrelu, rok && (h ? c1ok : c0ok)), pz[2 * r + h]);
        if (!PRE_Z) {
          unsigned char* o = Zb + zsw + r * ZROW + h * (H3_KP * 32);
#pragma unroll
          for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(o + m * ZPL) = pz[2 * r + h][m];
        }
      }
    }
  };
  auto prep2 = [&]() {                                              // NP = 2: masks and prologue in place, the wave's maxima to LDS
    unsigned my = 0, mz = 0;
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      if (st_skip && yrow0 + k * YRS < st_skip) ry[k] = zero4();
      const unsigned b = absbits4(ry[k]); my = b > my ? b : my;
    }
    const bool c0ok = __builtin_amdgcn_inverse_ballot_w64(zcm0), c1ok = __builtin_amdgcn_inverse_ballot_w64(zcm1);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const bool rok = (zrows >> r) & 1u;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        rz[2 * r + h] = wg_zpro(rz[2 * r + h], za, zb, zaff, zrelu, rok && (h ? c1ok : c0ok) && (h == 0 || zhalf1));
        const unsigned b = absbits4(rz[2 * r + h]); mz = b > mz ? b : mz;
      }
    }
    wg_publish_max(wmx, 4 * NG, wave8, lane, my, mz);
  };
  auto rescale2 = [&]() { wg_acc_rescale(acc, wg_rescale(wmx, 4 * NG, fsc)); };
  auto split_step = [&]() {
    if (NP == 2) { prep2(); return; }
#ifdef ADDK_WG_DIAG2
    WG_STAMP(sa);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    WG_STAMP(sb);
    dsub[0] += sb - sa;
#endif
    if (st_skip) {
#pragma unroll
      for (int k = 0; k < NYJ; ++k) if (yrow0 + k * YRS < st_skip) ry[k] = zero4();
    }
    if (PRE_Y) {
#pragma unroll
      for (int k = 0; k < NYJ; ++k) wg_split4<NP>(ry[k], py[k]);
    }
#ifdef ADDK_WG_DIAG2
    WG_STAMP(sc);
    dsub[1] += sc - sb;
#endif
    if (PRE_Z) split_z();
  };
  auto write_step = [&]() {
    if (NP == 2) {
      const float sy = wg_pow2(fsc.kfy), sz = wg_pow2(fsc.kfz);
#pragma unroll
      for (int k = 0; k < NYJ; ++k) {
        wg_split4<NP>(wg_mul4(ry[k], sy), py[0]);
        unsigned char* o = Yb + ((k & 1) ? ysw1 : ysw0) + k * (YRS << 5);
#pragma unroll
        for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(o + m * YPL) = py[0][m];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (h == 1 && !zhalf1) continue;
          wg_split4<NP>(wg_mul4(rz[2 * r + h], sz), pz[0]);
          unsigned char* o = Zb + zsw + r * ZROW + h * (H3_KP * 32);
#pragma unroll
          for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(o + m * ZPL) = pz[0][m];
        }
      return;
    }
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      if (!PRE_Y) wg_split4<NP>(ry[k], py[k]);
      unsigned char* o = Yb + ((k & 1) ? ysw1 : ysw0) + k * (YRS << 5);
#pragma unroll
      for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(o + m * YPL) = py[k][m];
    }
    if (!PRE_Z) { split_z(); return; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 1 && !zhalf1) continue;
        unsigned char* o = Zb + zsw + r * ZROW + h * (H3_KP * 32);
#pragma unroll
        for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(o + m * ZPL) = pz[2 * r + h][m];
      }
  };

#ifdef ADDK_WG_DIAG
  const unsigned long long diag_c0 = __builtin_amdgcn_s_memtime(), diag_r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long dph[5] = {0, 0, 0, 0, 0};
#endif
  const unsigned char* Zg = Zb + grp * ZTILE;
  if (sbeg < send) {
    load_prep(true);
#pragma unroll
    for (int i = 0; i < NIT; ++i) load_item(i);
    split_step();
    if (NP == 2) { __syncthreads(); rescale2(); }
    write_step();
    __syncthreads();
    for (int seg = sbeg; seg < send; ++seg) {
      const bool more = seg + 1 < send;
#ifdef ADDK_WG_DIAG
      WG_STAMP(dt0);
#endif
      load_prep(more);
#ifdef ADDK_WG_DIAG
      WG_STAMP(dt1);
#endif
#pragma unroll
      for (int ks = 0; ks < H3_KP / 32; ++ks) {
        wg_bf16x8 yf[NT][NP];
#pragma unroll
        for (int i = 0; i < NT; ++i) wg_tr_read<NP>(Yb + (wave * NT + i) * YIMG, YPL, ks * 32, lrow, tp, yf[i]);
        wg_bf16x8 zf[2][NP];
        wg_tr_read<NP>(Zg, ZPL, ks * 32, lrow, tp, zf[0]);                              // tap 0: patch row 0, shift 0
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          load_item(ks * 9 + tap);
          if (tap + 1 < 9) wg_tr_read<NP>(Zg + ((tap + 1) / 3) * ZROW, ZPL, ks * 32 + ((tap + 1) % 3) * d, lrow, tp, zf[(tap + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
          wg_terms<NP>(acc, tap, yf, zf[tap & 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#ifdef ADDK_WG_DIAG
      WG_STAMP(dt2);
#endif
      if (more) split_step();
#ifdef ADDK_WG_DIAG
      WG_STAMP(dt3);
#endif
      __syncthreads();
#ifdef ADDK_WG_DIAG
      WG_STAMP(dt4);
#endif
      if (more) { if (NP == 2) rescale2(); write_step(); __syncthreads(); }
#ifdef ADDK_WG_DIAG
      WG_STAMP(dt5);
      dph[0] += dt1 - dt0; dph[1] += dt2 - dt1; dph[2] += dt3 - dt2; dph[3] += dt4 - dt3; dph[4] += dt5 - dt4;
#endif
    }
  }
#ifdef ADDK_WG_DIAG
  if (lane == 0) {
    unsigned long long* dslot = g_wg_diag[(blockIdx.x * 4 + wave8) & 63];
    atomicAdd(&dslot[0], __builtin_amdgcn_s_memtime() - diag_c0); atomicAdd(&dslot[1], __builtin_amdgcn_s_memrealtime() - diag_r0); atomicAdd(&dslot[2], 1ull);
    for (int i = 0; i < 5; ++i) atomicAdd(&dslot[3 + i], dph[i]);
#ifdef ADDK_WG_DIAG2
    atomicAdd(&dslot[1], 0ull); atomicAdd(&g_wg_diag2[(blockIdx.x * 4 + wave8) & 63][0], dsub[0]); atomicAdd(&g_wg_diag2[(blockIdx.x * 4 + wave8) & 63][1], dsub[1]);
#endif
  }
#endif
  const int C = p.src.C;
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * 9 * C;
  const int c = c0 + 16 * grp + li;
  if (NP == 2) {                       // the two operand scales leave the partial tile (exact; one after the other)
    const float iy = wg_pow2(254 - fsc.kfy), iz = wg_pow2(254 - fsc.kfz);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < 9; ++j) acc[i][j] = acc[i][j] * iy * iz;
  }
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cow = co0 + (wave * NT + i) * 16 + kq * 4 + r;
      if (cow < p.Cout && c < C) {
        gfloat* o = wsb + (long)cow * 9 * C + c;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) o[tap * C] = acc[i][tap][r];
      }
    }
}
// [r4] The same arithmetic and LDS images for the wide 1x1 heads (ASPP's 1x1 branch and its 1280 -> 256 concat conv, 256 <- 256..400 channels at
// 64x128: aspp_train.py:34-58): no halo, so the nine accumulator "taps" of wgrad_h3b_kernel become FOUR 16-channel input tiles per workgroup
// (128 output x 64 input channels, 96 MFMA per wave and 64-pixel segment).  These weight gradients ran on the fp32 MFMA kernel (wgrad_os_kernel<4,2>:
// 11.9 GF per exit in 200 us = 60 TFLOP/s) while their forward and data gradient already used the split-bf16 kernel.
template <bool BATCH, int NP>
__global__ void __launch_bounds__(256, 2) wgrad_h1b_kernel(const WgK pv, const WgK* __restrict__ ops, const int4* __restrict__ work) {
  int op, blk_x, blk_y;
  const WgK p = wg_block<BATCH>(pv, ops, work, op, blk_x, blk_y);
  constexpr int NT = 2, TP = H1_TP, BCO = 64 * NT, YT = BCO / 16, YQ = BCO / 4, YRS = 256 / YQ, NYJ = H3_KP / YRS;
  constexpr int YIMG = H3_KP * 32 + 32;                              // a [64 px][16 ch] bf16 tile image, 32 bytes off the bank period (see wgrad_h3b_kernel)
  constexpr int YPL = YT * YIMG, ZPL = TP * YIMG;
  constexpr int NIT = NYJ + TP;
  extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];
  unsigned char* Yb = wsm;                                           // [NP][YT][64 px][16 co]
  unsigned char* Zb = wsm + NP * YPL;                                // [NP][TP][64 px][16 ci]
  unsigned* wmx = reinterpret_cast<unsigned*>(wsm + NP * (YPL + ZPL));      // NP = 2: [2][4] the waves' largest magnitudes of the segment being staged (wgrad_h3b_kernel)
  WgScale fsc = {0, 0};
  const int t = threadIdx.x, lane = t & 63, li = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int zt = blk_x % p.nzt, yt = blk_x / p.nzt;
  const int co0 = yt * BCO, c0 = zt * 16 * TP;
  const int spr = (p.OW + H3_KP - 1) / H3_KP;
  const int nseg = p.N * p.OH * spr;
  const int sbeg = blk_y * p.chunkP;
  int send = sbeg + p.chunkP; if (send > nseg) send = nseg;
  // staging geometry: thread constants + segment scalars (wgrad_h3b_kernel); the activation tile needs no row / column validity, only the channel tail
  const int yq = t & (YQ - 1), yrow0 = t / YQ;
  const int co = co0 + 4 * yq;
  const unsigned yoff = ((unsigned)yrow0 * (unsigned)p.lddy + (unsigned)co) * 4u;
  const long ystep = (long)YRS * p.lddy;
  const int ytile = (yq >> 2) * YIMG + 8 * (yq & 3);
  const int ysw0 = ytile + wg_prow(yrow0), ysw1 = ytile + wg_prow(yrow0 + YRS) - (YRS << 5);
  const int zq = t & 3, zj0 = t >> 2;
  const int zsw = wg_prow(zj0) + 8 * zq;
  unsigned zoffk[TP]; unsigned zvalid = 0;
  float4 za[TP], zb[TP];
  const bool zrelu = p.src.relu != 0, zaff = p.src.a != nullptr;
#pragma unroll
  for (int k = 0; k < TP; ++k) {
    const int zc = c0 + 16 * k + 4 * zq;
    const bool ok = zc < p.src.C;                                   // whole quads: C % 4 == 0 (h1_ok)
    zvalid |= (ok ? 1u : 0u) << k;
    zoffk[k] = ok ? ((unsigned)zj0 * (unsigned)p.src.ld + (unsigned)zc) * 4u : 0u;
    za[k] = make_float4(1.f, 1.f, 1.f, 1.f); zb[k] = zero4();
    if (zaff && ok) { za[k] = ld4(p.src.a + zc); zb[k] = ld4(p.src.b + zc); }
  }
  const int tq = li >> 2, tp = li & 3;
  const int lrow = 8 * kq + tq;
  f32x4 acc[NT][TP];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 ry[NYJ], rz[TP];
  int l_sx, l_oh, l_n, c_sx, c_oh, c_n;
  { const int rowid = sbeg / spr; l_sx = sbeg - rowid * spr; l_n = rowid / p.OH; l_oh = rowid - l_n * p.OH; c_sx = l_sx; c_oh = l_oh; c_n = l_n; }
  const float* yseg = p.dy; const float* zseg = p.src.x;
  int st_skip = 0;
  auto load_prep = [&](bool next) {
    if (next) { c_sx = l_sx; c_oh = l_oh; c_n = l_n; if (++l_sx == spr) { l_sx = 0; if (++l_oh == p.OH) { l_oh = 0; ++l_n; } } }
    int ow0 = c_sx * H3_KP;
    st_skip = ow0 + H3_KP - p.OW; if (st_skip < 0) st_skip = 0;      // the last segment of an image row is moved left; the pixels it shares get dy = 0
    ow0 -= st_skip;
    const long pix = ((long)c_n * p.OH + c_oh) * p.OW + ow0;
    yseg = p.dy + pix * p.lddy;
    zseg = p.src.x + pix * p.src.ld;
  };
  auto load_item = [&](int i) {
    if (i < NYJ) ry[i] = ld4so(yseg + i * ystep, yoff);
    else if (i < NIT) rz[i - NYJ] = ld4so(zseg, zoffk[i - NYJ]);
  };
  auto zpro = [&](int k) {      // (wg_zpro, written out: with it the NP = 3 form gets another register allocation)
    float4 v = rz[k];
    if (zaff) { v.x = fmaf(za[k].x, v.x, zb[k].x); v.y = fmaf(za[k].y, v.y, zb[k].y); v.z = fmaf(za[k].z, v.z, zb[k].z); v.w = fmaf(za[k].w, v.w, zb[k].w); }
    if (zrelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    const bool ok = (zvalid >> k) & 1u;
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
    return v;
  };
  auto prep2 = [&]() {                                               // NP = 2: masks and prologue in place, the wave's maxima to LDS (in front of the barrier)
    unsigned my = 0, mz = 0;
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      if (st_skip && yrow0 + k * YRS < st_skip) ry[k] = zero4();
      const unsigned b = absbits4(ry[k]); my = b > my ? b : my;
    }
#pragma unroll
    for (int k = 0; k < TP; ++k) { rz[k] = zpro(k); const unsigned b = absbits4(rz[k]); mz = b > mz ? b : mz; }
    wg_publish_max(wmx, 4, wave, lane, my, mz);
  };
  auto rescale2 = [&]() { wg_acc_rescale(acc, wg_rescale(wmx, 4, fsc)); };
  auto store_step = [&]() {
    const float sy = NP == 2 ? wg_pow2(fsc.kfy) : 1.f, sz = NP == 2 ? wg_pow2(fsc.kfz) : 1.f;
    if (NP != 2 && st_skip) {
#pragma unroll
      for (int k = 0; k < NYJ; ++k) if (yrow0 + k * YRS < st_skip) ry[k] = zero4();
    }
#pragma unroll
    for (int k = 0; k < NYJ; ++k) {
      uint2 pl[NP];
      wg_split4<NP>(NP == 2 ? wg_mul4(ry[k], sy) : ry[k], pl);
      unsigned char* o = Yb + ((k & 1) ? ysw1 : ysw0) + k * (YRS << 5);
#pragma unroll
      for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(o + m * YPL) = pl[m];
    }
#pragma unroll
    for (int k = 0; k < TP; ++k) {
      const float4 v = NP == 2 ? wg_mul4(rz[k], sz) : zpro(k);
      uint2 pl[NP];
      wg_split4<NP>(v, pl);
      unsigned char* o = Zb + k * YIMG + zsw;
#pragma unroll
      for (int m = 0; m < NP; ++m) *reinterpret_cast<uint2*>(o + m * ZPL) = pl[m];
    }
  };
  if (sbeg < send) {
    load_prep(true);
#pragma unroll
    for (int i = 0; i < NIT; ++i) load_item(i);
    if (NP == 2) { prep2(); __syncthreads(); rescale2(); }
    store_step();
    __syncthreads();
    for (int seg = sbeg; seg < send; ++seg) {
      const bool more = seg + 1 < send;
      load_prep(more);
#pragma unroll
      for (int ks = 0; ks < H3_KP / 32; ++ks) {
        wg_bf16x8 yf[NT][NP];
#pragma unroll
        for (int i = 0; i < NT; ++i) wg_tr_read<NP>(Yb + (wave * NT + i) * YIMG, YPL, ks * 32, lrow, tp, yf[i]);
        wg_bf16x8 zf[2][NP];
        wg_tr_read<NP>(Zb, ZPL, ks * 32, lrow, tp, zf[0]);
#pragma unroll
        for (int j = 0; j < TP; ++j) {
          load_item(2 * (ks * TP + j)); load_item(2 * (ks * TP + j) + 1);      // the next segment's loads, two per input tile (NIT <= 16)
          if (j + 1 < TP) wg_tr_read<NP>(Zb + (j + 1) * YIMG, ZPL, ks * 32, lrow, tp, zf[(j + 1) & 1]);
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
  gfloat* wsb = (gfloat*)p.ws + (long)blk_y * p.Cout * C;
  if (NP == 2) {
    const float iy = wg_pow2(254 - fsc.kfy), iz = wg_pow2(254 - fsc.kfz);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < TP; ++j) acc[i][j] = acc[i][j] * iy * iz;
  }
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cow = co0 + (wave * NT + i) * 16 + kq * 4 + r;
#pragma unroll
      for (int j = 0; j < TP; ++j) {
        const int c = c0 + 16 * j + li;
        if (cow < p.Cout && c < C) wsb[(long)cow * C + c] = acc[i][j][r];
      }
    }
}

template <int NT, int NG, bool B> WgVariant wg_h3b(int np) {
  return np == 3 ? wg_dyn_lds<wgrad_h3b_kernel<NT, B, 3, NG>>(256 * NG, wg_h3b_lds(NT, 3, NG))
                 : wg_dyn_lds<wgrad_h3b_kernel<NT, B, 2, NG>>(256 * NG, wg_h3b_lds(NT, 2, NG));
}
}  // namespace

// In the split-precision modes (np = 2, 3) kind 5 runs wgrad_h3b_kernel (stem1 0.76 -> 0.61 ms alone); NG = 2 exists there only.
template <bool B> static WgVariant wg_h3_any(int cty, int ctz, int np) {
  if (cty != 4 && cty != 8) return {nullptr, 256, 0};
  if (!np) return {cty == 8 ? wgrad_h3_kernel<2, B> : wgrad_h3_kernel<1, B>, 256, 0};
  if (cty == 8) return ctz == 2 ? wg_h3b<2, 2, B>(np) : wg_h3b<2, 1, B>(np);
  return ctz == 2 ? wg_h3b<1, 2, B>(np) : wg_h3b<1, 1, B>(np);
}
WgVariant wg_variant_h3(bool batch, int cty, int ctz, int np) { return batch ? wg_h3_any<true>(cty, ctz, np) : wg_h3_any<false>(cty, ctz, np); }
template <bool B> static WgVariant wg_h1_any(int np) {
  return np == 3 ? wg_dyn_lds<wgrad_h1b_kernel<B, 3>>(256, wg_h1b_lds(3)) : wg_dyn_lds<wgrad_h1b_kernel<B, 2>>(256, wg_h1b_lds(2));
}
WgVariant wg_variant_h1(bool batch, int np) { return batch ? wg_h1_any<true>(np) : wg_h1_any<false>(np); }
