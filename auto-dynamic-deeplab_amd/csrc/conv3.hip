// Halo-patch form of the wide 3x3, stride-1, 'same'-padded convolutions (decoder, ASPP dilated branches, stem1),
// forward and data gradient, on the fp32 matrix cores of gfx950 (v_mfma_f32_16x16x4_f32).
//
// The generic implicit-GEMM kernel (conv.hip) walks K as (tap, 32-channel chunk) and re-stages the pixel tile for every
// tap: 9 global loads + 9 BatchNorm/ReLU prologues per input element, two barriers per 128 MFMAs, and the staging phase
// does not overlap the MFMA phase (measured: 454 us of staging + 714 us of MFMAs ~ the 1072 us of the decoder conv).
// Here a block owns 128 consecutive pixels of ONE output row and 64/128 output channels, and walks K in 16-channel
// chunks.  Per chunk it stages the three input rows oh-d, oh, oh+d ([3][128+2d px][16 ch], prologue applied once, zero
// padding after it) in LDS and runs all nine taps from that patch: one global load + one prologue per input element
// and 2 barriers per 576 MFMAs per wave.  The weights never touch LDS: a small pack kernel rewrites them per launch
// into MFMA-fragment order ([column block][chunk*9+tap][16-col tile][lane][4 k-slots]) so that a wave fetches the
// fragments of one tap with CT coalesced 16-byte loads (L1/L2 hits: every block reads the same stream), one tap ahead
// of their use.  The data gradient is the same kernel over dy with the packed weights transposed and tap-mirrored.
//
// Reference call sites: decoder.py:17-27 (3x3 conv+BN+ReLU x2), aspp_train.py:20-41 (dilated 3x3 branches),
// ADD.py:220-232 (stem1); autograd of nn.Conv2d for the data gradient.
#include "conv3b.h"

namespace {

constexpr int C3_RS = 20;                  // floats per patch pixel in LDS (16 + 4: ds_read_b64 fragment reads hit 64 distinct banks per half-wave)
constexpr int C3_MAXCH = 64;               // chunks per launch (K <= 1024 channels)
// widest patch row: 3x3 up to dilation 18 (ASPP), 5x5 up to dilation 2 (the cells' dil_conv_5x5)
constexpr int c3_pwmax(int ks) { return ks == 3 ? C3_BP + 2 * 18 : C3_BP + 4 * 2; }
constexpr int c3_maxdil(int ks) { return ks == 3 ? 18 : 2; }


struct PackK {
  const float* w; int ldw, cin_total;
  int mode;                 // fwd: rows = co, K = input channels; dgrad: rows = input channels, K = co
  int Cn;                   // GEMM N extent (rows of the packed tiles)
  int w_choff;              // dgrad: channel offset of the destination source inside a tap
  int nchunks, bct, taps;
  int cbase[C3_MAXCH];      // first K index of the chunk (fwd: absolute channel inside a tap; dgrad: co)
  int cvalid[C3_MAXCH];     // valid K entries in the chunk (<= 16)
  float* out;
  int planes;               // 0: fp32 fragments for conv3_kernel; 2 / 3: bf16 planes (h, m[, l]) in 32-row fragment order for conv3b_kernel
  int dil_odd;              // conv3b checkerboard accumulation (see conv3b_kernel): 1 = odd dilation, taps with odd (kh + kw) carry a minus sign;
                            // 2 = stride 2, the taps of kernel column 2 carry it
  int s2d;                  // conv3b: 1 = the four parity-class packs of the stride-2 data gradient (c3b_pack_s2d_body); 2 = the 16-wide-tile kernel's pack (c3n_pack_body)
  int sbase[C3_MAXCH];      // s2d == 2: first K-step of the chunk (conv3n.hip: two taps x 16 channels per step, four taps x 8 for a chunk of <= 8 channels)
  int wrows;                // rows of the whole weight tensor [wrows][ldw] behind `w` (the amax pass scans it contiguously)
  float* amax;              // planes == 2 (split-fp16, conv3b.h): the 128-float trailer of the pack buffer — [0..63] the amax pass's per-workgroup maxima of |w|,
                            // [64] = 2^-kw for the kernel's epilogue (C3K.wsc), [65] = 2^kw
};
constexpr int C3_AMAX_WG = 64;             // workgroups of the amax pass = partial maxima in the trailer
constexpr int C3_TRAILER = 128;            // floats

// out[colblk][T = chunk*taps + tap][tile i][lane][m]  =  W(row = colblk*BC + i*16 + li, tap, k = 8*(m>>1) + 2*kq + (m&1))
__device__ __forceinline__ void c3_pack_body(const PackK& p, long first, long stride);
__global__ void __launch_bounds__(256) c3_pack_kernel(const PackK p) { c3_pack_body(p, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256); }
// all packs of a plan in one launch at the start of the step (the weights only change in the optimizer): block (x, y) works on descriptor y
__global__ void __launch_bounds__(256) c3_pack_batch_kernel(const PackK* __restrict__ descs) {
  c3_pack_body(descs[blockIdx.y], (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256);
}
__device__ __forceinline__ void c3b_pack_body(const PackK& p, long first, long stride);
// split-fp16 packs (planes == 2): the pass in front of the pack scans the convolution's WHOLE weight tensor (contiguous, coalesced: forward and data-gradient
// packs of one convolution, and the data gradients towards its several sources, get the same scale) and leaves the largest |w| each of its C3_AMAX_WG
// workgroups saw in the trailer (max is order-independent: bit-reproducible); every pack thread folds the 64 partials into the tensor's scale 2^kw itself
__device__ __forceinline__ void c3_amax_body(const PackK& p) {
  if (p.planes != 2) return;
  float m = 0.f;
  const long n = (long)p.wrows * p.ldw;
  const gfloat* w = (const gfloat*)p.w;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(w[i]));
  __shared__ unsigned wm[4];
  const unsigned b = wave_umax(__float_as_uint(m));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned r = wm[0];
    for (int i = 1; i < 4; ++i) r = wm[i] > r ? wm[i] : r;
    p.amax[blockIdx.x] = __uint_as_float(r);
  }
}
__global__ void __launch_bounds__(256) c3_pack_amax_kernel(const PackK p) { c3_amax_body(p); }
__global__ void __launch_bounds__(256) c3_pack_amax_batch_kernel(const PackK* __restrict__ descs) { c3_amax_body(descs[blockIdx.y]); }
// scale of a split-fp16 pack from the amax pass's partials; the first thread of the pack leaves its inverse for the convolution's epilogue
__device__ __forceinline__ float c3_pack_scale(const PackK& p, long first) {
  if (p.planes != 2) return 1.f;
  float m = 0.f;
  const float4* q = reinterpret_cast<const float4*>(p.amax);
#pragma unroll
  for (int i = 0; i < C3_AMAX_WG / 4; ++i) { const float4 v = q[i]; m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }
  const int kf = f16_scale_field(__float_as_uint(m));
  if (first == 0) { p.amax[C3_AMAX_WG] = __uint_as_float((unsigned)(254 - kf) << 23); p.amax[C3_AMAX_WG + 1] = __uint_as_float((unsigned)kf << 23); }
  return __uint_as_float((unsigned)kf << 23);
}
__device__ __forceinline__ void c3_pack_body(const PackK& p, long first, long stride) {
  if (p.planes) { c3b_pack_body(p, first, stride); return; }
  const int BC = 16 * p.bct;
  const int nT = p.nchunks * p.taps;
  const long per_blk = (long)nT * p.bct * 256;
  const long total = (long)((p.Cn + BC - 1) / BC) * per_blk;
  for (long idx = first; idx < total; idx += stride) {
    const int m = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
    long r = idx >> 8;
    const int i = (int)(r % p.bct); r /= p.bct;
    const int T = (int)(r % nT); const int blk = (int)(r / nT);
    const int chunk = T / p.taps, tap = T - chunk * p.taps;
    const int li = lane & 15, kq = lane >> 4;
    const int row = blk * BC + i * 16 + li;
    const int kk = 8 * (m >> 1) + 2 * kq + (m & 1);
    float v = 0.f;
    if (row < p.Cn && kk < p.cvalid[chunk]) {
      if (p.mode == MODE_FWD) v = p.w[(long)row * p.ldw + (long)tap * p.cin_total + p.cbase[chunk] + kk];
      else                    v = p.w[(long)(p.cbase[chunk] + kk) * p.ldw + (long)(p.taps - 1 - tap) * p.cin_total + p.w_choff + row];
    }
    p.out[idx] = v;
  }
}

template <int BCT, int KS, int MODE>
__global__ void __launch_bounds__(256, 2) conv3_kernel(const C3K p) {
  constexpr int BC = 16 * BCT;
  constexpr int TAPS = KS * KS, HK = KS / 2;
  constexpr int C3_PWMAX = c3_pwmax(KS);
  constexpr int C3_NS = (KS * C3_PWMAX * 4 + 255) / 256;   // 16-byte patch slots per thread
  constexpr int WC = (BCT == 8 || BCT == 4) ? 2 : 1;      // waves across output channels
  constexpr int WP = 4 / WC;                // waves across pixels
  constexpr int PT = 8 / WP;                // 16-pixel tiles per wave
  constexpr int CT = BCT / WC;              // 16-channel tiles per wave
  __shared__ __attribute__((aligned(16))) float Ps[KS * C3_PWMAX * C3_RS];
  __shared__ double red[WP][BC][2];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int wc = wave % WC, wpx = wave / WC;
  const int n0 = blockIdx.y * BC;
  const int d = p.dil, PW = C3_BP + (KS - 1) * d;
  double tot0 = 0.0, tot1 = 0.0;

  // fixed patch-slot geometry, packed to one register per slot: slot -> (row r | patch column pj << 3); r == KS: outside the patch
  const int q = t & 3;
  int geo[C3_NS];
#pragma unroll
  for (int k = 0; k < C3_NS; ++k) {
    const int pix = (t + 256 * k) >> 2;
    int r = pix / PW; const int pj = pix - r * PW;
    if (r > KS) r = KS;
    geo[k] = r | (pj << 3);
  }
  // fragment read bases (bytes are implied by float indexing): pixel (wpx*PT*16 + li) of patch row 0, k pair 2*kq, per kw
  int xb[KS];
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) xb[kw] = (wpx * PT * 16 + li + kw * d) * C3_RS + 2 * kq;
  const float4* wpl = reinterpret_cast<const float4*>(p.wp + (long)blockIdx.y * p.wp_blk) + (long)wc * CT * 64 + lane;
  const int nT = p.nT;

  const int tpx = p.ntiles >> 3;
  const bool swz = (p.ntiles & 7) == 0 && p.ntiles >= 64;
  for (int tlin = blockIdx.x; tlin < p.ntiles; tlin += gridDim.x) {
    const int tile = swz ? (tlin & 7) * tpx + (tlin >> 3) : tlin;
    const int rowid = tile / p.spr, sx = tile - rowid * p.spr;
    const int n = rowid / p.H, oh = rowid - n * p.H;
    const int ow0 = sx * C3_BP;
    // per-tile validity of the slots (image borders)
    unsigned vmask = 0;
    const int pbase = (n * p.H + oh - HK * d) * p.W + ow0 - HK * d;      // pixel index of patch (row 0, column 0)
#pragma unroll
    for (int k = 0; k < C3_NS; ++k) {
      const int r = geo[k] & 7, pj = geo[k] >> 3;
      const int ih = oh + (r - HK) * d, iw = ow0 - HK * d + pj;
      const bool ok = r < KS && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      vmask |= (ok ? 1u : 0u) << k;
    }

    f32x4 acc[CT][PT];
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
      for (int j = 0; j < PT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    float4 ra[C3_NS];
    float4 pa = make_float4(1.f, 1.f, 1.f, 1.f), pb = zero4();
    bool prelu = false, pch = false;
    auto load_patch = [&](int s_, int c0_) {      // branch-free: masked slots read the source base and are zeroed at store time
      const addk_src S = p.src[s_];
      const int c = c0_ + 4 * q;
      pch = c < S.C;
      prelu = S.relu != 0;
      pa = make_float4(1.f, 1.f, 1.f, 1.f); pb = zero4();
      if (S.a && pch) { pa = ld4(S.a + c); pb = ld4(S.b + c); }
      const float* sb = S.x + (pch ? c : 0);
#pragma unroll
      for (int k = 0; k < C3_NS; ++k) {
        const int r = geo[k] & 7, pj = geo[k] >> 3;
        const int po = ((vmask >> k) & 1u) ? pbase + r * d * p.W + pj : 0;
        ra[k] = ld4(sb + (long)po * S.ld);
      }
    };
    auto store_patch = [&]() {
#pragma unroll
      for (int k = 0; k < C3_NS; ++k) {
        float4 v = ra[k];
        v.x = fmaf(pa.x, v.x, pb.x); v.y = fmaf(pa.y, v.y, pb.y); v.z = fmaf(pa.z, v.z, pb.z); v.w = fmaf(pa.w, v.w, pb.w);
        if (prelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        const bool ok = pch && ((vmask >> k) & 1u);
        v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
        const int r = geo[k] & 7, pj = geo[k] >> 3;
        if (r < KS) lds_st4(&Ps[(r * C3_PWMAX + pj) * C3_RS + 4 * q], v);
      }
    };

    // weight fragments: two register sets, the next tap's fragments are fetched while the current tap's MFMAs issue
    float4 wr[2][CT];
    auto load_w = [&](int T, float4* dst) {
      const int Tc = T < nT ? T : nT - 1;
      const float4* src = wpl + (long)Tc * (BCT * 64);
#pragma unroll
      for (int i = 0; i < CT; ++i) dst[i] = src[i * 64];
    };
    // pixel fragments: one buffer per half of the 16-channel chunk (k 0-7 / 8-15), read one half ahead
    float2 xf[2][PT];
    auto read_x = [&](int tap, int h, float2* x) {
      const int kh = tap / KS, kw = tap - kh * KS;
      const float* b = &Ps[xb[kw] + kh * C3_PWMAX * C3_RS + 8 * h];
#pragma unroll
      for (int j = 0; j < PT; ++j) x[j] = *reinterpret_cast<const float2*>(b + j * 16 * C3_RS);
    };
    auto mma = [&](const float4* w, int h, const float2* x) {
#pragma unroll
      for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(h ? w[i].z : w[i].x, x[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(h ? w[i].w : w[i].y, x[j].y, acc[i][j], 0, 0, 0);
    };

    int s = 0, c0 = 0, T0 = 0;
    load_w(0, wr[0]);
    load_patch(0, 0);
    store_patch();
    __syncthreads();
    while (true) {
      int s2 = s, c2 = c0 + C3_BK;
      if (c2 >= p.src[s].C) { c2 = 0; ++s2; }
      const bool more = s2 < p.nsrc;
      read_x(0, 0, xf[0]);
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) {
        load_w(T0 + tap + 1, wr[(tap + 1) & 1]);
        if (tap == 0 && more) load_patch(s2, c2);
        read_x(tap, 1, xf[1]);
        __builtin_amdgcn_sched_barrier(0);
        mma(wr[tap & 1], 0, xf[0]);
        __builtin_amdgcn_sched_barrier(0);
        if (tap + 1 < TAPS) read_x(tap + 1, 0, xf[0]);
        __builtin_amdgcn_sched_barrier(0);
        mma(wr[tap & 1], 1, xf[1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      T0 += TAPS;
#pragma unroll
      for (int i = 0; i < CT; ++i) wr[0][i] = wr[1][i];      // odd tap count: the set fetched during the last tap is next chunk's tap 0
      __syncthreads();
      if (!more) break;
      s = s2; c0 = c2;
      store_patch();
      __syncthreads();
    }

    // ---- epilogue (same contract as conv.hip) ----
    const bool want_red = p.slab != nullptr;
#pragma unroll
    for (int i = 0; i < CT; ++i) {
      const int col = (wc * CT + i) * 16 + kq * 4;
      const int c = n0 + col;
      const int nrem = p.Cn - c;
      double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < PT; ++j) {
        const int lp = (wpx * PT + j) * 16 + li;
        const long pp = (long)rowid * p.W + ow0 + lp;
        const bool pv = ow0 + lp < p.W && nrem > 0;
        float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        if (MODE == MODE_FWD) {
          if (pv) {
            if (p.bias) { float4 b = ld4g(p.bias + c, nrem, false); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
            if (p.bias_n) {
              float4 b = ld4g(p.bias_n + (long)n * p.Cn + c, nrem, false);
              v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
            }
            st4g(p.y + pp * p.ldy + c, v, nrem, p.vecY);
            if (want_red) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                double f = (e < nrem) ? (double)get4(v, e) : 0.0;
                s1[e] += f; s2v[e] += f * f;
              }
            }
          }
        } else {
          if (pv) {
            float4 x = ld4g(p.dst.x + pp * p.dst.ld + c, nrem, p.vecY);
            float4 av = make_float4(1.f, 1.f, 1.f, 1.f), bv = zero4();
            if (p.dst.a) { av = ld4g(p.dst.a + c, nrem, p.vecY); bv = ld4g(p.dst.b + c, nrem, p.vecY); }
            float4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float xe = get4(x, e), ae = get4(av, e), be = get4(bv, e), dz = get4(v, e);
              bool m = (e < nrem) && (!p.dst.relu || fmaf(ae, xe, be) > 0.f);
              set4(g, e, m ? dz * ae : 0.f);
              if (want_red && m) { s1[e] += (double)dz * (double)xe; s2v[e] += (double)dz; }
            }
            float* gp = p.y + pp * p.ldy + c;
            if (p.accumulate) { float4 o = ld4g(gp, nrem, p.vecY); g.x += o.x; g.y += o.y; g.z += o.z; g.w += o.w; }
            st4g(gp, g, nrem, p.vecY);
          }
        }
      }
      if (want_red) {
        if (p.red32) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float a = (float)s1[e], b = (float)s2v[e];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); }
            if (li == 0) { red[wpx][col + e][0] = a; red[wpx][col + e][1] = b; }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            double a = s1[e], b = s2v[e];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); }
            if (li == 0) { red[wpx][col + e][0] = a; red[wpx][col + e][1] = b; }
          }
        }
      }
    }
    if (want_red) {
      __syncthreads();
      if (t < BC) {
#pragma unroll
        for (int w = 0; w < WP; ++w) { tot0 += red[w][t][0]; tot1 += red[w][t][1]; }
      }
      __syncthreads();
    }
  }
  if (p.slab && t < BC && n0 + t < p.Cn) {
    double* o = p.slab + ((long)blockIdx.x * p.slab_ld + n0 + t) * 2;
    o[0] = tot0; o[1] = tot1;
  }
}


// packed weights: out (16-byte units) [colblk][T = chunk*taps + tap][tile (wave) i][plane][lane] = 8 bf16:
//   W(row = colblk*32*bct + i*32 + (lane & 31), tap, k = 8*(lane >> 5) + j), j = 0..7       (bct = 32-row tiles per block)
// Stride-2 data gradient (3x3, pad 1): input pixel (2a + pi, 2b + pj) collects dy(a + th, b + tw) W[kh][kw] over th <= pi, tw <= pj with
// kh = 1 for pi = 0, else {2, 0}[th] (same for columns) — 1, 2, 2, 4 of the nine taps per parity class.  Four packs back to back, class
// c = 2 pi + pj at (taps of the classes before) * unit, each [colblk][chunk * tc + tap][tile][plane][lane]; tap (th, tw) carries
// (-1)^(th + tw), its share of the checkerboard sign over the class grid (a, b).
__device__ __forceinline__ void c3b_pack_s2d_body(const PackK& p, long first, long stride) {
  const int BC = 32 * p.bct, NP = p.planes;
  const float wsc = c3_pack_scale(p, first);
  const long unit = (long)((p.Cn + BC - 1) / BC) * p.nchunks * p.bct * 64;          // lanes per tap
  uint4* out = reinterpret_cast<uint4*>(p.out);
  for (long idx = first; idx < 9 * unit; idx += stride) {
    const int u = (int)(idx / unit);
    const int cls = u < 1 ? 0 : u < 3 ? 1 : u < 5 ? 2 : 3, pre = cls == 0 ? 0 : cls == 1 ? 1 : cls == 2 ? 3 : 5;
    const int pi = cls >> 1, pj = cls & 1, twn = 1 + pj, tc = (1 + pi) * twn;
    long r = idx - pre * unit;
    const int lane = (int)(r & 63); r >>= 6;
    const int i = (int)(r % p.bct); r /= p.bct;
    const int nT = p.nchunks * tc;
    const int T = (int)(r % nT); const int blk = (int)(r / nT);
    const int chunk = T / tc, tap = T - chunk * tc;
    const int th = tap / twn, tw = tap - th * twn;
    const int kh = pi ? (th ? 0 : 2) : 1, kw = pj ? (tw ? 0 : 2) : 1;
    const int row = blk * BC + i * 32 + (lane & 31), k0 = 8 * (lane >> 5);
    unsigned b[3][8];
    float vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = 0.f;
      const int kk = k0 + j;
      if (row < p.Cn && kk < p.cvalid[chunk]) v = p.w[(long)(p.cbase[chunk] + kk) * p.ldw + (long)(kh * 3 + kw) * p.cin_total + p.w_choff + row];
      if ((th + tw) & 1) v = -v;
      vv[j] = v * wsc;
#pragma unroll
      for (int k = 0; k < 3; ++k) { b[k][j] = bf16_hi(v); v = v - bf16_f(b[k][j]); }
    }
    uint4* o = out + pre * unit * NP + (((long)blk * nT + T) * p.bct + i) * NP * 64 + lane;
    if (NP == 2) { split8h(vv, o[0], o[64]); continue; }
    for (int k = 0; k < NP; ++k)
      o[k * 64] = make_uint4(b[k][0] | (b[k][1] << 16), b[k][2] | (b[k][3] << 16), b[k][4] | (b[k][5] << 16), b[k][6] | (b[k][7] << 16));
  }
}

// conv3n_kernel (conv3n.hip): out (16-byte units) [K-step T][16-row tile i (3)][plane][lane] = 8 bf16: row co = 16 i + lane % 16; lane group g = lane / 16 holds, in a
// pair step, channels 8 (g & 1) .. + 7 of tap 2 st + (g >> 1), in a quad step (chunk of <= 8 channels) channels 0..7 of tap 4 st + g; taps beyond the kernel: zeros
__device__ __forceinline__ void c3n_pack_body(const PackK& p, long first, long stride) {
  const int NP = p.planes;
  const float wsc = c3_pack_scale(p, first);
  const int ks = p.taps == 9 ? 3 : 5;
  const int last = p.nchunks - 1;
  const int steps = p.sbase[last] + (p.cvalid[last] <= 8 ? (p.taps + 3) / 4 : (p.taps + 1) / 2);
  uint4* out = reinterpret_cast<uint4*>(p.out);
  for (long idx = first; idx < (long)steps * 3 * 64; idx += stride) {
    const int lane = (int)(idx & 63);
    const int r = (int)(idx >> 6);
    const int i = r % 3, T = r / 3;
    int chunk = 0;
    while (chunk < last && p.sbase[chunk + 1] <= T) ++chunk;
    const int st = T - p.sbase[chunk];
    const bool quad = p.cvalid[chunk] <= 8;
    const int g = lane >> 4, row = 16 * i + (lane & 15);
    const int tap = quad ? 4 * st + g : 2 * st + (g >> 1), kc0 = quad ? 0 : 8 * (g & 1);
    const bool flip = p.dil_odd == 1 && tap < p.taps && (((tap / ks) + (tap % ks)) & 1) != 0;
    unsigned b[3][8];
    float vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = 0.f;
      const int kk = kc0 + j;
      if (row < p.Cn && tap < p.taps && kk < p.cvalid[chunk]) {
        if (p.mode == MODE_FWD) v = p.w[(long)row * p.ldw + (long)tap * p.cin_total + p.cbase[chunk] + kk];
        else                    v = p.w[(long)(p.cbase[chunk] + kk) * p.ldw + (long)(p.taps - 1 - tap) * p.cin_total + p.w_choff + row];
      }
      if (flip) v = -v;
      vv[j] = v * wsc;
#pragma unroll
      for (int k = 0; k < 3; ++k) { b[k][j] = bf16_hi(v); v = v - bf16_f(b[k][j]); }
    }
    uint4* o = out + ((long)(T * 3 + i) * NP) * 64 + lane;
    if (NP == 2) { split8h(vv, o[0], o[64]); continue; }
    for (int k = 0; k < NP; ++k)
      o[k * 64] = make_uint4(b[k][0] | (b[k][1] << 16), b[k][2] | (b[k][3] << 16), b[k][4] | (b[k][5] << 16), b[k][6] | (b[k][7] << 16));
  }
}

__device__ __forceinline__ void c3b_pack_body(const PackK& p, long first, long stride) {
  if (p.s2d == 2) { c3n_pack_body(p, first, stride); return; }
  if (p.s2d) { c3b_pack_s2d_body(p, first, stride); return; }
  const int BC = 32 * p.bct, NP = p.planes;
  const float wsc = c3_pack_scale(p, first);
  const int nT = p.nchunks * p.taps;
  const long per_blk = (long)nT * p.bct * 64;
  const long total = (long)((p.Cn + BC - 1) / BC) * per_blk;
  uint4* out = reinterpret_cast<uint4*>(p.out);
  for (long idx = first; idx < total; idx += stride) {
    const int lane = (int)(idx & 63);
    long r = idx >> 6;
    const int i = (int)(r % p.bct); r /= p.bct;
    const int T = (int)(r % nT); const int blk = (int)(r / nT);
    const int chunk = T / p.taps, tap = T - chunk * p.taps;
    const int row = blk * BC + i * 32 + (lane & 31), k0 = 8 * (lane >> 5);
    const int ks = p.taps == 9 ? 3 : 5;
    const bool flip = p.dil_odd == 1 ? (((tap / ks) + (tap % ks)) & 1) != 0      // (-1)^((kh+kw) d): the tap's share of the checkerboard sign
                    : p.dil_odd == 2 ? (tap % ks) == 2 : false;
    unsigned b[3][8];
    float vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = 0.f;
      const int kk = k0 + j;
      if (row < p.Cn && kk < p.cvalid[chunk]) {
        if (p.mode == MODE_FWD) v = p.w[(long)row * p.ldw + (long)tap * p.cin_total + p.cbase[chunk] + kk];
        else                    v = p.w[(long)(p.cbase[chunk] + kk) * p.ldw + (long)(p.taps - 1 - tap) * p.cin_total + p.w_choff + row];
      }
      if (flip) v = -v;
      vv[j] = v * wsc;
#pragma unroll
      for (int k = 0; k < 3; ++k) { b[k][j] = bf16_hi(v); v = v - bf16_f(b[k][j]); }
    }
    uint4* o = out + (((long)blk * nT + T) * p.bct + i) * NP * 64 + lane;
    if (NP == 2) { split8h(vv, o[0], o[64]); continue; }
    for (int k = 0; k < NP; ++k)
      o[k * 64] = make_uint4(b[k][0] | (b[k][1] << 16), b[k][2] | (b[k][3] << 16), b[k][4] | (b[k][5] << 16), b[k][6] | (b[k][7] << 16));
  }
}

// 32-row tiles (= waves) per block of the split-bf16 kernel: the count in 3..5 that pads the channel count least (ties: the wider)
int c3b_wc(int Cn, long P) {
  if (Cn <= 64) return 2;                 // two channel tiles; the launch adds the two pixel halves (4 waves, conv3b_kernel PH = 2)
  int best = 4; long bc = -1;
  const int cands[3] = {5, 4, 3};
  for (int i = 0; i < 3; ++i) {
    const long cols = (long)cdiv(Cn, 32 * cands[i]) * 32 * cands[i];
    if (bc < 0 || cols < bc) { bc = cols; best = cands[i]; }
  }
  // 5-wave blocks sit badly on 4 SIMDs (one block per CU at this register count, one SIMD with two waves): 4-wave blocks win
  // up to ~10 % more padded columns (ASPP data gradient, 400 channels: 4 x 128 instead of 3 x 160, 304 -> 200 us)
  if (best == 5 && (long)cdiv(Cn, 128) * 128 * 10 <= bc * 11) best = 4;
  // small maps (160 channels at 32x64): two 3-wave column blocks on half-width tiles instead of one 5-wave block per row
  if (best == 5 && P < 8192) best = 3;
  return best;
}

// bf16 planes of a launch (3: six product terms, 2: three), or 0 = the exact fp32 MFMA kernel.  Every halo launch takes the
// split kernel, the <= 64-channel ones (stem1, the cells' 40-channel dilated convs) on 4-wave blocks = 2 channel tiles x 2
// pixel halves (PH = 2; the first 2-wave form staged 13-22 slots per thread, spilled and was slower than fp32: 125 vs 78 us
// for a 5x5 at 40 channels, now 62).  Accuracy: the network amplifies any 1e-7 perturbation of the stems to 1e-4..1e-3 in the
// whole-network frozen-BatchNorm gradients, so one input draw cannot rank arithmetics — the draw of
// test_add_whole_net_frozen_bn_gradients that once suggested keeping the narrow launches on fp32 (4.9e-4 vs 2.5e-4 median) was
// a sample of that spread: over four more draws at 2x512x1024 split-bf16 everywhere was CLOSER to fp64 than the fp32 kernels
// in all four (median 0.40-0.89x the fp32 oracle's error against 0.84-1.22x; profiles/r02_split_threshold_study.txt).
// addk_set_split_min_channels(n) keeps launches with fewer than n output channels on the fp32 kernel.
int g_c3b_minc = 0;
inline int c3_planes(int mode, int Cn) {
  if (mode == 0 || Cn < g_c3b_minc) return 0;
  if (mode == 3) return Cn >= 192 ? 2 : 3;       // tail_x3: three product terms in the exit heads (ASPP, decoder: 256 / 304 / 400 channels), six elsewhere
  return mode == 2 ? 3 : 2;
}
// Column block (16-channel tiles per block).  128-channel blocks (2x2 waves) for the wide heads when that still
// yields >= 512 blocks and the kernel has that form (the 3x3); otherwise the narrowest of 3/4/5 tiles that pads the channel count
// least (cells: 40 -> 3 tiles, 80 and 160 -> 5 tiles; stem / small ASPP maps: 4 tiles).
int c3_bct(int Cn, long P, int ks, int dir) {
  const long tiles = (P + C3_BP - 1) / C3_BP;
  if (Cn >= 128 && Cn % 128 == 0 && tiles * (Cn / 128) >= 512 && c3_variant_fp32(8, ks, dir).fn) return 8;
  int best = 4; long bc = -1;
  const int cands[3] = {5, 4, 3};
  for (int i = 0; i < 3; ++i) {
    const long cols = (long)cdiv(Cn, 16 * cands[i]) * 16 * cands[i];
    if (bc < 0 || cols < bc) { bc = cols; best = cands[i]; }
  }
  return best;
}
inline int c3n_steps(int taps, int valid) { return valid <= 8 ? (taps + 3) / 4 : (taps + 1) / 2; }

// Does a halo-patch kernel take this geometry?  (H, W: input map; OH, OW: output map of the forward convolution, for both directions)
bool c3_geometry_ok(int mode, int mask, int KH, int KW, int stride, int pad, int dil, int H, int W, int OH, int OW, long P, int Cn, bool fwd) {
  if (!(mask & ADDK_FAST_CONV3)) return false;
  if (KH == 1 && KW == 1) {      // wide pointwise heads (ASPP 1x1, the 1280 -> 256 concat conv): the split kernel as a plain GEMM (KS = 1)
    // (the FORWARD of the cells' many-input glue convs, K = 200..800 -> 40..160, was measured on this path in round 3 and is NOT taken: 28.6 vs 29.4 us
    // per launch at 40 output channels, 41.6 vs 25.7 us at 80 — the streaming-K fp32 kernel (pwk_kernel) is memory-bound on those shapes)
    return stride == 1 && dil == 1 && pad == 0 && OH == H && OW == W && Cn >= 192 && c3_planes(mode, Cn) != 0 && W >= 48 && P >= 2048;
  }
  if (stride == 2) {             // [r3] stem2 (3x3, stride 2, pad 1) forward on the split kernel: 128-channel blocks of 4 waves, de-interleaved patch rows
    if (!(KH == 3 && KW == 3 && dil == 1 && pad == 1 && OH == (H - 1) / 2 + 1 && OW == (W - 1) / 2 + 1 && c3_planes(mode, Cn) != 0 && OW >= 96)) return false;
    if (fwd) return Cn >= 96 && c3b_wc(Cn, (long)P) == 4 && P >= 8192;
    return Cn >= 32 && Cn <= 64 && P >= 32768;      // data gradient: the four parity classes as 2-tile blocks (conv3s_kernel)
  }
  if (KH != KW || !(KH == 3 || KH == 5) || stride != 1 || dil < 1 || dil > c3_maxdil(KH)) return false;
  if (!(pad == dil * (KH / 2) && OH == H && OW == W && Cn >= 32)) return false;
  if (dil <= 2 && H < 2 * dil) return false;      // two-row tiles (the one-row forms of these shapes are not instantiated)
  // the split kernel has half-width (64-pixel) tiles and also takes the 32x64 maps of level 3 (dil_conv at 160 channels: 152 us on
  // the generic kernel); the fp32 halo kernel keeps its 128-pixel tiles and the larger maps
  if (c3_planes(mode, Cn)) return W >= 48 && P >= 2048;
  return W >= 100 && P >= 8192;
}

// Kind, tile walk, grid, LDS and weight-pack layout of a halo launch with Cn output channels over the N x H x W output map (data gradient: the
// gradient map) whose K side is the chunks cvalid[0..nch) of <= 16 channels, and the kernel itself.  false: no unit instantiates that form
bool c3_layout(ConvChoice& c, int mode, int dir, int Cn, int N, int H, int W, int taps, int dil, int st, int nch, const int* cvalid) {
  const long P = (long)N * H * W;
  const int np = c3_planes(mode, Cn);
  const int ks = taps == 1 ? 1 : taps == 9 ? 3 : 5;
  const long trailer = np == 2 ? C3_TRAILER : 0;      // split-fp16: the scale trailer of the pack (PackK.amax)
  c.nchunks = nch; c.planes = np; c.dil_odd = 0; c.s2d = 0;
  if (!np) {                        // exact fp32: conv3_kernel, 128-pixel one-row tiles, 16 x bct columns per block
    c.kind = CK_HALO; c.bct = c3_bct(Cn, P, ks, dir); c.v[0] = c.bct; c.v[1] = ks;
    c.var = c3_variant_fp32(c.bct, ks, dir);
    c.nT = nch * taps; c.wp_blk = (long)nch * taps * c.bct * 256;
    c.spr = cdiv(W, C3_BP); c.HT = H; c.ntiles = N * H * c.spr;
    c.pack_floats = (long)cdiv(Cn, 16 * c.bct) * nch * taps * c.bct * 256;
    c.pack_blocks = cdiv(c.pack_floats, 256 * 4);
    c.gx = c.rows; c.gy = cdiv(Cn, 16 * c.bct);
  } else if (st == 2 && dir == MODE_DGRAD) {
    // stride-2 data gradient: every workgroup runs the four parity classes of the input pixel (1 / 2 / 2 / 4 taps) from one staged image of dy;
    // a tile is dy row a x 64 positions b (gradient rows 2a, 2a + 1 x 128 pixels)
    c.kind = CK_SPLIT_S2D; c.v[0] = np;
    c.var = c3b_variant_s2d(np);
    c.bct = 2; c.s2d = 1;
    const long unit = (long)cdiv(Cn, 64) * nch * 2 * 64;       // 16-byte units per tap of the four class streams (c3b_pack_s2d_body)
    c.nT = 9 * nch; c.wp_blk = unit * np;
    c.HT = (H + 1) / 2; c.spr = cdiv((W + 1) / 2, 64); c.ntiles = N * c.HT * c.spr;
    c.pack_floats = 9 * unit * np * 4 + trailer;
    c.pack_blocks = cdiv(9 * unit, 256);
    c.gx = c.rows < c.ntiles ? c.rows : c.ntiles; c.gy = 1;
    c.lds = 2 * 64 * 16 + (size_t)np * 2 * (64 + 16) * 32;
  } else if (Cn <= 48 && taps == 25 && dil <= 2 && st == 1) {
    // [r5] the 16-wide-tile kernel (conv3n.hip) takes the 5x5 launches at dilation <= 2 with at most 48 output channels (the cells' dil_conv_5x5 at
    // 40 channels, forward and data gradient).  The 3x3 stays on conv3b_kernel: 24.8 against 25.4-26.8 us at 2x125x253 — one workgroup per CU
    // leaves its 13 K-steps nothing to hide the staging behind.
    c.kind = CK_C3N; c.v[0] = ks; c.v[1] = np;
    c.var = c3n_variant(ks, dir, np);
    c.bct = 3; c.dil_odd = dil & 1; c.s2d = 2;
    int steps = 0;
    for (int i = 0; i < nch; ++i) steps += c3n_steps(taps, cvalid[i]);
    c.nT = steps; c.wp_blk = 0;
    c.HT = cdiv(H, 2 * dil) * dil; c.spr = cdiv(W, CN_BPX); c.ntiles = N * c.HT * c.spr;
    // 1 KB per (K-step, 16-row tile, plane); a chunk has at most (taps + 1) / 2 steps
    c.pack_floats = (long)nch * ((taps + 1) / 2) * 3 * np * 256 + trailer;
    c.pack_blocks = cdiv((long)steps * 3 * 64, 256);
    // one workgroup per tile at most: a workgroup without a tile would still queue for a CU's LDS and registers (989 slab rows against 252 tiles at 2x125x253)
    c.gx = c.rows < c.ntiles ? c.rows : c.ntiles; c.gy = 1;
    c.lds = 4 * 48 * 16 + (size_t)np * (ks + 1) * cn_pwp(ks) * 32;
  } else {
    const int wc = c3b_wc(Cn, P);
    c.kind = CK_SPLIT; c.bct = wc; c.dil_odd = st == 2 ? 2 : (dil & 1);
    c.nT = nch * taps; c.wp_blk = (long)nch * taps * wc * np * 64;          // 16-byte units per column block
    const bool bigd = taps == 9 && dil > 2;
    const int ph = wc == 2 ? 2 : 1;                                  // <= 64 channels: 4 waves = 2 channel tiles x 2 pixel halves
    // half-width tiles where 128-pixel tiles leave the chip short of blocks (instantiated for 3- and 4-wave blocks)
    const long blocks128 = (long)N * H * cdiv(W, C3_BP) * cdiv(Cn, 32 * wc);
    const bool half = st == 1 && ph == 1 && (wc == 3 || wc == 4) && !(wc == 3 && bigd) && !(wc == 4 && ks == 5) && !(wc == 3 && ks == 1) && blocks128 < 384;      // (rows of <= 64 pixels land here too)
    // quarter-width (32-pixel) tiles where even 64-pixel tiles leave the chip short of workgroups: the cells' dilated convs on the 32x64 maps ran as
    // 128 workgroups of 3 waves — half the CUs idle, one wave per SIMD on the others, every LDS / weight round trip exposed
    const long blocks64 = (long)N * H * cdiv(W, 64) * cdiv(Cn, 32 * wc);
    const bool quarter = half && wc == 3 && !bigd && (ks == 3 || ks == 5) && blocks64 < 192;      // measured: 160 ch @ 32x64 85 -> 63 us (5x5), 45 -> 34 (3x3); 80 ch @ 63x127 (252 blocks) is slower quartered (53 -> 66)
    const int bpx = st == 2 ? 64 : quarter ? 32 : half ? 64 : C3_BP;
    // two-row tiles (2 rows, d apart, of half the one-row width) for the 3x3 / 5x5 launches at dilation <= 2: KS + 1 staged rows per two output rows
    // (every 3x3 / 5x5 launch at dilation <= 2 of full width, or of half width on 3-wave blocks, takes them; c3_geometry_ok requires H >= 2 dil)
    const bool tworow = st == 1 && (ks == 3 || ks == 5) && !bigd && (bpx == C3_BP || (bpx == 64 && wc == 3)) && H >= 2 * dil;
    const int rpx = tworow ? bpx / 2 : bpx;                       // pixels per tile row
    c.v[0] = wc; c.v[1] = ks; c.v[2] = rpx; c.v[3] = tworow ? 2 : 1;
    // the instantiations live in conv3b_tr3 / conv3b_tr5 / conv3b_row / conv3b_s2.hip (compiled in parallel)
    c.var = tworow ? (ks == 3 ? c3b_variant_tr3(wc, rpx, dir, np) : c3b_variant_tr5(wc, rpx, dir, np))
          : st == 2 ? c3b_variant_s2f(wc, rpx, np)          // (the forward: the stride-2 data gradient is CK_SPLIT_S2D)
          : c3b_variant_row(wc, ks, bigd, rpx, dir, np);
    c.HT = tworow ? cdiv(H, 2 * dil) * dil : H;
    c.spr = cdiv(W, rpx); c.ntiles = N * c.HT * c.spr;
    c.pack_floats = (long)cdiv(Cn, 32 * wc) * nch * taps * wc * np * 256 + trailer;      // 1 KB per (tap, 32-row tile, plane)
    c.pack_blocks = cdiv((long)cdiv(Cn, 32 * wc) * c.nT * wc * 64, 256);              // one pack thread per (tile, lane)
    // no workgroups without a tile (they would queue for LDS and registers just to write zeros); the channel blocks of a tile side by side (conv3b_kernel)
    c.gx = (c.rows < c.ntiles ? c.rows : c.ntiles) * cdiv(Cn, 32 * wc); c.gy = 1;
    c.lds = (size_t)((ph * 32 * wc * 16 + 15) & ~15) + (size_t)np * (tworow ? ks + 1 : ks) * cb_pwmax(ks, bigd, rpx, st) * 32;
  }
  if (c.pack_blocks > 4096) c.pack_blocks = 4096;
  return c.var.fn != nullptr;
}

inline bool c3_pack_fits(const float* wpack, int64_t floats, int64_t need) { return wpack && aligned16(wpack) && floats >= need; }

}  // namespace

bool c3_choose_fwd(const addk_conv_args* a, int mode, int mask, ConvChoice& c) {
  if (!c3_geometry_ok(mode, mask, a->KH, a->KW, a->stride, a->pad, a->dil, a->H, a->W, a->OH, a->OW, (long)a->N * a->OH * a->OW, a->Cout, true)) return false;
  int cvalid[C3_MAXCH], nch = 0;
  for (int i = 0; i < a->nsrc; ++i) {
    if (!src_vec_ok(a->src[i]) || a->src[i].rs_hw) return false;
    for (int c0 = 0; c0 < a->src[i].C; c0 += C3_BK) {
      if (nch == C3_MAXCH) return false;
      cvalid[nch++] = a->src[i].C - c0 < C3_BK ? a->src[i].C - c0 : C3_BK;
    }
  }
  if (a->ldy % 4 || !aligned16(a->y)) return false;
  ConvChoice h = c;
  if (!c3_layout(h, mode, MODE_FWD, a->Cout, a->N, a->OH, a->OW, a->KH * a->KW, a->dil, a->stride, nch, cvalid)) return false;
  if (!c3_pack_fits(a->wpack, a->wpack_floats, h.pack_floats)) return false;
  c = h;
  return true;
}
bool c3_choose_dgrad(const addk_conv_dgrad_args* a, int mode, int mask, ConvChoice& c) {
  if (!c3_geometry_ok(mode, mask, a->KH, a->KW, a->stride, a->pad, a->dil, a->H, a->W, a->OH, a->OW, (long)a->N * a->H * a->W, a->dst.C, false)) return false;
  if (a->Cout % 4 || a->lddy % 4 || a->ldg % 4 || !aligned16(a->dy) || !aligned16(a->g) || !src_vec_ok(a->dst)) return false;
  int cvalid[C3_MAXCH], nch = 0;
  for (int c0 = 0; c0 < a->Cout; c0 += C3_BK) {
    if (nch == C3_MAXCH) return false;
    cvalid[nch++] = a->Cout - c0 < C3_BK ? a->Cout - c0 : C3_BK;
  }
  ConvChoice h = c;
  if (!c3_layout(h, mode, MODE_DGRAD, a->dst.C, a->N, a->H, a->W, a->KH * a->KW, a->dil, a->stride, nch, cvalid)) return false;
  if (!c3_pack_fits(a->wpack, a->wpack_floats, h.pack_floats)) return false;
  c = h;
  return true;
}

namespace {

// the pack descriptor of a halo launch: the K chunks (fwd: channels of the sources inside a tap; dgrad: dy channels) and the choice's layout
void c3_pack_fill(const ConvChoice& c, int dir, const float* w, int ldw, int cin_total, int w_choff, int taps, int wrows, int Cn,
                  const addk_src* src, int nsrc, float* wpack, PackK& pk) {
  pk = PackK{};
  int nch = 0, choff = 0;
  for (int i = 0; i < nsrc; ++i) {
    for (int c0 = 0; c0 < src[i].C; c0 += C3_BK) {
      pk.cbase[nch] = (dir == MODE_FWD ? w_choff : 0) + choff + c0;
      pk.cvalid[nch] = src[i].C - c0 < C3_BK ? src[i].C - c0 : C3_BK;
      ++nch;
    }
    choff += src[i].C;
  }
  pk.nchunks = nch; pk.taps = taps; pk.w = w; pk.ldw = ldw; pk.cin_total = cin_total; pk.w_choff = dir == MODE_FWD ? 0 : w_choff; pk.out = wpack;
  pk.amax = c.planes == 2 ? wpack + (c.pack_floats - C3_TRAILER) : nullptr;
  pk.wrows = wrows;
  pk.mode = dir; pk.Cn = Cn; pk.bct = c.bct; pk.planes = c.planes; pk.dil_odd = c.dil_odd; pk.s2d = c.s2d;
  if (c.kind == CK_C3N)
    for (int i = 0, steps = 0; i < nch; ++i) { pk.sbase[i] = steps; steps += c3n_steps(taps, pk.cvalid[i]); }
}
void c3_pack_fill_fwd(const ConvChoice& c, const addk_conv_args* a, PackK& pk) {
  c3_pack_fill(c, MODE_FWD, a->w, a->ldw, a->cin_total, a->w_choff, a->KH * a->KW, a->Cout, a->Cout, a->src, a->nsrc, a->wpack, pk);
}
void c3_pack_fill_dgrad(const ConvChoice& c, const addk_conv_dgrad_args* a, PackK& pk) {
  const addk_src dy{a->dy, nullptr, nullptr, a->lddy, a->Cout, 0, 0};
  c3_pack_fill(c, MODE_DGRAD, a->w, a->ldw, a->cin_total, a->w_choff, a->KH * a->KW, a->Cout, a->dst.C, &dy, 1, a->wpack, pk);
}

// the pack (unless a plan's addk_conv_pack_batch already wrote it), then the convolution; k holds the launch's tensors
int c3_run(const ConvChoice& c, C3K& k, const PackK& pk, bool packed, hipStream_t st) {
  k.wp = pk.out; k.wsc = pk.amax ? pk.amax + C3_AMAX_WG : nullptr;
  k.nT = c.nT; k.wp_blk = c.wp_blk; k.HT = c.HT; k.spr = c.spr; k.ntiles = c.ntiles; k.slab_rows = c.rows;
  k.red32 = c.kind == CK_HALO ? k.P >= 4096 : 1;
  k.ny = c.kind == CK_SPLIT ? cdiv(k.Cn, 32 * c.v[0]) : 1;
  if (!packed) {
    if (pk.planes == 2) hipLaunchKernelGGL(c3_pack_amax_kernel, dim3(C3_AMAX_WG), dim3(256), 0, st, pk);
    hipLaunchKernelGGL(c3_pack_kernel, dim3(c.pack_blocks), dim3(256), 0, st, pk);
  }
  if (c.var.raise_lds) c.var.raise_lds();
  hipLaunchKernelGGL(c.var.fn, dim3(c.gx, c.gy), dim3(c.var.threads), c.lds, st, k);      // (c.lds: 0 for conv3_kernel, whose LDS is static)
  return addk_check_launch(c.kind == CK_HALO ? "conv3" : c.kind == CK_C3N ? "conv3n" : c.kind == CK_SPLIT_S2D ? "conv3b stride-2 data gradient" : "conv3b");
}

template <int BCT, int KS> C3Variant c3_fp32_pair(int mode) {
  return mode == MODE_FWD ? c3_static_variant<conv3_kernel<BCT, KS, MODE_FWD>>(256) : c3_static_variant<conv3_kernel<BCT, KS, MODE_DGRAD>>(256);
}

}  // namespace

C3Variant c3_variant_fp32(int bct, int ks, int mode) {
  if (mode != MODE_FWD && mode != MODE_DGRAD) return {};
  if (ks == 3) return bct == 3 ? c3_fp32_pair<3, 3>(mode) : bct == 4 ? c3_fp32_pair<4, 3>(mode) : bct == 5 ? c3_fp32_pair<5, 3>(mode) : bct == 8 ? c3_fp32_pair<8, 3>(mode) : C3Variant{};
  if (ks == 5) return bct == 3 ? c3_fp32_pair<3, 5>(mode) : bct == 4 ? c3_fp32_pair<4, 5>(mode) : bct == 5 ? c3_fp32_pair<5, 5>(mode) : C3Variant{};      // (no 128-channel block: c3_bct)
  return {};
}

int c3_run_fwd(const ConvChoice& c, const addk_conv_args* a, hipStream_t st) {
  C3K k; PackK pk;
  c3_pack_fill_fwd(c, a, pk);
  k.nsrc = a->nsrc;
  for (int i = 0; i < a->nsrc; ++i) k.src[i] = a->src[i];
  k.N = a->N; k.H = a->OH; k.W = a->OW; k.IH = a->H; k.IW = a->W; k.dil = a->dil; k.st = a->stride;
  k.om = 1; k.oro = k.oco = 0; k.OHo = a->OH; k.OWo = a->OW;
  k.Cn = a->Cout; k.ldy = a->ldy; k.y = a->y; k.bias = a->bias; k.bias_n = a->bias_n;
  k.slab = (double*)a->stats; k.slab_ld = a->stats_ld > 0 ? a->stats_ld : a->Cout;
  k.dst = addk_src{nullptr, nullptr, nullptr, 0, 0, 0, 0}; k.accumulate = 0;
  k.vecY = 1;
  k.P = (long)a->N * a->OH * a->OW;
  return c3_run(c, k, pk, a->wpack_ready != 0, st);
}
int c3_run_dgrad(const ConvChoice& c, const addk_conv_dgrad_args* a, hipStream_t st) {
  C3K k; PackK pk;
  c3_pack_fill_dgrad(c, a, pk);
  k.nsrc = 1;
  k.src[0] = addk_src{a->dy, nullptr, nullptr, a->lddy, a->Cout, 0, 0};
  k.N = a->N; k.H = a->H; k.W = a->W; k.IH = a->OH; k.IW = a->OW; k.dil = a->dil; k.st = a->stride;      // the gather runs over dy (OH x OW)
  k.om = 1; k.oro = k.oco = 0; k.OHo = a->H; k.OWo = a->W;
  k.Cn = a->dst.C; k.ldy = a->ldg; k.y = a->g; k.bias = nullptr; k.bias_n = nullptr;
  k.slab = (double*)a->dab; k.slab_ld = a->dst.C;
  k.dst = a->dst; k.accumulate = a->accumulate;
  k.vecY = 1;
  k.P = (long)a->N * a->H * a->W;
  return c3_run(c, k, pk, a->wpack_ready != 0, st);
}

// Floats of `wpack` the launch's halo-patch kernel needs: the choice the launch would make with a large enough workspace.  0 = it takes another kernel.
template <typename Args>
static int64_t c3_pack_floats(const Args* a, int (*choose)(const Args*, int, int, ConvChoice&)) {
  if (!a) return 0;
  Args t = *a;
  t.wpack = reinterpret_cast<float*>(alignof(float4)); t.wpack_floats = INT64_MAX;      // any aligned address: the choice never dereferences it
  ConvChoice c;
  if (choose(&t, addk_get_conv_precision(), addk_get_fast_paths(), c) || !conv_kind_halo(c.kind)) return 0;
  return c.pack_floats;
}
extern "C" int64_t addk_conv_fwd_pack_floats(const addk_conv_args* a) { return c3_pack_floats(a, conv_choose_fwd); }
extern "C" int64_t addk_conv_dgrad_pack_floats(const addk_conv_dgrad_args* a) { return c3_pack_floats(a, conv_choose_dgrad); }

#ifdef ADDK_C3B_DIAG
// (shader ticks, reference ticks, workgroups, 0) summed since the last call; resets the counters
extern "C" int addk_c3b_diag(unsigned long long* out12) {
  for (int k = 0; k < 12; ++k) out12[k] = 0;
  c3b_diag_tr3(out12); c3b_diag_tr5(out12); c3b_diag_row(out12); c3b_diag_s2(out12);      // every instantiating unit has its own counters
  return ADDK_OK;
}
#endif
extern "C" int addk_set_split_min_channels(int c) { g_c3b_minc = c < 0 ? 0 : c; return ADDK_OK; }

// Hoisting the weight packs out of the step's critical path: a plan collects one descriptor per halo-patch launch,
// uploads the table and runs ONE addk_conv_pack_batch at the start of the step; the launches then carry wpack_ready = 1.
extern "C" int64_t addk_conv_pack_desc_bytes(void) { return (int64_t)sizeof(PackK); }
extern "C" int addk_conv_fwd_pack_desc(const addk_conv_args* a, void* host_desc) {
  ADDK_REQUIRE(a && host_desc, "conv_fwd_pack_desc: null pointer");
  ConvChoice c;
  if (const int rc = conv_choose_fwd(a, addk_get_conv_precision(), addk_get_fast_paths(), c)) return rc;
  if (!conv_kind_halo(c.kind)) { addk_set_error("conv_fwd_pack_desc: the launch does not take a halo-patch kernel"); return ADDK_ERR_UNSUPPORTED; }
  c3_pack_fill_fwd(c, a, *reinterpret_cast<PackK*>(host_desc));
  return ADDK_OK;
}
extern "C" int addk_conv_dgrad_pack_desc(const addk_conv_dgrad_args* a, void* host_desc) {
  ADDK_REQUIRE(a && host_desc, "conv_dgrad_pack_desc: null pointer");
  ConvChoice c;
  if (const int rc = conv_choose_dgrad(a, addk_get_conv_precision(), addk_get_fast_paths(), c)) return rc;
  if (!conv_kind_halo(c.kind)) { addk_set_error("conv_dgrad_pack_desc: the launch does not take a halo-patch kernel"); return ADDK_ERR_UNSUPPORTED; }
  c3_pack_fill_dgrad(c, a, *reinterpret_cast<PackK*>(host_desc));
  return ADDK_OK;
}
extern "C" int addk_conv_pack_batch(const void* dev_descs, int32_t n, void* stream) {
  ADDK_REQUIRE(dev_descs && n > 0, "conv_pack_batch: bad args");
  const int m = addk_get_conv_precision();
  if (m == 1 || m == 3)        // modes with split-fp16 launches: their packs take the tensor's scale from the amax pass (descriptors of other packs return at once)
    hipLaunchKernelGGL(c3_pack_amax_batch_kernel, dim3(C3_AMAX_WG, n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const PackK*>(dev_descs));
  hipLaunchKernelGGL(c3_pack_batch_kernel, dim3(64, n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const PackK*>(dev_descs));
  return addk_check_launch("conv_pack_batch");
}
