// Bilinear resize, align_corners=False, no antialias — F.interpolate(mode='bilinear') as called at
// ADD.py:76-77,84,89,317 and decoder.py:24,28 (used for both up- and down-sampling).
// Index arithmetic follows ATen's area_pixel_compute_source_index in fp32:
//     scale = in/out;  src = max(0, scale*(dst+0.5)-0.5);  i0 = floor(src); i1 = min(i0+1, in-1); l1 = src-i0.
// Forward: one thread per (output pixel, channel quad), 16 B per lane.
// Backward is a GATHER (deterministic, no atomics): an input pixel enumerates the few output rows/cols
// whose i0/i1 hit it, recomputing exactly the forward weights.
#include "common.h"

namespace {

// candidate output range [lo, hi] whose taps may touch input index i
__device__ __forceinline__ void out_range(int i, float scale, int out, int& lo, int& hi) {
  float inv = 1.f / scale;
  float a = ((float)i - 1.f + 0.5f) * inv - 0.5f;
  float b = ((float)i + 1.f + 0.5f) * inv - 0.5f;
  lo = (int)floorf(a) - 1; hi = (int)ceilf(b) + 1;
  if (lo < 0) lo = 0;
  if (hi > out - 1) hi = out - 1;
}

// weight with which output index o reads input index i (0 when it does not)
__device__ __forceinline__ float tap_weight(int o, int i, float scale, int in) {
  int i0, i1; float l0, l1;
  src_index(o, scale, in, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

// Block sums of the (dA, dB) pairs the NHWC backward kernels keep per thread (as affine_sum_bwd_kernel's): the pixel lanes write an
// [npl][C4][2] fp64 panel, one barrier, then thread k < 2C adds the npl rows of column (channel k / 2, A|B) in fixed order into row `row` of the slab
__device__ __forceinline__ void panel_sum(double* panel, const double (&sA)[4], const double (&sB)[4], bool active, int pl, int c, int C, int C4, int npl, double* slab, long row) {
  if (active) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { panel[((pl * C4) + c + e) * 2] = sA[e]; panel[((pl * C4) + c + e) * 2 + 1] = sB[e]; }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < C * 2; k += 256) {
    const int ch = k >> 1, ab = k & 1;
    double acc = 0.0;
    for (int r = 0; r < npl; ++r) acc += panel[((r * C4) + ch) * 2 + ab];
    slab[row * C * 2 + k] = acc;
  }
}

__device__ __forceinline__ float4 fma4(float k, const float4 d, const float4 dz) {
  return make_float4(fmaf(k, d.x, dz.x), fmaf(k, d.y, dz.y), fmaf(k, d.z, dz.z), fmaf(k, d.w, dz.w));
}

struct RsK {
  addk_src src; int N, H, W, OH, OW;
  float* y; int ldy; int nchw;
  const float* dy; int lddy; const float* dy_scale;
  float* g; int ldg; int accumulate; double* dab;
  int nq, npl, vec; long P;
};

__global__ void __launch_bounds__(256) resize_fwd_kernel(const RsK p) {
  const int q = threadIdx.x % p.nq, pl = threadIdx.x / p.nq;
  if (pl >= p.npl) return;
  const int c = 4 * q, nrem = p.src.C - c;
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  const long ohw = (long)p.OH * p.OW;
  const bool relu = p.src.relu != 0;
  for (long pp = (long)blockIdx.x * p.npl + pl; pp < p.P; pp += (long)gridDim.x * p.npl) {
    int n = (int)(pp / ohw); int rem = (int)(pp - (long)n * ohw);
    int oh = rem / p.OW, ow = rem - oh * p.OW;
    int h0, h1, w0, w1; float lh0, lh1, lw0, lw1;
    src_index(oh, sh, p.H, h0, h1, lh0, lh1);
    src_index(ow, sw, p.W, w0, w1, lw0, lw1);
    const float* b = p.src.x + (long)n * p.H * p.W * p.src.ld + c;
    float4 v00 = prologue4(ld4g(b + ((long)h0 * p.W + w0) * p.src.ld, nrem, p.vec), p.src.a, p.src.b, c, nrem, relu, p.vec);
    float4 v01 = prologue4(ld4g(b + ((long)h0 * p.W + w1) * p.src.ld, nrem, p.vec), p.src.a, p.src.b, c, nrem, relu, p.vec);
    float4 v10 = prologue4(ld4g(b + ((long)h1 * p.W + w0) * p.src.ld, nrem, p.vec), p.src.a, p.src.b, c, nrem, relu, p.vec);
    float4 v11 = prologue4(ld4g(b + ((long)h1 * p.W + w1) * p.src.ld, nrem, p.vec), p.src.a, p.src.b, c, nrem, relu, p.vec);
    const float4 o = lerp4(v00, v01, v10, v11, lh0, lh1, lw0, lw1);
    st4g(p.y + pp * p.ldy + c, o, nrem, p.vec);
  }
}

// NCHW destination (final logits, decoder.py:28): one thread per output pixel, loop over channels so that
// stores are contiguous along W for every channel plane.
__global__ void __launch_bounds__(256) resize_fwd_nchw_kernel(const RsK p) {
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  const long ohw = (long)p.OH * p.OW;
  const int C = p.src.C;
  for (long pp = (long)blockIdx.x * blockDim.x + threadIdx.x; pp < p.P; pp += (long)gridDim.x * blockDim.x) {
    int n = (int)(pp / ohw); long rem = pp - (long)n * ohw;
    int oh = (int)(rem / p.OW), ow = (int)(rem - (long)oh * p.OW);
    int h0, h1, w0, w1; float lh0, lh1, lw0, lw1;
    src_index(oh, sh, p.H, h0, h1, lh0, lh1);
    src_index(ow, sw, p.W, w0, w1, lw0, lw1);
    const float* b = p.src.x + (long)n * p.H * p.W * p.src.ld;
    const float* p00 = b + ((long)h0 * p.W + w0) * p.src.ld;
    const float* p01 = b + ((long)h0 * p.W + w1) * p.src.ld;
    const float* p10 = b + ((long)h1 * p.W + w0) * p.src.ld;
    const float* p11 = b + ((long)h1 * p.W + w1) * p.src.ld;
    float* yo = p.y + (long)n * C * ohw + rem;
    for (int c = 0; c < C; ++c) {
      float a = p.src.a ? p.src.a[c] : 1.f, bb = p.src.b ? p.src.b[c] : 0.f;
      float v00 = fmaf(a, p00[c], bb), v01 = fmaf(a, p01[c], bb), v10 = fmaf(a, p10[c], bb), v11 = fmaf(a, p11[c], bb);
      if (p.src.relu) { v00 = fmaxf(v00, 0.f); v01 = fmaxf(v01, 0.f); v10 = fmaxf(v10, 0.f); v11 = fmaxf(v11, 0.f); }
      yo[(long)c * ohw] = lh0 * (lw0 * v00 + lw1 * v01) + lh1 * (lw0 * v10 + lw1 * v11);
    }
  }
}


// Backward of the final logits up-sampling (NCHW gradient in, NHWC gradient out; decoder.py:28), LDS-tiled and SEPARABLE:
// a block owns an 8x8 tile of low-resolution pixels of one channel plane, stages the block of the high-resolution
// gradient those pixels receive from (<= RB_PM x RB_PM, contiguous row segments, independent loads), reduces it along W
// with the column weights (t1[row][j]) and then along H with the row weights: 2*T taps per pixel instead of T*T
// (T = 21 at the x8 up-sampling of config 2).  The thread-per-pixel kernel below walks its T*T x 19 taps as dependent
// global loads (1.17 ms per exit at 1024x2048).
constexpr int RB_T = 8, RB_PM = 88, RB_MAXT = 22;

__global__ void __launch_bounds__(256) resize_bwd_nchw_tile_kernel(const RsK p, int tiles_x, int tiles_y) {
  __shared__ float patch[RB_PM][RB_PM + 1];
  __shared__ float t1[RB_PM][RB_T];
  __shared__ float wtw[RB_T][RB_MAXT], wth[RB_T][RB_MAXT];
  __shared__ int lo_w[RB_T], lo_h[RB_T], n_w[RB_T], n_h[RB_T];
  const int C = p.src.C;
  int b = blockIdx.x;
  const int tx = b % tiles_x; b /= tiles_x;
  const int ty = b % tiles_y; const int n = b / tiles_y;
  const int c = blockIdx.y;
  const int ih0 = ty * RB_T, iw0 = tx * RB_T;
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  int rlo, rhi, clo, chi, tmp;
  out_range(ih0, sh, p.OH, rlo, tmp);
  out_range(min(ih0 + RB_T - 1, p.H - 1), sh, p.OH, tmp, rhi);
  out_range(iw0, sw, p.OW, clo, tmp);
  out_range(min(iw0 + RB_T - 1, p.W - 1), sw, p.OW, tmp, chi);
  const int PH = rhi - rlo + 1, PW = chi - clo + 1;          // host guarantees <= RB_PM
  const float* plane = p.dy + ((long)n * C + c) * ((long)p.OH * p.OW) + (long)rlo * p.OW + clo;
  const int per = PH * PW;
#pragma unroll 4
  for (int i = threadIdx.x; i < per; i += 256) {
    const int r = i / PW, cc = i - r * PW;
    patch[r][cc] = plane[(long)r * p.OW + cc];
  }
  // per-axis weight tables of the tile's 8 columns / 8 rows
  if (threadIdx.x < 2 * RB_T) {
    const bool isw = threadIdx.x < RB_T;
    const int j = threadIdx.x & (RB_T - 1);
    const int i = (isw ? iw0 : ih0) + j;
    const int lim = isw ? p.W : p.H;
    int lo = 0, hi = -1;
    if (i < lim) out_range(i, isw ? sw : sh, isw ? p.OW : p.OH, lo, hi);
    if (isw) { lo_w[j] = lo; n_w[j] = hi - lo + 1; } else { lo_h[j] = lo; n_h[j] = hi - lo + 1; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * RB_T * RB_MAXT; i += 256) {
    const bool isw = i < RB_T * RB_MAXT;
    const int r = isw ? i : i - RB_T * RB_MAXT;
    const int j = r / RB_MAXT, k = r - j * RB_MAXT;
    if (isw) wtw[j][k] = k < n_w[j] ? tap_weight(lo_w[j] + k, iw0 + j, sw, p.W) : 0.f;
    else     wth[j][k] = k < n_h[j] ? tap_weight(lo_h[j] + k, ih0 + j, sh, p.H) : 0.f;
  }
  __syncthreads();
  // pass 1: along W
  for (int i = threadIdx.x; i < PH * RB_T; i += 256) {
    const int r = i / RB_T, j = i - r * RB_T;
    const float* row = &patch[r][lo_w[j] - clo];
    float acc = 0.f;
    const int nw = n_w[j];
#pragma unroll
    for (int k = 0; k < RB_MAXT; ++k) if (k < nw) acc = fmaf(wtw[j][k], row[k], acc);
    t1[r][j] = acc;
  }
  __syncthreads();
  // pass 2: along H, one thread per pixel of the tile
  if (threadIdx.x < RB_T * RB_T) {
    const int i = threadIdx.x / RB_T, j = threadIdx.x - i * RB_T;
    const int ih = ih0 + i, iw = iw0 + j;
    if (ih < p.H && iw < p.W) {
      const int nh = n_h[i], r0 = lo_h[i] - rlo;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < RB_MAXT; ++k) if (k < nh) acc = fmaf(wth[i][k], t1[r0 + k][j], acc);
      const float gs = p.dy_scale ? *p.dy_scale : 1.f;
      const float a = p.src.a ? p.src.a[c] : 1.f;
      float* gp = p.g + ((long)(n * p.H + ih) * p.W + iw) * p.ldg + c;
      const float gv = acc * gs * a;
      *gp = p.accumulate ? *gp + gv : gv;
    }
  }
}

template <bool NCHW>
__global__ void __launch_bounds__(256) resize_bwd_kernel(const RsK p) {
  extern __shared__ double redt[];       // [C4][2]
  const int C = p.src.C;
  const int q = NCHW ? 0 : threadIdx.x % p.nq, pl = NCHW ? threadIdx.x : threadIdx.x / p.nq;
  const bool active = pl < p.npl;
  const int c = 4 * q, nrem = C - c;
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  const long hw = (long)p.H * p.W, ohw = (long)p.OH * p.OW;
  const float gs = p.dy_scale ? *p.dy_scale : 1.f;
  float4 av = make_float4(1.f, 1.f, 1.f, 1.f), bv = zero4();
  double sA[4] = {0.0, 0.0, 0.0, 0.0}, sB[4] = {0.0, 0.0, 0.0, 0.0};
  if (!NCHW && active && p.src.a) { av = ld4g(p.src.a + c, nrem, p.vec); bv = ld4g(p.src.b + c, nrem, p.vec); }
  if (active) {
    for (long pp = (long)blockIdx.x * p.npl + pl; pp < p.P; pp += (long)gridDim.x * p.npl) {
      int n = (int)(pp / hw); int rem = (int)(pp - (long)n * hw);
      int ih = rem / p.W, iw = rem - ih * p.W;
      int hlo, hhi, wlo, whi;
      out_range(ih, sh, p.OH, hlo, hhi);
      out_range(iw, sw, p.OW, wlo, whi);
      if (NCHW) {
        // channel loop outside: dy planes are contiguous along W; no prologue on the logits source
        for (int cc = 0; cc < C; ++cc) {
          const float* d = p.dy + ((long)n * C + cc) * ohw;
          float s = 0.f;
          for (int oh = hlo; oh <= hhi; ++oh) {
            float wh = tap_weight(oh, ih, sh, p.H);
            if (wh == 0.f) continue;
            float r = 0.f;
            for (int ow = wlo; ow <= whi; ++ow) {
              float ww = tap_weight(ow, iw, sw, p.W);
              if (ww != 0.f) r = fmaf(ww, d[(long)oh * p.OW + ow], r);
            }
            s = fmaf(wh, r, s);
          }
          s *= gs;
          float a = p.src.a ? p.src.a[cc] : 1.f;
          float* gp = p.g + pp * p.ldg + cc;
          float gv = s * a;
          *gp = p.accumulate ? *gp + gv : gv;
        }
      } else {
        float4 dz = zero4();
        // trim the conservative candidate ranges to the taps that really read this pixel (weights > 0 form one run)
        while (hlo < hhi && tap_weight(hlo, ih, sh, p.H) == 0.f) ++hlo;
        while (hhi > hlo && tap_weight(hhi, ih, sh, p.H) == 0.f) --hhi;
        while (wlo < whi && tap_weight(wlo, iw, sw, p.W) == 0.f) ++wlo;
        while (whi > wlo && tap_weight(whi, iw, sw, p.W) == 0.f) --whi;
        const int nh = hhi - hlo + 1, nw = whi - wlo + 1;
        if (nh <= 5 && nw <= 5 && p.vec && nrem >= 4) {
          // up to x2 up-sampling: <= 5x5 taps
          float ww5[5]; int wo5[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            ww5[k] = k < nw ? tap_weight(wlo + k, iw, sw, p.W) : 0.f;
            wo5[k] = (k < nw ? wlo + k : wlo) * p.lddy;
          }
          for (int a = 0; a < nh; ++a) {
            const float wh = tap_weight(hlo + a, ih, sh, p.H);
            const float* rowp = p.dy + (long)(n * p.OH + hlo + a) * p.OW * p.lddy + c;
            float4 d5[5];
#pragma unroll
            for (int b = 0; b < 5; ++b) d5[b] = ld4(rowp + wo5[b]);
#pragma unroll
            for (int b = 0; b < 5; ++b) dz = fma4(wh * ww5[b], d5[b], dz);
          }
        } else if (nh <= 8 && nw <= 8) {
          // per-axis weights in registers (static indexing), then at most 8x8 taps
          float wh8[8], ww8[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            wh8[k] = k < nh ? tap_weight(hlo + k, ih, sh, p.H) : 0.f;
            ww8[k] = k < nw ? tap_weight(wlo + k, iw, sw, p.W) : 0.f;
          }
#pragma unroll
          for (int a = 0; a < 8; ++a) {
            if (wh8[a] != 0.f) {
#pragma unroll
              for (int b = 0; b < 8; ++b) {
                if (ww8[b] != 0.f) {
                  float4 d = ld4g(p.dy + ((long)(n * p.OH + hlo + a) * p.OW + wlo + b) * p.lddy + c, nrem, p.vec);
                  dz = fma4(wh8[a] * ww8[b], d, dz);
                }
              }
            }
          }
        } else {
          for (int oh = hlo; oh <= hhi; ++oh) {
            float wh = tap_weight(oh, ih, sh, p.H);
            if (wh == 0.f) continue;
            for (int ow = wlo; ow <= whi; ++ow) {
              float ww = tap_weight(ow, iw, sw, p.W);
              if (ww == 0.f) continue;
              float4 d = ld4g(p.dy + ((long)(n * p.OH + oh) * p.OW + ow) * p.lddy + c, nrem, p.vec);
              dz = fma4(wh * ww, d, dz);
            }
          }
        }
        dz.x *= gs; dz.y *= gs; dz.z *= gs; dz.w *= gs;
        if (p.src.relu || p.dab) {
          float4 x = ld4g(p.src.x + pp * p.src.ld + c, nrem, p.vec);
          if (p.src.relu) {
            if (!(fmaf(av.x, x.x, bv.x) > 0.f)) dz.x = 0.f;
            if (!(fmaf(av.y, x.y, bv.y) > 0.f)) dz.y = 0.f;
            if (!(fmaf(av.z, x.z, bv.z) > 0.f)) dz.z = 0.f;
            if (!(fmaf(av.w, x.w, bv.w) > 0.f)) dz.w = 0.f;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) { sA[e] += (double)get4(dz, e) * (double)get4(x, e); sB[e] += (double)get4(dz, e); }
        }
        float4 gv = make_float4(dz.x * av.x, dz.y * av.y, dz.z * av.z, dz.w * av.w);
        float* gp = p.g + pp * p.ldg + c;
        if (p.accumulate) { float4 o = ld4g(gp, nrem, p.vec); gv.x += o.x; gv.y += o.y; gv.z += o.z; gv.w += o.w; }
        st4g(gp, gv, nrem, p.vec);
      }
    }
  }
  const int C4 = p.nq * 4;
  if (!NCHW && p.dab) panel_sum(redt, sA, sB, active, pl, c, C, C4, p.npl, p.dab, blockIdx.x);
}

// Table-driven backward for resizes of at most x2 up-sampling (every in-network resize of the path: /4, /2, x2 and the
// 63 <-> 64 / 125 <-> 128 fits of even-sized inputs).  The kernel above re-derives, in EVERY (pixel, channel quad) thread, the
// candidate output range of its input pixel and trims it with up to ten tap_weight evaluations per axis before it can issue a
// load: 28 us per launch at 1.1 TB/s.  Here a workgroup walks row segments of `tw` input pixels; per segment it builds the
// per-axis tables (first output index, tap count <= 5, weights — the very same fp32 expressions, so results are bit-identical)
// ONCE in LDS, tw + 1 threads busy for a few dozen cycles, and every thread then issues its nh*nw independent 16-byte loads
// straight from the table.  Statistics ((dA, dB) of a ReLU'd lazy source) as above: registers across segments, one row per workgroup.
constexpr int RT_MAXW = 128;
// MT: taps per axis an input pixel can receive from — 5 up to x2 up-sampling, 9 up to x4, 17 up to x8 (the resizes in front of ASPP)
template <int MT>
__device__ __forceinline__ void resize_bwd_tab_body(const RsK& p, int tiles_per_row, int ntiles, int tw, const int bx, const int gx) {      // workgroup bx of gx
  extern __shared__ double redt[];       // [npl][C4][2]
  __shared__ float wt_w[RT_MAXW][MT], wt_h[MT];
  __shared__ int lo_w[RT_MAXW], n_w[RT_MAXW], lo_h, n_h;
  const int C = p.src.C;
  const int q = threadIdx.x % p.nq, pl = threadIdx.x / p.nq;
  const bool active = pl < p.npl;
  const int c = 4 * q;
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  const float gs = p.dy_scale ? *p.dy_scale : 1.f;
  float4 av = make_float4(1.f, 1.f, 1.f, 1.f), bv = zero4();
  double sA[4] = {0.0, 0.0, 0.0, 0.0}, sB[4] = {0.0, 0.0, 0.0, 0.0};
  if (active && p.src.a) { av = ld4(p.src.a + c); bv = ld4(p.src.b + c); }
  for (int tile = bx; tile < ntiles; tile += gx) {
    const int rowid = tile / tiles_per_row, seg = tile - rowid * tiles_per_row;
    const int n = rowid / p.H, ih = rowid - n * p.H, iw0 = seg * tw;
    __syncthreads();                                   // the previous segment's readers are done with the tables
    if ((int)threadIdx.x <= tw) {
      const bool isw = (int)threadIdx.x < tw;
      const int i = isw ? iw0 + (int)threadIdx.x : ih, lim = isw ? p.W : p.H, in = lim, out = isw ? p.OW : p.OH;
      const float sc = isw ? sw : sh;
      int lo = 0, cnt = 0; float wv[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k) wv[k] = 0.f;
      if (i < lim) {
        int hi; out_range(i, sc, out, lo, hi);
        while (lo < hi && tap_weight(lo, i, sc, in) == 0.f) ++lo;
        while (hi > lo && tap_weight(hi, i, sc, in) == 0.f) --hi;
        cnt = hi - lo + 1;
        if (cnt > MT) cnt = MT;                           // (cannot happen for the scales the host sends here)
#pragma unroll
        for (int k = 0; k < MT; ++k) wv[k] = k < cnt ? tap_weight(lo + k, i, sc, in) : 0.f;
      }
      if (isw) { lo_w[threadIdx.x] = lo; n_w[threadIdx.x] = cnt;
#pragma unroll
        for (int k = 0; k < MT; ++k) wt_w[threadIdx.x][k] = wv[k]; }
      else { lo_h = lo; n_h = cnt;
#pragma unroll
        for (int k = 0; k < MT; ++k) wt_h[k] = wv[k]; }
    }
    __syncthreads();
    if (!active) continue;
    const int nh = n_h, hlo = lo_h;
    for (int px = pl; px < tw; px += p.npl) {
      const int iw = iw0 + px;
      if (iw >= p.W) break;
      const int nw = n_w[px], wlo = lo_w[px];
      const long pp = (long)rowid * p.W + iw;
      float4 dz = zero4();
      float ww5[MT]; int wo5[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k) { ww5[k] = wt_w[px][k]; wo5[k] = (k < nw ? wlo + k : wlo) * p.lddy; }
      for (int a = 0; a < nh; ++a) {
        const float wh = wt_h[a];
        const float* rowp = p.dy + (long)(n * p.OH + hlo + a) * p.OW * p.lddy + c;
        float4 d5[MT];
#pragma unroll
        for (int b = 0; b < MT; ++b) d5[b] = ld4(rowp + wo5[b]);
#pragma unroll
        for (int b = 0; b < MT; ++b) dz = fma4(wh * ww5[b], d5[b], dz);
      }
      dz.x *= gs; dz.y *= gs; dz.z *= gs; dz.w *= gs;
      if (p.src.relu || p.dab) {
        const float4 x = ld4(p.src.x + pp * p.src.ld + c);
        if (p.src.relu) {
          if (!(fmaf(av.x, x.x, bv.x) > 0.f)) dz.x = 0.f;
          if (!(fmaf(av.y, x.y, bv.y) > 0.f)) dz.y = 0.f;
          if (!(fmaf(av.z, x.z, bv.z) > 0.f)) dz.z = 0.f;
          if (!(fmaf(av.w, x.w, bv.w) > 0.f)) dz.w = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { sA[e] += (double)get4(dz, e) * (double)get4(x, e); sB[e] += (double)get4(dz, e); }
      }
      float4 gv = make_float4(dz.x * av.x, dz.y * av.y, dz.z * av.z, dz.w * av.w);
      float* gp = p.g + pp * p.ldg + c;
      if (p.accumulate) { const float4 o = ld4(gp); gv.x += o.x; gv.y += o.y; gv.z += o.z; gv.w += o.w; }
      st4(gp, gv);
    }
  }
  if (p.dab) {
    const int C4 = p.nq * 4;
    __syncthreads();
    panel_sum(redt, sA, sB, active, pl, c, C, C4, p.npl, p.dab, bx);
  }
}

template <int MT>
__global__ void __launch_bounds__(256) resize_bwd_tab_kernel(const RsK p, int tiles_per_row, int ntiles, int tw) {
  resize_bwd_tab_body<MT>(p, tiles_per_row, ntiles, tw, blockIdx.x, gridDim.x);
}
// [r4] the mutually independent resize backwards of one dependency level (a dense-in cell receives up to ten resized feature maps,
// ADD.py:84-90: ten gathers of 15-18 us, each little more than its launch floor) in ONE launch: block (x, z) = workgroup x of table entry z
struct RsTabItem { RsK p; int tpr, ntiles, tw, rows; };
template <int MT>
__global__ void __launch_bounds__(256) resize_bwd_tab_batch_kernel(const RsTabItem* __restrict__ tab) {
  const RsTabItem& e = tab[blockIdx.z];
  if ((int)blockIdx.x >= e.rows) return;
  resize_bwd_tab_body<MT>(e.p, e.tpr, e.ntiles, e.tw, blockIdx.x, e.rows);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
// what the forward and the backward kernel argument share
RsK rs_fill(const addk_src& src, int N, int H, int W, int OH, int OW) {
  RsK k{};
  k.src = src; k.N = N; k.H = H; k.W = W; k.OH = OH; k.OW = OW;
  return k;
}

// Wide NHWC tensors (the concat buffers at F=40, level 3: 1600 channels) run as launches of at most 1024 channels (a workgroup holds 256 channel
// quads): rs_for_slices hands f the launch itself or, one after the other, its slices.  A launch that cannot be sliced goes to f whole and fails its checks.
constexpr int RS_SLICE = 1024;
template <class T> T* rs_at(T* p, int c0) { return p ? p + c0 : p; }
addk_src rs_slice_src(addk_src s, int c0) {
  s.C = s.C - c0 < RS_SLICE ? s.C - c0 : RS_SLICE;
  s.x = rs_at(s.x, c0); s.a = rs_at(s.a, c0); s.b = rs_at(s.b, c0);
  return s;
}
bool rs_sliced(const addk_resize_args* a) { return a && a->src.C > RS_SLICE && !a->nchw_out; }
bool rs_sliced(const addk_resize_bwd_args* a) { return a && a->src.C > RS_SLICE && !a->nchw_in && !a->dab; }
addk_resize_args rs_slice(addk_resize_args a, int c0) { a.src = rs_slice_src(a.src, c0); a.y = rs_at(a.y, c0); return a; }
addk_resize_bwd_args rs_slice(addk_resize_bwd_args a, int c0) { a.src = rs_slice_src(a.src, c0); a.dy = rs_at(a.dy, c0); a.g = rs_at(a.g, c0); return a; }
template <typename Args, typename F>
int rs_for_slices(const Args* a, F f) {
  if (!rs_sliced(a)) return f(a);
  for (int c0 = 0; c0 < a->src.C; c0 += RS_SLICE) {
    const Args b = rs_slice(*a, c0);
    if (const int rc = f(&b)) return rc;
  }
  return ADDK_OK;
}

int rs_fwd(const addk_resize_args* a, hipStream_t st) {
  ADDK_REQUIRE(a && a->src.x && a->y && a->src.C > 0 && a->src.C <= 1024 && a->src.ld >= a->src.C, "resize_fwd: bad args");
  ADDK_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0, "resize_fwd: empty shape");
  ADDK_REQUIRE((a->src.a == nullptr) == (a->src.b == nullptr), "resize_fwd: a/b must come together");
  RsK k = rs_fill(a->src, a->N, a->H, a->W, a->OH, a->OW);
  k.y = a->y; k.ldy = a->ldy; k.nchw = a->nchw_out;
  k.P = (long)a->N * a->OH * a->OW;
  if (a->nchw_out) {
    long b = cdiv(k.P, 256); if (b > 8192) b = 8192;
    hipLaunchKernelGGL(resize_fwd_nchw_kernel, dim3((unsigned)b), dim3(256), 0, st, k);
  } else {
    ADDK_REQUIRE(a->ldy >= a->src.C, "resize_fwd: short ldy");
    EwMap m = ew_map(a->src.C); k.nq = m.nq; k.npl = m.npl;
    k.vec = src_vec_ok(a->src) && aligned16(a->y) && a->ldy % 4 == 0;
    long b = cdiv(k.P, (long)m.npl); if (b > 8192) b = 8192; if (b < 1) b = 1;
    hipLaunchKernelGGL(resize_fwd_kernel, dim3((unsigned)b), dim3(256), 0, st, k);
  }
  return addk_check_launch("resize_fwd");
}

// The kernel of one resize backward launch of at most 1024 channels.  rs_choose_bwd checks the arguments and decides; the launch, the batch
// key and prepare and addk_resize_bwd_config read the choice.
enum { RS_NHWC = 0, RS_NHWC_TAB = 1, RS_NCHW = 2, RS_NCHW_TILE = 3 };
struct RsChoice {
  int kind, taps;           // taps: taps per axis of the table-driven kernel (its template parameter: 5 / 9 / 17), else 0
  RsTabItem it;             // it.p: the kernel argument of every kind; tpr, ntiles, tw, rows: the table-driven kernel's geometry and batch descriptor
  int tiles_x, tiles_y;     // RS_NCHW_TILE
  int gx, gy; size_t lds;   // grid and dynamic LDS bytes
  int key;                  // batch key (= taps): a table-driven launch, shares a batch with equal keys; -1: none
};

// The fast-path mask (ADDK_FAST_DWTILE) is tested here and nowhere else: it gates the launch as well as the key.
int rs_choose_bwd(const addk_resize_bwd_args* a, RsChoice& c) {
  ADDK_REQUIRE(a && a->dy && a->g && a->src.C > 0 && a->src.C <= 1024 && a->ldg >= a->src.C, "resize_bwd: bad args");
  ADDK_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->OH > 0 && a->OW > 0, "resize_bwd: empty shape");
  ADDK_REQUIRE(!(a->src.relu || a->dab) || (a->src.x && a->src.ld >= a->src.C), "resize_bwd: prologue needs the forward input");
  ADDK_REQUIRE((a->src.a == nullptr) == (a->src.b == nullptr), "resize_bwd: a/b must come together");
  ADDK_REQUIRE(!a->nchw_in || (!a->src.relu && !a->dab), "resize_bwd: NCHW gradient input has no prologue support");
  ADDK_REQUIRE(a->nchw_in || a->lddy >= a->src.C, "resize_bwd: short lddy");
  c = RsChoice{};
  RsK& k = c.it.p = rs_fill(a->src, a->N, a->H, a->W, a->OH, a->OW);
  k.dy = a->dy; k.lddy = a->lddy; k.dy_scale = a->dy_scale; k.g = a->g; k.ldg = a->ldg; k.accumulate = a->accumulate; k.dab = (double*)a->dab;
  k.P = (long)a->N * a->H * a->W;
  c.gy = 1; c.key = -1;
  const bool fast = (addk_get_fast_paths() & ADDK_FAST_DWTILE) != 0;
  if (a->nchw_in) {
    k.nq = 1; k.npl = 256;
    // receptive block of an 8x8 tile: (8 + 2) / scale + 4 output rows / columns (out_range's margins), at most RB_PM
    const float invh = (float)a->OH / (float)a->H, invw = (float)a->OW / (float)a->W;
    const bool fits = (RB_T + 2) * invh + 5.f <= (float)RB_PM && (RB_T + 2) * invw + 5.f <= (float)RB_PM &&
                      2.f * invh + 5.f <= (float)RB_MAXT && 2.f * invw + 5.f <= (float)RB_MAXT && invh >= 1.f && invw >= 1.f;
    c.kind = fits && fast ? RS_NCHW_TILE : RS_NCHW;
    c.tiles_x = cdiv(a->W, RB_T); c.tiles_y = cdiv(a->H, RB_T);
    if (c.kind == RS_NCHW_TILE) { c.gx = a->N * c.tiles_y * c.tiles_x; c.gy = a->src.C; }
    else c.gx = cdiv(k.P, 256) > 8192 ? 8192 : cdiv(k.P, 256);
    return ADDK_OK;
  }
  EwMap m = ew_map(a->src.C); k.nq = m.nq; k.npl = m.npl;
  k.vec = aligned16(a->dy) && a->lddy % 4 == 0 && aligned16(a->g) && a->ldg % 4 == 0 && a->src.C % 4 == 0 && (!a->src.x || src_vec_ok(a->src));
  c.kind = RS_NHWC;
  c.gx = c.it.rows = ew_rows(k.P, a->src.C);
  c.lds = (size_t)m.npl * m.nq * 4 * 2 * sizeof(double);
  // the table-driven kernel: at most x2 / x4 / x8 up-sampling (<= 5 / 9 / 17 taps per axis), vector-aligned, a few pixel lanes per workgroup
  const bool up2 = a->OH <= 2 * a->H + 1 && a->OW <= 2 * a->W + 1, up4 = a->OH <= 4 * a->H + 1 && a->OW <= 4 * a->W + 1,
             up8 = a->OH <= 8 * a->H + 1 && a->OW <= 8 * a->W + 1;
  if (!(k.vec && a->src.C == m.nq * 4 && m.npl >= 2 && (up2 || up4 || up8) && fast && k.P < (1L << 30))) return ADDK_OK;
  int tw = m.npl >= 4 ? m.npl * 4 : m.npl * 8; if (tw > RT_MAXW) tw = RT_MAXW; if (tw > a->W) tw = a->W;      // (2-3 pixel lanes: 260-512 channels)
  c.kind = RS_NHWC_TAB; c.taps = c.key = up2 ? 5 : up4 ? 9 : 17;
  c.it.tpr = cdiv(a->W, tw); c.it.ntiles = a->N * a->H * c.it.tpr; c.it.tw = tw;
  return ADDK_OK;
}

int rs_launch_bwd(const RsChoice& c, hipStream_t st) {
  const RsTabItem& t = c.it;
  const dim3 grid((unsigned)c.gx, (unsigned)c.gy);
  if (c.kind == RS_NHWC_TAB) {
    if (c.taps == 5) hipLaunchKernelGGL(resize_bwd_tab_kernel<5>, grid, dim3(256), c.lds, st, t.p, t.tpr, t.ntiles, t.tw);
    else if (c.taps == 9) hipLaunchKernelGGL(resize_bwd_tab_kernel<9>, grid, dim3(256), c.lds, st, t.p, t.tpr, t.ntiles, t.tw);
    else hipLaunchKernelGGL(resize_bwd_tab_kernel<17>, grid, dim3(256), c.lds, st, t.p, t.tpr, t.ntiles, t.tw);
    return addk_check_launch("resize_bwd_tab");
  }
  if (c.kind == RS_NCHW_TILE) {
    hipLaunchKernelGGL(resize_bwd_nchw_tile_kernel, grid, dim3(256), 0, st, t.p, c.tiles_x, c.tiles_y);
    return addk_check_launch("resize_bwd_nchw_tile");
  }
  if (c.kind == RS_NCHW) hipLaunchKernelGGL(resize_bwd_kernel<true>, grid, dim3(256), 0, st, t.p);
  else hipLaunchKernelGGL(resize_bwd_kernel<false>, grid, dim3(256), c.lds, st, t.p);
  return addk_check_launch("resize_bwd");
}

}  // namespace

extern "C" int addk_resize_fwd(const addk_resize_args* a, void* stream) {
  return rs_for_slices(a, [stream](const addk_resize_args* s) { return rs_fwd(s, (hipStream_t)stream); });
}

extern "C" int addk_resize_bwd(const addk_resize_bwd_args* a, void* stream) {
  return rs_for_slices(a, [stream](const addk_resize_bwd_args* s) {
    RsChoice c;
    const int rc = rs_choose_bwd(s, c);
    return rc ? rc : rs_launch_bwd(c, (hipStream_t)stream);
  });
}

// cfg[8]: include/addk.h.  A launch of more than 1024 channels reports its first slice and the number of slices (its key is -1: it is no single launch).
extern "C" int addk_resize_bwd_config(const addk_resize_bwd_args* a, int32_t* cfg) {
  ADDK_REQUIRE(cfg, "resize_bwd_config: null cfg");
  const bool sliced = rs_sliced(a);
  const addk_resize_bwd_args first = sliced ? rs_slice(*a, 0) : addk_resize_bwd_args{};
  RsChoice c;
  if (const int rc = rs_choose_bwd(sliced ? &first : a, c)) return rc;
  cfg[0] = c.kind; cfg[1] = c.taps; cfg[2] = c.gx; cfg[3] = c.gy; cfg[4] = (int32_t)c.lds; cfg[5] = c.kind == RS_NHWC_TAB ? c.it.tw : 0;
  cfg[6] = sliced ? cdiv(a->src.C, RS_SLICE) : 1; cfg[7] = sliced ? -1 : c.key;
  return ADDK_OK;
}

// batched form: key >= 0 (the kernel variant) when the launch runs on the table-driven kernel and may share a batch
// Kept on purpose: an argument struct that addk_resize_bwd rejects with an error has key -1 (no error: the plan asks for the key of every
// launch it records), and a rejected item makes prepare fail like any other item that does not run on the table-driven kernel.
extern "C" int addk_resize_bwd_batch_key(const addk_resize_bwd_args* a) { RsChoice c; return rs_choose_bwd(a, c) == ADDK_OK ? c.key : -1; }
// host_blob = NULL: returns the blob size in bytes.  meta[0..3] = variant, n, grid x, dynamic LDS bytes
extern "C" int64_t addk_resize_bwd_batch_prepare(const addk_resize_bwd_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta) {
  size_t lds = 0;
  const int64_t total = batch_prepare<RsTabItem>("resize_bwd_batch_prepare", a, n, host_blob, blob_bytes, meta, [](const addk_resize_bwd_args* x, RsTabItem& it, BatchItem& b) {
    RsChoice c;
    if (rs_choose_bwd(x, c) != ADDK_OK || c.key < 0) return false;
    it = c.it; b = BatchItem{c.key, c.gx, c.gy, c.lds};
    return true;
  }, &lds);
  if (total > 0) meta[3] = (int64_t)lds;
  return total;
}
extern "C" int addk_resize_bwd_batch_run(const void* dev_blob, const int64_t* meta, void* stream) {
  ADDK_REQUIRE(dev_blob && meta && meta[1] > 0 && meta[2] > 0, "resize_bwd_batch_run: bad args");
  const RsTabItem* tab = reinterpret_cast<const RsTabItem*>(dev_blob);
  const dim3 grid((unsigned)meta[2], 1, (unsigned)meta[1]);
  hipStream_t st = (hipStream_t)stream;
  if (meta[0] == 5) hipLaunchKernelGGL(resize_bwd_tab_batch_kernel<5>, grid, dim3(256), (size_t)meta[3], st, tab);      // the batch kernels' own ladder (as dw_batch_run)
  else if (meta[0] == 9) hipLaunchKernelGGL(resize_bwd_tab_batch_kernel<9>, grid, dim3(256), (size_t)meta[3], st, tab);
  else if (meta[0] == 17) hipLaunchKernelGGL(resize_bwd_tab_batch_kernel<17>, grid, dim3(256), (size_t)meta[3], st, tab);
  else { addk_set_error("resize_bwd_batch_run: unknown variant %d", (int)meta[0]); return ADDK_ERR_INVALID; }
  return addk_check_launch("resize_bwd_batch");
}
