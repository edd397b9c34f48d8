// The inference heads on the decoder's low-resolution logits: the label map of one exit (label_up_kernel), of several views
// (label_views_kernel), of the sliding windows that cover an image (label_tiles_kernel), of the sliding windows of several scaled and
// mirrored views (label_tile_views_kernel), and the early-exit gate with and without the label map, plain and tempered (gate_up_kernel).
#include "up.h"

namespace {

// ---- fused logits up-sampling + label map (decoder.py:28 + eval.py:218-221) ------------------------------------------------------
// What inference keeps of an exit: the arg-max of the up-sampled logits, one byte per high-resolution pixel.  The walk is scu_walk
// (same tile, same interpolation), then the strict `>` arg-max sweep of score_up_kernel (a tie keeps the lowest channel) and one
// byte store — the class index, or lut[class] (train id -> Cityscapes labelId).  No exp, no LDS, no workspace; a wave row stores 64
// consecutive bytes.  label_px is also the store of the gate launch that leaves the map (gate_up_kernel<.., LABELS = true>).
struct LabelUpK : UpSrc { const uint8_t* lut; uint8_t* labels; };

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) label_up_kernel(const LabelUpK p) {
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    float mx = -INFINITY; int am = 0;
#pragma unroll
    for (int c = 0; c < CC; ++c)
      if (z[c] > mx) { mx = z[c]; am = c; }                      // strict: a tie keeps the lowest channel
    label_px(p.lut, p.labels, pix, am);
  });
}

// ---- fused multi-view label map: up-sample, softmax, weighted sum over views, arg-max (multi-scale + flip inference) -----------------
// What a multi-scale submission keeps: the arg-max of the weighted mean of the class probabilities of up to 8 views of one image —
// low-resolution NHWC maps of different sizes, some of them horizontally mirrored — one byte per high-resolution pixel.  A wave owns
// 64 consecutive output columns and LVU_R rows; a thread owns one column X.  The view loop is outermost (run-time count, descriptors
// from the argument block: wave-uniform).  Within a view the thread samples column Xv = mirror ? OW-1-X : X with the walk of scu_walk:
// the two W-interpolated rows t0 / t1 stay in registers and are reloaded only when the wave-uniform row pair changes, z = lh0*t0 +
// lh1*t1 carries the bits addk_resize_fwd writes at (Y, Xv).  Then max, exp sweep, acc[r][c] += (weight / Σe) * e[c]; acc[LVU_R][CC]
// lives in registers (the row loop is fully unrolled: nothing is indexed at run time).  After the last view: the strict `>` arg-max of
// acc and label_px.  No LDS, no atomics, no workspace; the maps (a few MB) stay in L2, HBM sees the one byte per pixel.
constexpr int LVU_W = 64, LVU_WAVES = 4, LVU_R = 4;      // tile: 64 columns x (4 waves x 4 rows)

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) label_views_kernel(const addk_label_views_args p) {
  const int lane = threadIdx.x & (LVU_W - 1), wv = threadIdx.x / LVU_W;
  const int X = blockIdx.x * LVU_W + lane, n = blockIdx.z;
  if (X >= p.OW) return;
  const int ybeg = (blockIdx.y * LVU_WAVES + wv) * LVU_R;
  float acc[LVU_R][CC];
#pragma unroll
  for (int r = 0; r < LVU_R; ++r)
#pragma unroll
    for (int c = 0; c < CC; ++c) acc[r][c] = 0.f;
  for (int v = 0; v < p.nview; ++v) {
    const float* x = p.view[v].logits;
    const int ld = p.view[v].ld, H = p.view[v].H, W = p.view[v].W;
    const long img = (long)(p.view[v].n0 + n) * H;
    const float wt = p.view[v].weight;
    const float sh = (float)H / (float)p.OH, sw = (float)W / (float)p.OW;
    int w0, w1; float lw0, lw1;
    src_index(p.view[v].mirror ? p.OW - 1 - X : X, sw, W, w0, w1, lw0, lw1);
    float t0[CC], t1[CC];
    int ph0 = -1, ph1 = -1;
#pragma unroll
    for (int r = 0; r < LVU_R; ++r) {
      const int Y = ybeg + r;
      if (Y < p.OH) {                                              // wave-uniform
        int h0, h1; float lh0, lh1;
        src_index(Y, sh, H, h0, h1, lh0, lh1);
        if (h0 != ph0 || h1 != ph1) {                              // wave-uniform
          const float* r0 = x + ((img + h0) * W) * ld;
          const float* r1 = x + ((img + h1) * W) * ld;
          float a[cpad(CC)], b[cpad(CC)];
          load_px<CC>(r0 + (long)w0 * ld, a, VEC); load_px<CC>(r0 + (long)w1 * ld, b, VEC);
#pragma unroll
          for (int c = 0; c < CC; ++c) t0[c] = lw0 * a[c] + lw1 * b[c];
          load_px<CC>(r1 + (long)w0 * ld, a, VEC); load_px<CC>(r1 + (long)w1 * ld, b, VEC);
#pragma unroll
          for (int c = 0; c < CC; ++c) t1[c] = lw0 * a[c] + lw1 * b[c];
          ph0 = h0; ph1 = h1;
        }
        float e[CC];
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < CC; ++c) { e[c] = lh0 * t0[c] + lh1 * t1[c]; mx = fmaxf(mx, e[c]); }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < CC; ++c) { e[c] = __expf(e[c] - mx); se += e[c]; }
        const float s = wt / se;
#pragma unroll
        for (int c = 0; c < CC; ++c) acc[r][c] += s * e[c];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LVU_R; ++r) {
    const int Y = ybeg + r;
    if (Y < p.OH) {
      float mx = -INFINITY; int am = 0;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (acc[r][c] > mx) { mx = acc[r][c]; am = c; }            // strict: a tie keeps the lowest channel
      label_px(p.lut256, p.labels, ((long)n * p.OH + Y) * p.OW + X, am);
    }
  }
}

dim3 lvu_grid(int N, int OH, int OW) { return dim3(cdiv(OW, LVU_W), cdiv(OH, LVU_WAVES * LVU_R), N); }
bool lvu_ok(int nview, int N, int OH, int OW, int C) {
  if (nview < 1 || nview > ADDK_MAX_VIEWS || !gate_class_ok(C) || N <= 0 || OH <= 0 || OW <= 0) return false;
  const dim3 g = lvu_grid(N, OH, OW);
  return N <= 65535 && g.y <= 65535 && (long)(int)g.z * (int)g.y * (int)g.x < (1L << 30);
}

// ---- fused tiled label map: up-sample every window that covers a pixel, softmax, sum, arg-max (sliding-window inference) ------------
// What sliding-window inference keeps: the arg-max of the summed class probabilities of the windows that cover a pixel, one byte per
// image pixel, from the stored low-resolution NHWC logits of the windows (all of one grid (h, w), one size (th, tw) in output pixels).
// The tile and the walk are label_views_kernel's: a wave owns 64 consecutive columns and LVU_R rows, a thread one column X, acc[LVU_R][CC]
// lives in registers.  The window grid is ny x nx origins from the argument block.  The window-row loop and its cover test are wave-
// uniform (a wave's rows are the same in every lane); the window-column cover test is per lane: a lane outside [x0, x0 + tw) sits the
// window out — it loads nothing and adds nothing — and a wave with no lane inside skips it.  Within a window the two W-interpolated rows
// t0 / t1 are reloaded only when the wave-uniform row pair changes; z = lh0*t0 + lh1*t1 carries the bits addk_resize_fwd writes at
// (Y - y0, X - x0) of a (h, w) -> (th, tw) resize.  Clamped last windows let three or more windows overlap on an axis: nothing here
// counts on two.  Rows Y >= OH are never sampled, so the padded part of a window larger than the image is not.  No LDS, no atomics, no
// workspace: every pixel's sum runs in the same order (ascending iy, then ix) on every launch.
template <int CC, bool VEC>
__global__ void __launch_bounds__(256) label_tiles_kernel(const addk_label_tiles_args p) {
  const int lane = threadIdx.x & (LVU_W - 1), wv = threadIdx.x / LVU_W;
  const int X = blockIdx.x * LVU_W + lane, n = blockIdx.z;
  if (X >= p.OW) return;
  const int ybeg = (blockIdx.y * LVU_WAVES + wv) * LVU_R;
  if (ybeg >= p.OH) return;                                            // wave-uniform
  const int ylast = (ybeg + LVU_R < p.OH ? ybeg + LVU_R : p.OH) - 1;
  const float sh = (float)p.h / (float)p.th, sw = (float)p.w / (float)p.tw;
  const long tile_floats = (long)p.h * p.w * p.ld;
  float acc[LVU_R][CC];
#pragma unroll
  for (int r = 0; r < LVU_R; ++r)
#pragma unroll
    for (int c = 0; c < CC; ++c) acc[r][c] = 0.f;
  for (int iy = 0; iy < p.ny; ++iy) {
    const int y0 = p.y0[iy];
    if (y0 > ylast || y0 + p.th <= ybeg) continue;                      // wave-uniform: the window row misses this wave's rows
    for (int ix = 0; ix < p.nx; ++ix) {
      const int lx = X - p.x0[ix];
      if (lx >= 0 && lx < p.tw) {                                       // per lane: this window covers column X
        const float* x = p.logits + ((long)p.t0 + ((long)n * p.ny + iy) * p.nx + ix) * tile_floats;
        int w0, w1; float lw0, lw1;
        src_index(lx, sw, p.w, w0, w1, lw0, lw1);
        float t0[CC], t1[CC];
        int ph0 = -1, ph1 = -1;
#pragma unroll
        for (int r = 0; r < LVU_R; ++r) {
          const int ly = ybeg + r - y0;
          if (ybeg + r < p.OH && ly >= 0 && ly < p.th) {               // wave-uniform
            int h0, h1; float lh0, lh1;
            src_index(ly, sh, p.h, h0, h1, lh0, lh1);
            if (h0 != ph0 || h1 != ph1) {                              // wave-uniform
              const float* r0 = x + ((long)h0 * p.w) * p.ld;
              const float* r1 = x + ((long)h1 * p.w) * p.ld;
              float a[cpad(CC)], b[cpad(CC)];
              load_px<CC>(r0 + (long)w0 * p.ld, a, VEC); load_px<CC>(r0 + (long)w1 * p.ld, b, VEC);
#pragma unroll
              for (int c = 0; c < CC; ++c) t0[c] = lw0 * a[c] + lw1 * b[c];
              load_px<CC>(r1 + (long)w0 * p.ld, a, VEC); load_px<CC>(r1 + (long)w1 * p.ld, b, VEC);
#pragma unroll
              for (int c = 0; c < CC; ++c) t1[c] = lw0 * a[c] + lw1 * b[c];
              ph0 = h0; ph1 = h1;
            }
            float e[CC];
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < CC; ++c) { e[c] = lh0 * t0[c] + lh1 * t1[c]; mx = fmaxf(mx, e[c]); }
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < CC; ++c) { e[c] = __expf(e[c] - mx); se += e[c]; }
            const float s = 1.0f / se;
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[r][c] += s * e[c];
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LVU_R; ++r) {
    const int Y = ybeg + r;
    if (Y < p.OH) {
      float mx = -INFINITY; int am = 0;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (acc[r][c] > mx) { mx = acc[r][c]; am = c; }            // strict: a tie keeps the lowest channel
      label_px(p.lut256, p.labels, ((long)n * p.OH + Y) * p.OW + X, am);
    }
  }
}

bool ltu_ok(int N, int OH, int OW, int ny, int nx, int C) {
  if (!head_class_ok(C) || ny < 1 || ny > ADDK_MAX_TILES_AXIS || nx < 1 || nx > ADDK_MAX_TILES_AXIS || N <= 0 || OH <= 0 || OW <= 0) return false;
  const dim3 g = lvu_grid(N, OH, OW);
  return N <= 65535 && g.y <= 65535 && (long)(int)g.z * (int)g.y * (int)g.x < (1L << 30);
}
// the origins of one axis are a window grid of an image of L pixels: from 0, strictly increasing, no gap, inside the image, up to its end
bool ltu_axis_ok(const int32_t* o, int n, int t, int L) {
  if (o[0] != 0) return false;
  for (int i = 0; i < n; ++i) {
    if (o[i] < 0 || o[i] >= L) return false;
    if (i + 1 < n && (o[i + 1] <= o[i] || (long)o[i + 1] > (long)o[i] + t)) return false;
  }
  return (long)o[n - 1] + t >= L;
}

// ---- fused tiled multi-view label map: the windows of several scaled / mirrored views that cover a pixel (multi-scale + flip sliding windows) ----
// What a multi-scale, flipped sliding-window evaluation keeps: the arg-max of the weighted mean over views of the MEAN class probabilities
// of the view's windows that cover a pixel.  View v's windows lie on its scaled image (Hv, Wv); output pixel (Y, X) sits there at
// u = ((Y + 1/2) Hv/OH, (Xm + 1/2) Wv/OW), Xm the mirrored column, and is covered by window (iy, ix) iff y0 <= u_y < y0 + th and
// x0 <= u_x < x0 + tw — decided in 64-bit integers, 2 OH y0 <= (2Y+1) Hv < 2 OH (y0 + th), so no rounding moves a pixel in or out of a
// window.  The tile and the walk are label_tiles_kernel's: a wave owns 64 columns and LTV_R rows, a thread one column, acc[LTV_R][CC] in
// registers.  Per view the covering window rows of each of the wave's rows (bit mask rm[r]) and the weight over the cover count are wave-
// uniform; the covering window columns (bit mask cm) and their count are per lane.  A window samples its logits at a = (u - origin) * h/th - 1/2
// with src_index's border rule (src_at); at scale 1 the coordinate and z = lh0*t0 + lh1*t1 carry label_tiles_kernel's bits.  The row pair
// t0 / t1 is reloaded only when the wave-uniform row pair changes.  Dividing by the cover count is what lets views with different overlap
// be averaged.  No LDS, no atomics, no workspace: a pixel's sum runs in the same order (view, iy, ix) on every launch.
constexpr int LTV_R = LVU_R;

// src_index's tail for a source coordinate that is already computed
__device__ __forceinline__ void src_at(float s, int in, int& i0, int& i1, float& l0, float& l1) {
  if (!(s >= 0.f)) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) label_tile_views_kernel(const addk_label_tile_views_args p) {
  const int lane = threadIdx.x & (LVU_W - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x / LVU_W);
  const int X = blockIdx.x * LVU_W + lane, n = blockIdx.z;
  if (X >= p.OW) return;
  const int ybeg = (blockIdx.y * LVU_WAVES + wv) * LTV_R;
  if (ybeg >= p.OH) return;                                            // wave-uniform
  const float sh = (float)p.h / (float)p.th, sw = (float)p.w / (float)p.tw;
  const long tile_floats = (long)p.h * p.w * p.ld;
  const long OH2 = 2L * p.OH, OW2 = 2L * p.OW;
  float acc[LTV_R][CC];
#pragma unroll
  for (int r = 0; r < LTV_R; ++r)
#pragma unroll
    for (int c = 0; c < CC; ++c) acc[r][c] = 0.f;
  for (int v = 0; v < p.nview; ++v) {
    const addk_tile_view& V = p.view[v];
    const int ny = V.ny, nx = V.nx;
    const int Xm = V.mirror ? p.OW - 1 - X : X;
    const long cx = (long)(2 * Xm + 1) * V.Wv;
    unsigned cm = 0;                                                    // per lane: the window columns that cover X
    for (int ix = 0; ix < nx; ++ix) {
      const long lo = OW2 * V.x0[ix];
      if (lo <= cx && cx < lo + OW2 * p.tw) cm |= 1u << ix;
    }
    const int kx = __popc(cm);
    unsigned rm[LTV_R], rows = 0;                                       // wave-uniform: the window rows that cover row ybeg + r
    float wk[LTV_R];
#pragma unroll
    for (int r = 0; r < LTV_R; ++r) {
      rm[r] = 0;
      if (ybeg + r < p.OH) {
        const long cy = (long)(2 * (ybeg + r) + 1) * V.Hv;
        for (int iy = 0; iy < ny; ++iy) {
          const long lo = OH2 * V.y0[iy];
          if (lo <= cy && cy < lo + OH2 * p.th) rm[r] |= 1u << iy;
        }
      }
      rows |= rm[r];
      const int k = __popc(rm[r]) * kx;
      wk[r] = V.weight / (float)(k > 0 ? k : 1);
    }
    const float ux = ((float)Xm + 0.5f) * ((float)V.Wv / (float)p.OW);
    const float rh = (float)V.Hv / (float)p.OH;
    for (int iy = 0; iy < ny; ++iy) {
      if (!((rows >> iy) & 1u)) continue;                               // wave-uniform: the window row misses this wave's rows
      const float fy0 = (float)V.y0[iy];
      for (int ix = 0; ix < nx; ++ix) {
        if ((cm >> ix) & 1u) {                                          // per lane: this window covers column X
          const float* x = p.logits + ((long)V.t0 + ((long)n * ny + iy) * nx + ix) * tile_floats;
          int w0, w1; float lw0, lw1;
          src_at((ux - (float)V.x0[ix]) * sw - 0.5f, p.w, w0, w1, lw0, lw1);
          float t0[CC], t1[CC];
          int ph0 = -1, ph1 = -1;
#pragma unroll
          for (int r = 0; r < LTV_R; ++r) {
            if ((rm[r] >> iy) & 1u) {                                   // wave-uniform
              const float uy = ((float)(ybeg + r) + 0.5f) * rh;
              int h0, h1; float lh0, lh1;
              src_at((uy - fy0) * sh - 0.5f, p.h, h0, h1, lh0, lh1);
              if (h0 != ph0 || h1 != ph1) {                             // wave-uniform
                const float* r0 = x + ((long)h0 * p.w) * p.ld;
                const float* r1 = x + ((long)h1 * p.w) * p.ld;
                float a[cpad(CC)], b[cpad(CC)];
                load_px<CC>(r0 + (long)w0 * p.ld, a, VEC); load_px<CC>(r0 + (long)w1 * p.ld, b, VEC);
#pragma unroll
                for (int c = 0; c < CC; ++c) t0[c] = lw0 * a[c] + lw1 * b[c];
                load_px<CC>(r1 + (long)w0 * p.ld, a, VEC); load_px<CC>(r1 + (long)w1 * p.ld, b, VEC);
#pragma unroll
                for (int c = 0; c < CC; ++c) t1[c] = lw0 * a[c] + lw1 * b[c];
                ph0 = h0; ph1 = h1;
              }
              float e[CC];
              float mx = -INFINITY;
#pragma unroll
              for (int c = 0; c < CC; ++c) { e[c] = lh0 * t0[c] + lh1 * t1[c]; mx = fmaxf(mx, e[c]); }
              float se = 0.f;
#pragma unroll
              for (int c = 0; c < CC; ++c) { e[c] = __expf(e[c] - mx); se += e[c]; }
              const float s = wk[r] / se;
#pragma unroll
              for (int c = 0; c < CC; ++c) acc[r][c] += s * e[c];
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LTV_R; ++r) {
    const int Y = ybeg + r;
    if (Y < p.OH) {
      float mx = -INFINITY; int am = 0;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (acc[r][c] > mx) { mx = acc[r][c]; am = c; }            // strict: a tie keeps the lowest channel
      label_px(p.lut256, p.labels, ((long)n * p.OH + Y) * p.OW + X, am);
    }
  }
}

dim3 ltv_grid(int N, int OH, int OW) { return dim3(cdiv(OW, LVU_W), cdiv(OH, LVU_WAVES * LTV_R), N); }
bool ltv_ok(int nview, int N, int OH, int OW, int C) {
  if (nview < 1 || nview > ADDK_MAX_VIEWS || !head_class_ok(C) || N <= 0 || OH <= 0 || OW <= 0) return false;
  const dim3 g = ltv_grid(N, OH, OW);
  return N <= 65535 && g.y <= 65535 && (long)(int)g.z * (int)g.y * (int)g.x < (1L << 30);
}

// ---- fused logits up-sampling + early-exit gate (decoder.py:28 + operations.py:161-180) -----------------------------------
// The two gates of dynamic inference that need no trained EDM: the normalised Shannon entropy of the up-sampled prediction and the
// share of pixels whose top softmax probability passes a threshold.  The walk is scu_walk (same tile, same interpolation
// z = lh0*t0 + lh1*t1), then one max sweep and the exp sweep; no target, histogram, loss or map.  Per pixel: se = Σe, sx = Σe·d with
// d = z - max, entropy term log se - sx/se, top probability pmax = 1/se (the largest e is exp(0) = 1), counted when pmax > *max_thr.
// A workgroup leaves one fp32 entropy partial and one count, write-through; the workgroup that arrives LAST (csrc/bnfin.h ticket, as
// csrc/edm.hip) adds each image's partials in a FIXED order (fp64; the counts are integers), writes (entropy, share) to `out` and to
// the pinned host words the gate reads, and puts the ticket back to zero: one launch, bit-reproducible, graph-replayable, nothing spins.
struct GateUpK : UpSrc {
  const float* thr;
  float* out; float* out_host;
  unsigned* counter; float* part; unsigned* cnt;          // ws: [ticket, 16 bytes][nblk floats][nblk counts], image-major
  int nblk_img;
  double npix, ent_div;                                    // OH*OW and log(19) * OH*OW (up.h, up_tail_fill)
};

// LABELS: the launch also leaves the label map of label_up_kernel, speculatively, for every image (one byte per pixel): the max sweep
// becomes the strict `>` arg-max sweep, which leaves the max that fmaxf leaves, so `out` / `out_host` carry the bits of the plain gate
struct GateLabelUpK : GateUpK { const uint8_t* lut; uint8_t* labels; };
// TEMP: the tempered launch (addk_gate_upsample_t) judges softmax(z * *inv_temp); the word rides behind the untempered arguments, whose
// layout and kernels stay as they are
template <class K> struct Tempered : K { const float* inv_temp; };
template <bool LABELS, bool TEMP = false> struct GateUpArg { typedef GateUpK type; };
template <> struct GateUpArg<true, false> { typedef GateLabelUpK type; };
template <> struct GateUpArg<false, true> { typedef Tempered<GateUpK> type; };
template <> struct GateUpArg<true, true> { typedef Tempered<GateLabelUpK> type; };

template <int CC, bool VEC, bool LABELS = false, bool TEMP = false>
__global__ void __launch_bounds__(256) gate_up_kernel(const typename GateUpArg<LABELS, TEMP>::type p) {
  const float thr = *(const gfloat*)p.thr;
  float it = 1.f;
  if constexpr (TEMP) it = *(const gfloat*)p.inv_temp;
  float esum = 0.f; unsigned hit[1] = {0u};
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    float mx = -INFINITY;
    if constexpr (LABELS) {
      int am = 0;
#pragma unroll
      for (int c = 0; c < CC; ++c)
        if (z[c] > mx) { mx = z[c]; am = c; }                    // strict: a tie keeps the lowest channel
      label_px(p.lut, p.labels, pix, am);
    } else {
#pragma unroll
      for (int c = 0; c < CC; ++c) mx = fmaxf(mx, z[c]);
    }
    float se, sx;
    if constexpr (TEMP) exp_sweep_t<CC>(z, mx, it, se, sx);
    else exp_sweep<CC>(z, mx, se, sx);
    esum += logf(se) - sx / se;
    hit[0] += (1.f / se > thr) ? 1u : 0u;
  });
  up_finish<1>(esum, hit, 1, p.counter, p.part, p.cnt, p.N, p.nblk_img, p.out_host != nullptr, [&](int img, double es, auto&& count) {
    const float ent = (float)(es / p.ent_div), share = (float)((double)count(0) / p.npix);
    ((gfloat*)p.out)[2 * img] = ent; ((gfloat*)p.out)[2 * img + 1] = share;
    if (p.out_host) { p.out_host[2 * img] = ent; p.out_host[2 * img + 1] = share; }
  });
}

// the gate launch's arguments behind the UpSrc prefix (both of its forms): outputs, workspace layout, normalisation
void gate_up_fill(GateUpK& k, const addk_gate_upsample_args* a) {
  static_cast<UpSrc&>(k) = up_src(a);
  k.thr = a->max_thr; k.out = a->out; k.out_host = a->out_host;
  up_tail_fill(k, a->ws, a->N, a->OH, a->OW);
}

}  // namespace

extern "C" int addk_gate_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return scu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_gate_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  return up_ws_bytes(N, OH, OW, 1);
}
extern "C" int addk_gate_upsample(const addk_gate_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->max_thr && a->out && a->ws, "gate_upsample: null pointer");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "gate_upsample: unsupported shape (%s)", gate_classes_text().c_str());
  ADDK_REQUIRE(a->ld >= a->C, "gate_upsample: short stride");
  GateUpK k;
  gate_up_fill(k, a);
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), gate_up_kernel<CC, true>, gate_up_kernel<CC, false>, scu_grid(a->N, a->OH, a->OW), st, k);
  });
  return addk_check_launch("gate_upsample");
}
extern "C" int addk_gate_label_upsample(const addk_gate_label_upsample_args* b, void* stream) {
  ADDK_REQUIRE(b, "gate_label_upsample: null pointer");
  const addk_gate_upsample_args* a = &b->gate;
  ADDK_REQUIRE(a->logits && a->max_thr && a->out && a->ws && b->labels, "gate_label_upsample: null pointer");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "gate_label_upsample: unsupported shape (%s)", gate_classes_text().c_str());
  ADDK_REQUIRE(a->ld >= a->C, "gate_label_upsample: short stride");
  GateLabelUpK k;
  gate_up_fill(k, a);
  k.lut = b->lut256; k.labels = b->labels;
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), gate_up_kernel<CC, true, true>, gate_up_kernel<CC, false, true>, scu_grid(a->N, a->OH, a->OW), st, k);
  });
  return addk_check_launch("gate_label_upsample");
}

extern "C" int addk_gate_upsample_t(const addk_gate_upsample_t_args* b, void* stream) {
  ADDK_REQUIRE(b, "gate_upsample_t: null pointer");
  const addk_gate_upsample_args* a = &b->gate;
  ADDK_REQUIRE(a->logits && a->max_thr && a->out && a->ws && b->inv_temp, "gate_upsample_t: null pointer");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "gate_upsample_t: unsupported shape (%s)", gate_classes_text().c_str());
  ADDK_REQUIRE(a->ld >= a->C, "gate_upsample_t: short stride");
  const dim3 grid = scu_grid(a->N, a->OH, a->OW);
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    const bool vec = px_vec_ok<CC>(a->logits, a->ld);
    if (b->labels) {
      Tempered<GateLabelUpK> k;
      gate_up_fill(k, a);
      k.lut = b->lut256; k.labels = b->labels; k.inv_temp = b->inv_temp;
      launch_vec(vec, gate_up_kernel<CC, true, true, true>, gate_up_kernel<CC, false, true, true>, grid, st, k);
    } else {
      Tempered<GateUpK> k;
      gate_up_fill(k, a);
      k.inv_temp = b->inv_temp;
      launch_vec(vec, gate_up_kernel<CC, true, false, true>, gate_up_kernel<CC, false, false, true>, grid, st, k);
    }
  });
  return addk_check_launch("gate_upsample_t");
}

extern "C" int addk_label_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return scu_head_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int addk_label_upsample(const addk_label_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->labels, "label_upsample: null pointer");
  ADDK_REQUIRE(scu_head_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "label_upsample: unsupported shape (%s)", head_classes_text().c_str());
  ADDK_REQUIRE(a->ld >= a->C, "label_upsample: short stride");
  LabelUpK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.lut = a->lut256; k.labels = a->labels;
  hipStream_t st = (hipStream_t)stream;
  head_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), label_up_kernel<CC, true>, label_up_kernel<CC, false>, scu_grid(a->N, a->OH, a->OW), st, k);
  });
  return addk_check_launch("label_upsample");
}

extern "C" int addk_label_views_upsample_supported(int32_t nview, int32_t N, int32_t OH, int32_t OW, int32_t C) {
  return lvu_ok(nview, N, OH, OW, C) ? 1 : 0;
}
extern "C" int addk_label_views_upsample(const addk_label_views_args* a, void* stream) {
  ADDK_REQUIRE(a && a->labels, "label_views_upsample: null pointer");
  ADDK_REQUIRE(lvu_ok(a->nview, a->N, a->OH, a->OW, a->C), "label_views_upsample: unsupported shape (1..%d views, %s)", ADDK_MAX_VIEWS,
               gate_classes_text().c_str());
  for (int v = 0; v < a->nview; ++v) {
    const addk_view& w = a->view[v];
    ADDK_REQUIRE(w.logits, "label_views_upsample: null pointer (view %d)", v);
    ADDK_REQUIRE(w.H > 0 && w.W > 0 && w.n0 >= 0 && w.ld >= a->C, "label_views_upsample: bad size, image offset or stride (view %d)", v);
    ADDK_REQUIRE(w.weight > 0.f && isfinite(w.weight), "label_views_upsample: a weight must be positive and finite (view %d)", v);
  }
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    bool vec = true;                                             // 16-byte pixel loads only where every view allows them
    for (int v = 0; v < a->nview; ++v) vec = vec && px_vec_ok<CC>(a->view[v].logits, a->view[v].ld);
    launch_vec(vec, label_views_kernel<CC, true>, label_views_kernel<CC, false>, lvu_grid(a->N, a->OH, a->OW), st, *a);
  });
  return addk_check_launch("label_views_upsample");
}

extern "C" int addk_label_tiles_upsample_supported(int32_t N, int32_t OH, int32_t OW, int32_t ny, int32_t nx, int32_t C) {
  return ltu_ok(N, OH, OW, ny, nx, C) ? 1 : 0;
}
extern "C" int addk_label_tiles_upsample(const addk_label_tiles_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->labels, "label_tiles_upsample: null pointer");
  ADDK_REQUIRE(ltu_ok(a->N, a->OH, a->OW, a->ny, a->nx, a->C), "label_tiles_upsample: unsupported shape (1..%d windows per axis, %s)",
               ADDK_MAX_TILES_AXIS, head_classes_text().c_str());
  ADDK_REQUIRE(a->h > 0 && a->w > 0 && a->th > 0 && a->tw > 0 && a->ld >= a->C && a->t0 >= 0, "label_tiles_upsample: bad size, first tile or stride");
  ADDK_REQUIRE(ltu_axis_ok(a->y0, a->ny, a->th, a->OH) && ltu_axis_ok(a->x0, a->nx, a->tw, a->OW),
               "label_tiles_upsample: the origins are no window grid of the image (from 0, increasing, no gap, inside it, up to its end)");
  hipStream_t st = (hipStream_t)stream;
  head_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), label_tiles_kernel<CC, true>, label_tiles_kernel<CC, false>, lvu_grid(a->N, a->OH, a->OW), st, *a);
  });
  return addk_check_launch("label_tiles_upsample");
}

extern "C" int addk_label_tile_views_upsample_supported(int32_t nview, int32_t N, int32_t OH, int32_t OW, int32_t C) {
  return ltv_ok(nview, N, OH, OW, C) ? 1 : 0;
}
extern "C" int addk_label_tile_views_upsample(const addk_label_tile_views_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->labels, "label_tile_views_upsample: null pointer");
  ADDK_REQUIRE(ltv_ok(a->nview, a->N, a->OH, a->OW, a->C), "label_tile_views_upsample: unsupported shape (1..%d views, %s)", ADDK_MAX_VIEWS,
               head_classes_text().c_str());
  ADDK_REQUIRE(a->h > 0 && a->w > 0 && a->th > 0 && a->tw > 0 && a->ld >= a->C, "label_tile_views_upsample: bad size or stride");
  for (int v = 0; v < a->nview; ++v) {
    const addk_tile_view& w = a->view[v];
    ADDK_REQUIRE(w.ny >= 1 && w.ny <= ADDK_MAX_TILES_AXIS && w.nx >= 1 && w.nx <= ADDK_MAX_TILES_AXIS,
                 "label_tile_views_upsample: 1..%d windows per axis (view %d)", ADDK_MAX_TILES_AXIS, v);
    ADDK_REQUIRE(w.Hv > 0 && w.Wv > 0 && w.t0 >= 0, "label_tile_views_upsample: bad scaled size or first tile (view %d)", v);
    ADDK_REQUIRE(w.weight > 0.f && isfinite(w.weight), "label_tile_views_upsample: a weight must be positive and finite (view %d)", v);
    ADDK_REQUIRE(ltu_axis_ok(w.y0, w.ny, a->th, w.Hv) && ltu_axis_ok(w.x0, w.nx, a->tw, w.Wv),
                 "label_tile_views_upsample: the origins are no window grid of the scaled image (view %d)", v);
  }
  hipStream_t st = (hipStream_t)stream;
  head_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), label_tile_views_kernel<CC, true>, label_tile_views_kernel<CC, false>,
               ltv_grid(a->N, a->OH, a->OW), st, *a);
  });
  return addk_check_launch("label_tile_views_upsample");
}
