// Input side of sliding-window (tiled) inference (segment.TiledSegmenter): the windows of one chunk, cut from images of any size into
// the tile plan's resident NCHW input.  The reference pads after normalising (dataloaders/custom_transforms.py:289-320, ZeroPad2d), so a
// position outside its image is 0.0f.  The other half of the feature, the head that stitches the windows' logits into the label map,
// is label_tiles_kernel in label_up.hip; gather_tile_views_kernel cuts the windows of scaled, mirrored views (the head: label_tile_views_kernel).
#include "common.h"
#include "up.h"

namespace {

// x [B][Cin][th][tw]: row (b, c, i) of the output is one contiguous run of tw floats.  A workgroup takes 256 consecutive columns of a
// row (coalesced stores along tw) and strides over the rows; the row's slot, plane and source row are wave-uniform, the window
// descriptor comes from the device table.  Slots >= ntiles are zero-filled.
__global__ void __launch_bounds__(256) gather_tiles_kernel(const addk_tile_desc* __restrict__ tiles, int ntiles, int Cin, int th, int tw,
                                                           float* __restrict__ x, long rows) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= tw) return;
  for (long row = blockIdx.y; row < rows; row += gridDim.y) {
    const int i = (int)(row % th);
    const long bc = row / th;
    const int c = (int)(bc % Cin), b = (int)(bc / Cin);
    float v = 0.f;
    if (b < ntiles) {
      const addk_tile_desc d = tiles[b];
      const long sy = (long)d.y0 + i, sx = (long)d.x0 + j;
      if (sy >= 0 && sy < d.H && sx >= 0 && sx < d.W) v = ((const gfloat*)d.image)[((long)c * d.H + sy) * d.W + sx];
    }
    ((gfloat*)x)[row * tw + j] = v;
  }
}

// The same rows over views (multi-scale + flip sliding windows): a window is cut from the image resized to (Hv, Wv) and, for a mirrored view,
// flipped along the width — an image that is never written.  Position (sy, sx) of it is the bilinear sample of the plane at
// (sy, mirror ? Wv-1-sx : sx) of the (H, W) -> (Hv, Wv) resize: src_index and the lerp expression of resize_fwd_nchw_kernel, so the value
// carries the bits addk_resize_fwd writes there.  The row's source rows and weights are wave-uniform, the columns per lane.  A view of the
// image's own size, unmirrored, copies the pixel (gather_tiles_kernel's bytes); a descriptor whose Hv or Wv is not positive leaves zeros.
__global__ void __launch_bounds__(256) gather_tile_views_kernel(const addk_tile_view_desc* __restrict__ tiles, int ntiles, int Cin, int th, int tw,
                                                                float* __restrict__ x, long rows) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= tw) return;
  for (long row = blockIdx.y; row < rows; row += gridDim.y) {
    const int i = (int)(row % th);
    const long bc = row / th;
    const int c = (int)(bc % Cin), b = (int)(bc / Cin);
    float v = 0.f;
    if (b < ntiles) {
      const addk_tile_view_desc d = tiles[b];
      const long sy = (long)d.y0 + i, sx = (long)d.x0 + j;
      if (sy >= 0 && sy < d.Hv && sx >= 0 && sx < d.Wv && d.H > 0 && d.W > 0) {
        const gfloat* plane = (const gfloat*)d.image + (long)c * d.H * d.W;
        const int xv = d.mirror ? d.Wv - 1 - (int)sx : (int)sx;
        if (d.Hv == d.H && d.Wv == d.W && !d.mirror) {
          v = plane[sy * d.W + xv];
        } else {
          const float sh = (float)d.H / (float)d.Hv, sw = (float)d.W / (float)d.Wv;
          int h0, h1, w0, w1; float lh0, lh1, lw0, lw1;
          src_index((int)sy, sh, d.H, h0, h1, lh0, lh1);
          src_index(xv, sw, d.W, w0, w1, lw0, lw1);
          const float v00 = plane[(long)h0 * d.W + w0], v01 = plane[(long)h0 * d.W + w1];
          const float v10 = plane[(long)h1 * d.W + w0], v11 = plane[(long)h1 * d.W + w1];
          v = lh0 * (lw0 * v00 + lw1 * v01) + lh1 * (lw0 * v10 + lw1 * v11);
        }
      }
    }
    ((gfloat*)x)[row * tw + j] = v;
  }
}

// ---- per-window early exits (segment.TiledSegmenter with `threshold`) -------------------------------------------------------------------
// The gate of the windows of one chunk: gate_up_kernel's walk, sweep and last-arriver tail (up.h: scu_walk, exp_sweep_t, up_finish) with
// one image per slot, restricted to the slot's valid extent (vh, vw) — the part of the window that lies on its image; the rest is the
// zero padding of gather_tiles_kernel, which would vote for one class with confidence.  A pixel outside the extent adds nothing, a
// workgroup whose tile lies outside it walks nothing and only takes its ticket; the divisors are the extent's pixel count.  The extents
// are device words (they change with every chunk, the captured launch does not) and are clamped to the window here.
typedef __attribute__((address_space(1))) int gint;
struct GateTilesK : UpSrc {
  const int* ext; const float* thr; const float* inv_temp;
  float* out; float* out_host;
  unsigned* counter; float* part; unsigned* cnt;          // ws: [ticket, 16 bytes][B*nblk floats][B*nblk counts], slot-major
  int nblk_img;
  double logc;                                             // log C
};
__device__ __forceinline__ void tile_extent(const GateTilesK& p, int b, int& vh, int& vw) {
  vh = ((const gint*)p.ext)[2 * b]; vw = ((const gint*)p.ext)[2 * b + 1];
  vh = vh < 1 ? 1 : vh > p.OH ? p.OH : vh;
  vw = vw < 1 ? 1 : vw > p.OW ? p.OW : vw;
}

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) gate_tiles_kernel(const GateTilesK p) {
  int vh, vw;
  tile_extent(p, blockIdx.z, vh, vw);
  const float thr = *(const gfloat*)p.thr;
  const float it = p.inv_temp ? *(const gfloat*)p.inv_temp : 1.f;
  float esum = 0.f; unsigned hit[1] = {0u};
  if ((int)blockIdx.y * (SCU_WAVES * SCU_R) < vh && (int)blockIdx.x * SCU_W < vw) {      // workgroup-uniform
    const int X = blockIdx.x * SCU_W + (threadIdx.x & (SCU_W - 1));
    int Y = (blockIdx.y * SCU_WAVES + threadIdx.x / SCU_W) * SCU_R;                       // the walk calls back for Y, Y + 1, ... of its column
    scu_walk<CC, VEC>(p, [&](long, const float (&z)[CC]) {
      const bool valid = Y < vh && X < vw;
      ++Y;
      if (!valid) return;
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < CC; ++c) mx = fmaxf(mx, z[c]);
      float se, sx;
      exp_sweep_t<CC>(z, mx, it, se, sx);
      esum += logf(se) - sx / se;
      hit[0] += (1.f / se > thr) ? 1u : 0u;
    });
  }
  up_finish<1>(esum, hit, 1, p.counter, p.part, p.cnt, (int)gridDim.z, p.nblk_img, p.out_host != nullptr, [&](int b, double es, auto&& count) {
    int eh, ew;
    tile_extent(p, b, eh, ew);
    const double npix = (double)eh * (double)ew;
    const float ent = (float)(es / (p.logc * npix)), share = (float)((double)count(0) / npix);
    ((gfloat*)p.out)[2 * b] = ent; ((gfloat*)p.out)[2 * b + 1] = share;
    if (p.out_host) { p.out_host[2 * b] = ent; p.out_host[2 * b + 1] = share; }
  });
}

// Rows of the plan's logits -> tiles of the store: workgroup column i of the grid copies entry i, its threads stride over the tile's
// pixels x channel quads (VEC: both strides are multiples of four floats and both bases 16-byte aligned) or over its single floats.  The
// store's padding channels are written as zero: the label heads' 16-byte loader reads them.
struct ScatterTilesK {
  const float* src; float* store; const int* src_row; const int* dst_tile;
  int lds, ld, B, T, C; long px;                           // px = h*w
};
template <bool VEC>
__global__ void __launch_bounds__(256) scatter_tile_logits_kernel(const ScatterTilesK p) {
  const int i = blockIdx.y;
  const int r = p.src_row ? ((const gint*)p.src_row)[i] : i, t = ((const gint*)p.dst_tile)[i];
  if (r < 0 || r >= p.B || t < 0 || t >= p.T) return;      // device words: checked where they are read
  const float* s = p.src + (long)r * p.px * p.lds;
  float* d = p.store + (long)t * p.px * p.ld;
  const long step = (long)gridDim.x * 256;
  if constexpr (VEC) {
    const int q = p.ld / 4;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < p.px * q; e += step) {
      const long pix = e / q;
      const int c = (int)(e - pix * q) * 4;
      st4(d + pix * p.ld + c, ld4g(s + pix * p.lds + c, p.C - c, true));
    }
  } else {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < p.px * p.ld; e += step) {
      const long pix = e / p.ld;
      const int c = (int)(e - pix * p.ld);
      ((gfloat*)d)[e] = c < p.C ? ((const gfloat*)s)[pix * p.lds + c] : 0.f;
    }
  }
}

}  // namespace

extern "C" int addk_gate_tiles_upsample_supported(int32_t B, int32_t h, int32_t w, int32_t th, int32_t tw, int32_t C) {
  return scu_head_ok(B, h, w, th, tw, C) ? 1 : 0;
}
extern "C" int64_t addk_gate_tiles_upsample_ws_bytes(int32_t B, int32_t th, int32_t tw) {
  if (B <= 0 || th <= 0 || tw <= 0) return 0;
  return up_ws_bytes(B, th, tw, 1);
}
extern "C" int addk_gate_tiles_upsample(const addk_gate_tiles_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->ext && a->max_thr && a->out && a->ws, "gate_tiles_upsample: null pointer");
  ADDK_REQUIRE(scu_head_ok(a->B, a->h, a->w, a->th, a->tw, a->C), "gate_tiles_upsample: unsupported shape (%s)", head_classes_text().c_str());
  ADDK_REQUIRE(a->nb >= 0 && a->nb <= a->B, "gate_tiles_upsample: %d windows for %d slots", a->nb, a->B);
  ADDK_REQUIRE(a->ld >= a->C, "gate_tiles_upsample: short stride");
  if (a->nb == 0) return ADDK_OK;
  GateTilesK k;
  static_cast<UpSrc&>(k) = UpSrc{a->logits, a->ld, a->nb, a->h, a->w, a->th, a->tw};
  k.ext = a->ext; k.thr = a->max_thr; k.inv_temp = a->inv_temp; k.out = a->out; k.out_host = a->out_host;
  const dim3 grid = scu_grid(a->nb, a->th, a->tw);
  k.nblk_img = (int)(grid.x * grid.y);
  k.counter = (unsigned*)a->ws;
  k.part = (float*)((char*)a->ws + 16);
  k.cnt = (unsigned*)(k.part + (long)a->B * k.nblk_img);   // the layout is the plan's (B slots), whatever nb
  k.logc = log((double)a->C);
  head_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), gate_tiles_kernel<CC, true>, gate_tiles_kernel<CC, false>, grid, (hipStream_t)stream, k);
  });
  return addk_check_launch("gate_tiles_upsample");
}

extern "C" int addk_scatter_tile_logits(const addk_scatter_tile_logits_args* a, void* stream) {
  ADDK_REQUIRE(a && a->src && a->store && a->dst_tile, "scatter_tile_logits: null pointer");
  ADDK_REQUIRE(a->B > 0 && a->T > 0 && a->h > 0 && a->w > 0 && a->C > 0, "scatter_tile_logits: non-positive size");
  ADDK_REQUIRE(a->n >= 0 && a->n <= a->B, "scatter_tile_logits: %d rows of %d", a->n, a->B);
  ADDK_REQUIRE(a->lds >= a->C && a->ld >= a->C, "scatter_tile_logits: short stride");
  if (a->n == 0) return ADDK_OK;
  ScatterTilesK k{a->src, a->store, a->src_row, a->dst_tile, a->lds, a->ld, a->B, a->T, a->C, (long)a->h * a->w};
  const bool vec = a->lds % 4 == 0 && a->ld % 4 == 0 && aligned16(a->src) && aligned16(a->store);
  const long units = vec ? k.px * (a->ld / 4) : k.px * a->ld;
  const dim3 grid((unsigned)(units < 64L * 256 ? cdiv(units, 256) : 64), (unsigned)a->n);
  hipLaunchKernelGGL(vec ? scatter_tile_logits_kernel<true> : scatter_tile_logits_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, k);
  return addk_check_launch("scatter_tile_logits");
}

extern "C" int addk_gather_tiles(const addk_tile_desc* tiles_dev, int32_t ntiles, int32_t Cin, int32_t th, int32_t tw, float* x, int32_t B,
                                 void* stream) {
  ADDK_REQUIRE(x && (tiles_dev || ntiles == 0), "gather_tiles: null pointer");
  ADDK_REQUIRE(B > 0 && Cin > 0 && th > 0 && tw > 0, "gather_tiles: non-positive size");
  ADDK_REQUIRE(ntiles >= 0 && ntiles <= B, "gather_tiles: %d windows for %d slots", ntiles, B);
  const long rows = (long)B * Cin * th;
  const dim3 grid(cdiv(tw, 256), (unsigned)(rows < 2048 ? rows : 2048));     // a few thousand workgroups, the rest by stride
  hipLaunchKernelGGL(gather_tiles_kernel, grid, dim3(256), 0, (hipStream_t)stream, tiles_dev, ntiles, Cin, th, tw, x, rows);
  return addk_check_launch("gather_tiles");
}

extern "C" int addk_gather_tile_views(const addk_tile_view_desc* tiles_dev, int32_t ntiles, int32_t Cin, int32_t th, int32_t tw, float* x,
                                      int32_t B, void* stream) {
  ADDK_REQUIRE(x && (tiles_dev || ntiles == 0), "gather_tile_views: null pointer");
  ADDK_REQUIRE(B > 0 && Cin > 0 && th > 0 && tw > 0, "gather_tile_views: non-positive size");
  ADDK_REQUIRE(ntiles >= 0 && ntiles <= B, "gather_tile_views: %d windows for %d slots", ntiles, B);
  const long rows = (long)B * Cin * th;
  const dim3 grid(cdiv(tw, 256), (unsigned)(rows < 2048 ? rows : 2048));
  hipLaunchKernelGGL(gather_tile_views_kernel, grid, dim3(256), 0, (hipStream_t)stream, tiles_dev, ntiles, Cin, th, tw, x, rows);
  return addk_check_launch("gather_tile_views");
}
