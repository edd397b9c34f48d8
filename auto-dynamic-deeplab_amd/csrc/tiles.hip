// Input side of sliding-window (tiled) inference (segment.TiledSegmenter): the windows of one chunk, cut from images of any size into
// the tile plan's resident NCHW input.  The reference pads after normalising (dataloaders/custom_transforms.py:289-320, ZeroPad2d), so a
// position outside its image is 0.0f.  The other half of the feature, the head that stitches the windows' logits into the label map,
// is label_tiles_kernel in label_up.hip; gather_tile_views_kernel cuts the windows of scaled, mirrored views (the head: label_tile_views_kernel).
#include "common.h"

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

}  // namespace

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
