// Boundary-band ("trimap") metric: distance to the nearest ground-truth class boundary and the confusion matrix per distance ring
// (include/addk.h, "Boundary-band confusion").  Integer-only: two calls give equal bits.
//   addk_boundary_dist   : trimap_row_kernel (edge flags as 64-bit ballot words -> row distance h, bytes) + trimap_col_kernel
//                          (LDS tile of h with a halo of `radius` rows -> dist)
//   addk_confusion_banded: confusion_banded_kernel (grid-stride, per-workgroup LDS histogram, 64-bit integer atomics on the flush)
#include "common.h"

namespace {

constexpr int ROW_TR = 8;        // rows of a row-pass tile: each target row is read (ROW_TR + 2) / ROW_TR times
constexpr int ROW_WB = 14;       // 64-column words of a row-pass tile at most
constexpr int ROW_WC = ROW_WB + 2;   // ... plus one halo word on either side (the search radius is at most 64 columns)
constexpr int COL_TH = 64;       // rows of a column-pass tile (64 columns wide)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
constexpr int COL_LS = 20;       // LDS row stride of the h tile in 32-bit words (16 used): the four row groups of a wave fall on distinct banks

// class of a target value, or -1: 0 <= t < C as 64-bit values; -1 outside the image.  The load itself is unconditional, from the nearest
// pixel inside the image, so that the loads of a wave's word column are all in flight together instead of one per branch.
__device__ __forceinline__ int tm_code(const int64_t* img, int OH, int OW, int C, int y, int x) {
  const bool in = y >= 0 && y < OH && x >= 0 && x < OW;
  const int yc = min(max(y, 0), OH - 1), xc = min(max(x, 0), OW - 1);
  const int64_t v = img[(long)yc * OW + xc];
  return (in && v >= 0 && v < (int64_t)C) ? (int)v : -1;
}

// One workgroup: rows [y0, y0 + ROW_TR) x words [w0, wend) of image n.  A wave owns a word column: it loads the ROW_TR + 2 rows of class
// codes once (up / cur / down of every row are three of them); left / right come from the neighbour lanes, the two end lanes load
// theirs.  The flags leave the wave as one ballot word; h follows from the word and its two neighbours by count-trailing / count-leading
// zeros.
__global__ __launch_bounds__(256) void trimap_row_kernel(const int64_t* __restrict__ target, int OH, int OW, int C, int R, int nwords, int WB,
                                                         int nseg, int nband, uint8_t* __restrict__ h, int vec) {
  __shared__ unsigned long long words[ROW_TR][ROW_WC];
  int b = (int)blockIdx.x;
  const int seg = b % nseg; b /= nseg;
  const int band = b % nband;
  const int n = b / nband;
  const int y0 = band * ROW_TR, w0 = seg * WB;
  const int wend = min(w0 + WB, nwords);
  const int nwc = wend - w0 + 2;                       // word column j stands for word w0 - 1 + j
  const int64_t* img = target + (long)n * OH * OW;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  for (int j = wave; j < nwc; j += 4) {
    const int w = w0 - 1 + j;
    if (w < 0 || w >= nwords) {
      if (lane < ROW_TR) words[lane][j] = 0ull;
      continue;
    }
    const int x = w * 64 + lane;
    // every load of the word column is issued before the first flag is formed: ROW_TR + 2 rows, and the column beside the word for the
    // two end lanes
    int code[ROW_TR + 2], side[ROW_TR];
#pragma unroll
    for (int r = 0; r < ROW_TR + 2; ++r) code[r] = tm_code(img, OH, OW, C, y0 - 1 + r, x);
    const int xs = lane == 0 ? x - 1 : lane == 63 ? x + 1 : -1;
#pragma unroll
    for (int r = 0; r < ROW_TR; ++r) side[r] = tm_code(img, OH, OW, C, y0 + r, xs);
#pragma unroll
    for (int r = 0; r < ROW_TR; ++r) {
      const int up = code[r], cur = code[r + 1], down = code[r + 2];      // rows past OH read as invalid: their words are 0
      int left = __shfl_up(cur, 1), right = __shfl_down(cur, 1);
      if (lane == 0) left = side[r];
      if (lane == 63) right = side[r];
      const bool e = cur >= 0 && ((up >= 0 && up != cur) || (down >= 0 && down != cur) || (left >= 0 && left != cur) || (right >= 0 && right != cur));
      const unsigned long long m = __ballot(e);
      if (lane == 0) words[r][j] = m;
    }
  }
  __syncthreads();
  const int qpr = (wend - w0) * 16;                    // 4-pixel groups per tile row
  for (int i = (int)threadIdx.x; i < ROW_TR * qpr; i += 256) {
    const int r = i / qpr, q = i - r * qpr;
    const int y = y0 + r, x = w0 * 64 + q * 4;
    if (y >= OH) break;
    if (x >= OW) continue;
    const int j = (q >> 4) + 1;
    const unsigned long long wm = words[r][j], wl = words[r][j - 1], wr = words[r][j + 1];
    unsigned pack = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int bit = ((q & 15) << 2) + e;
      const unsigned long long mr = wm >> bit, ml = wm << (63 - bit);
      const int dr = mr ? __builtin_ctzll(mr) : wr ? 64 - bit + __builtin_ctzll(wr) : 1000;
      const int dl = ml ? __builtin_clzll(ml) : wl ? bit + 1 + __builtin_clzll(wl) : 1000;
      const int d = min(dl, dr);
      pack |= (unsigned)(d > R ? ADDK_TRIMAP_FAR : d) << (8 * e);
    }
    const long o = ((long)n * OH + y) * OW + x;
    if (vec) {
      *reinterpret_cast<unsigned*>(h + o) = pack;      // OW % 4 == 0: the group is inside the row and 4-byte aligned
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < OW) h[o + e] = (uint8_t)(pack >> (8 * e));
    }
  }
}

// One workgroup: 64 columns x COL_TH rows of image n.  The h tile with R halo rows above and below (rows outside THIS image and columns
// past OW read as "no edge") sits in LDS, four pixels to a word.  A thread owns 4 columns x 4 rows and walks the 4 + 2R source rows once.
// A source row further than R away can only propose dy^2 > R^2, which is FAR anyway, so the window needs no per-row bounds.
__global__ __launch_bounds__(256) void trimap_col_kernel(const uint8_t* __restrict__ h, int OH, int OW, int R, int tilesX, int tilesY,
                                                         uint8_t* __restrict__ dist, int vec) {
  extern __shared__ unsigned tm_tile[];
  int b = (int)blockIdx.x;
  const int tx = b % tilesX; b /= tilesX;
  const int ty = b % tilesY;
  const int n = b / tilesY;
  const int x0 = tx * 64, y0 = ty * COL_TH;
  const int rows = COL_TH + 2 * R;
  const uint8_t* hi = h + (long)n * OH * OW;
  if (vec) {
    // unconditional 4-byte loads from the nearest group inside the image (OW % 4 == 0, so OW - 4 is one), four rows in flight per thread
    const int c = (int)threadIdx.x & 15, x = x0 + 4 * c;
    const int xc = min(x, OW - 4);
    for (int s0 = (int)threadIdx.x >> 4; s0 < rows; s0 += 64) {
      unsigned v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int y = y0 - R + s0 + 16 * u;
        v[u] = *reinterpret_cast<const unsigned*>(hi + (long)min(max(y, 0), OH - 1) * OW + xc);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int s = s0 + 16 * u, y = y0 - R + s;
        if (s < rows) tm_tile[s * COL_LS + c] = (y >= 0 && y < OH && x < OW) ? v[u] : 0xFFFFFFFFu;
      }
    }
  } else {
    for (int i = (int)threadIdx.x; i < rows * 16; i += 256) {
      const int s = i >> 4, c = i & 15;
      const int y = y0 - R + s, x = x0 + 4 * c;
      unsigned v = 0xFFFFFFFFu;
      if (y >= 0 && y < OH && x < OW) {
        const long o = (long)y * OW + x;
        v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) v |= (unsigned)(x + e < OW ? hi[o + e] : (uint8_t)ADDK_TRIMAP_FAR) << (8 * e);
      }
      tm_tile[s * COL_LS + c] = v;
    }
  }
  __syncthreads();
  const int c = (int)threadIdx.x & 15, ly0 = ((int)threadIdx.x >> 4) * 4;
  // squared distances as 16-bit pairs (packed add / min): h is at most 64 or FAR, FAR & 0x7F = 127 still squares past every R^2, and
  // 127^2 + (R + 5)^2 fits 16 bits
  u16x2 best[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) best[j][0] = best[j][1] = u16x2{0xFFFF, 0xFFFF};
  const int send = ly0 + 3 + 2 * R;
  for (int s4 = ly0; s4 <= send; s4 += 4) {
    // four LDS words in flight; the window is 4 + 2R rows, so the last group of an odd R repeats row `send` under a larger dy: such a
    // candidate is never below the one the row already gave
    unsigned wd4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wd4[u] = tm_tile[min(s4 + u, send) * COL_LS + c];
    const int base = s4 - R - ly0;                     // dy of source row s4 + u for output row ly0 + j is base + (u - j)
    const int b2 = base * base, bx = 2 * base;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (wd4[u] == 0xFFFFFFFFu) continue;             // no edge within R on this row for any of the four columns
      const unsigned m = wd4[u] & 0x7F7F7F7Fu;
      const unsigned h0 = m & 255u, h1 = (m >> 8) & 255u, h2 = (m >> 16) & 255u, h3 = m >> 24;
      const u16x2 q01 = __builtin_bit_cast(u16x2, h0 * h0 | (h1 * h1) << 16), q23 = __builtin_bit_cast(u16x2, h2 * h2 | (h3 * h3) << 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = u - j;
        const unsigned dy2 = (unsigned)(b2 + k * bx + k * k);
        const u16x2 dd = __builtin_bit_cast(u16x2, dy2 | dy2 << 16);
        best[j][0] = __builtin_elementwise_min(best[j][0], (u16x2)(q01 + dd));
        best[j][1] = __builtin_elementwise_min(best[j][1], (u16x2)(q23 + dd));
      }
    }
  }
  const unsigned R2 = (unsigned)(R * R);
  const int x = x0 + 4 * c;
  if (x >= OW) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = y0 + ly0 + j;
    if (y >= OH) break;
    unsigned pack = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned d2 = best[j][e >> 1][e & 1];
      unsigned k = ADDK_TRIMAP_FAR;
      if (d2 <= R2) {                                  // k = ceil(sqrt(d2)), exactly: the float root, then the integer correction
        k = (unsigned)__builtin_sqrtf((float)d2);
        if (k * k < d2) ++k;
        else if (k > 0 && (k - 1) * (k - 1) >= d2) --k;
      }
      pack |= k << (8 * e);
    }
    const long o = ((long)n * OH + y) * OW + x;
    if (vec) {
      *reinterpret_cast<unsigned*>(dist + o) = pack;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < OW) dist[o + e] = (uint8_t)(pack >> (8 * e));
    }
  }
}

struct BandWidths { int32_t nw; int32_t width[ADDK_TRIMAP_MAX_WIDTHS]; };

// Segment `seg` is the whole batch (stride 0) or one image; its workgroups walk absolute, 4-aligned pixel groups.  The dist word is read
// first: a group with no pixel inside the widest band costs 4 bytes, not 40.
__global__ __launch_bounds__(256) void confusion_banded_kernel(const int64_t* __restrict__ target, const uint8_t* __restrict__ pred,
                                                               const uint8_t* __restrict__ dist, long segpx, int C, BandWidths bw,
                                                               unsigned long long* __restrict__ cm, long stride, int bps, int vec) {
  extern __shared__ unsigned tm_hist[];                // [nw][C][C] counts, then the 256-entry ring table
  const int CC = C * C, ne = bw.nw * CC;
  uint8_t* ring = reinterpret_cast<uint8_t*>(tm_hist + ne);
  for (int i = (int)threadIdx.x; i < ne; i += 256) tm_hist[i] = 0u;
  {
    const int d = (int)threadIdx.x;                    // ring of distance d: the number of widths below d (they ascend)
    int j = 0;
#pragma unroll
    for (int q = 0; q < ADDK_TRIMAP_MAX_WIDTHS; ++q) j += (q < bw.nw && d > bw.width[q]) ? 1 : 0;
    ring[d] = (uint8_t)(j < bw.nw ? j : 255);
  }
  __syncthreads();
  const int seg = (int)blockIdx.x / bps, bi = (int)blockIdx.x % bps;
  const long start = (long)seg * segpx, end = start + segpx;
  const long g1 = (end + 3) >> 2;
  for (long g = (start >> 2) + (long)bi * 256 + (long)threadIdx.x; g < g1; g += (long)bps * 256) {
    const long p = g << 2;
    if (vec && p >= start && p + 4 <= end) {
      const unsigned dw = *reinterpret_cast<const unsigned*>(dist + p);
      unsigned rg[4];
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) { rg[e] = ring[(dw >> (8 * e)) & 255u]; any |= rg[e] != 255u; }
      if (!any) continue;
      const unsigned pw = *reinterpret_cast<const unsigned*>(pred + p);
      const longlong2 t01 = *reinterpret_cast<const longlong2*>(target + p), t23 = *reinterpret_cast<const longlong2*>(target + p + 2);
      const long long t[4] = {t01.x, t01.y, t23.x, t23.y};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned pr = (pw >> (8 * e)) & 255u;
        if (rg[e] != 255u && t[e] >= 0 && t[e] < (long long)C && pr < (unsigned)C)
          atomicAdd(&tm_hist[rg[e] * CC + (int)t[e] * C + (int)pr], 1u);
      }
    } else {
      for (int e = 0; e < 4; ++e) {
        const long q = p + e;
        if (q < start || q >= end) continue;
        const unsigned r = ring[dist[q]];
        if (r == 255u) continue;
        const long long t = target[q];
        const unsigned pr = pred[q];
        if (t >= 0 && t < (long long)C && pr < (unsigned)C) atomicAdd(&tm_hist[r * CC + (int)t * C + (int)pr], 1u);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = cm + (long)seg * stride;
  for (int i = (int)threadIdx.x; i < ne; i += 256) {
    const unsigned v = tm_hist[i];
    if (v) atomicAdd(&out[i], (unsigned long long)v);
  }
}

bool tm_sizes_ok(int32_t N, int32_t OH, int32_t OW, int32_t C) {
  return N > 0 && OH > 0 && OW > 0 && C >= 1 && C <= 32 && (int64_t)N * OH * OW < ((int64_t)1 << 31);
}
bool tm_aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

extern "C" int addk_boundary_dist_supported(int32_t N, int32_t OH, int32_t OW, int32_t C, int32_t radius) {
  return tm_sizes_ok(N, OH, OW, C) && radius >= 1 && radius <= ADDK_TRIMAP_MAX_RADIUS ? 1 : 0;
}

extern "C" int64_t addk_boundary_dist_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  return ((int64_t)N * OH * OW + 15) / 16 * 16;        // h, one byte per pixel
}

extern "C" int addk_boundary_dist(const addk_boundary_dist_args* a, void* stream) {
  ADDK_REQUIRE(a && a->target && a->dist && a->ws, "boundary_dist: null pointer");
  ADDK_REQUIRE(addk_boundary_dist_supported(a->N, a->OH, a->OW, a->C, a->radius) == 1,
               "boundary_dist: unsupported [%d,%d,%d], %d classes, radius %d", a->N, a->OH, a->OW, a->C, a->radius);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* h = static_cast<uint8_t*>(a->ws);
  const int vec = (a->OW % 4 == 0 && tm_aligned(h, 4) && tm_aligned(a->dist, 4)) ? 1 : 0;
  const int nwords = cdiv(a->OW, 64), nseg = cdiv(nwords, ROW_WB), WB = cdiv(nwords, nseg), nband = cdiv(a->OH, ROW_TR);
  const long rb = (long)a->N * nband * nseg;
  const int tilesX = cdiv(a->OW, 64), tilesY = cdiv(a->OH, COL_TH);
  const long cb = (long)a->N * tilesY * tilesX;
  ADDK_REQUIRE(rb < ((long)1 << 31) && cb < ((long)1 << 31), "boundary_dist: grid too large");
  hipLaunchKernelGGL(trimap_row_kernel, dim3((unsigned)rb), dim3(256), 0, st, a->target, a->OH, a->OW, a->C, a->radius, nwords, WB, nseg, nband, h, vec);
  int rc = addk_check_launch("trimap_row");
  if (rc) return rc;
  const size_t lds = (size_t)(COL_TH + 2 * a->radius) * COL_LS * sizeof(unsigned);
  hipLaunchKernelGGL(trimap_col_kernel, dim3((unsigned)cb), dim3(256), lds, st, h, a->OH, a->OW, a->radius, tilesX, tilesY, a->dist, vec);
  return addk_check_launch("trimap_col");
}

extern "C" int addk_confusion_banded_supported(int32_t N, int32_t OH, int32_t OW, int32_t C, int32_t nw) {
  return tm_sizes_ok(N, OH, OW, C) && nw >= 1 && nw <= ADDK_TRIMAP_MAX_WIDTHS ? 1 : 0;
}

extern "C" int addk_confusion_banded(const addk_confusion_banded_args* a, void* stream) {
  ADDK_REQUIRE(a && a->target && a->pred && a->dist && a->cm, "confusion_banded: null pointer");
  ADDK_REQUIRE(addk_confusion_banded_supported(a->N, a->OH, a->OW, a->C, a->nw) == 1,
               "confusion_banded: unsupported [%d,%d,%d], %d classes, %d widths", a->N, a->OH, a->OW, a->C, a->nw);
  BandWidths bw{};
  bw.nw = a->nw;
  for (int j = 0; j < a->nw; ++j) {
    ADDK_REQUIRE(a->width[j] >= 0 && a->width[j] <= 254 && (j == 0 || a->width[j] > a->width[j - 1]),
                 "confusion_banded: widths must ascend strictly inside [0, 254]");
    bw.width[j] = a->width[j];
  }
  const int64_t ne = (int64_t)a->nw * a->C * a->C;
  ADDK_REQUIRE(a->image_stride == 0 || a->image_stride >= ne, "confusion_banded: image_stride %lld below nw*C*C = %lld",
               (long long)a->image_stride, (long long)ne);
  const int nsegs = a->image_stride ? a->N : 1;
  const long segpx = a->image_stride ? (long)a->OH * a->OW : (long)a->N * a->OH * a->OW;
  // about two workgroups per CU in all, none with fewer than 8 pixel groups per thread: every workgroup flushes up to nw*C*C atomics
  long bps = (segpx / 4 + 256 * 8 - 1) / (256 * 8);
  const long cap = nsegs >= 512 ? 1 : 512 / nsegs;
  if (bps > cap) bps = cap;
  if (bps < 1) bps = 1;
  const int vec = (tm_aligned(a->target, 16) && tm_aligned(a->pred, 4) && tm_aligned(a->dist, 4)) ? 1 : 0;
  const size_t lds = (size_t)ne * sizeof(unsigned) + 256;
  hipLaunchKernelGGL(confusion_banded_kernel, dim3((unsigned)(bps * nsegs)), dim3(256), lds, (hipStream_t)stream, a->target, a->pred, a->dist,
                     segpx, a->C, bw, reinterpret_cast<unsigned long long*>(a->cm), (long)a->image_stride, (int)bps, vec);
  return addk_check_launch("confusion_banded");
}
