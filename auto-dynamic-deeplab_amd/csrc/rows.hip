// Row gather / scatter over several buffers in one launch (addk_gather_rows): the batch compaction of dynamic.BatchedGate.
// A bandwidth kernel.  The unit of work is up to 16 KiB of one row of one item; the units of all items form ONE sequence
// (item-major, then row, then position in the row) that the workgroups walk with a grid stride, each keeping a running prefix
// over the item table — a level-3 tensor and the low-level feature differ by 100x in row size and still share the grid evenly.
#include <vector>

#include "common.h"

namespace {

constexpr int ROWS_THREADS = 256;
constexpr long ROWS_UNIT = 16384;        // bytes; a multiple of 16: every unit but a row's first starts on the row's access width
constexpr int ROWS_MAX_ITEMS = 65536;
constexpr long ROWS_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups: the rest is grid stride

struct RowsK {
  const addk_rows_item* items; int nitems;
  const int32_t* src_row; const int32_t* dst_row; int nrows;
  long total;                             // units of all items
};

__device__ __forceinline__ long rows_units(long row_bytes) { return (row_bytes + ROWS_UNIT - 1) / ROWS_UNIT; }

__device__ __forceinline__ void copy_bytes(const uint8_t* s, uint8_t* d, long lo, long hi) {
  for (long i = lo + threadIdx.x; i < hi; i += ROWS_THREADS) d[i] = s[i];
}

// bytes [lo, hi) of a row in accesses of type V: s + lo and d + lo are aligned to V and hi - lo is a multiple of its size.
// Four loads are in flight per thread before the first store: one 16 KiB unit is exactly one round of 16-byte accesses.
template <typename V>
__device__ __forceinline__ void copy_wide(const uint8_t* s, uint8_t* d, long lo, long hi) {
  const V* sv = (const V*)(s + lo);
  V* dv = (V*)(d + lo);
  const long n = (hi - lo) / (long)sizeof(V);
  long i = threadIdx.x;
  for (; i + 3 * ROWS_THREADS < n; i += 4 * ROWS_THREADS) {
    const V a = sv[i], b = sv[i + ROWS_THREADS], c = sv[i + 2 * ROWS_THREADS], e = sv[i + 3 * ROWS_THREADS];
    dv[i] = a; dv[i + ROWS_THREADS] = b; dv[i + 2 * ROWS_THREADS] = c; dv[i + 3 * ROWS_THREADS] = e;
  }
  for (; i < n; i += ROWS_THREADS) dv[i] = sv[i];
}

__global__ void __launch_bounds__(ROWS_THREADS) gather_rows_kernel(const RowsK p) {
  int it = 0;
  long base = 0;                          // units before item `it`
  long rb = p.items[0].row_bytes, upr = rows_units(rb), cnt = upr * p.nrows;
  for (long u = blockIdx.x; u < p.total; u += gridDim.x) {
    while (u >= base + cnt) {             // u only grows: the prefix is walked once per workgroup
      base += cnt;
      if (++it >= p.nitems) return;       // (total is the sum of the counts: not reached)
      rb = p.items[it].row_bytes; upr = rows_units(rb); cnt = upr * p.nrows;
    }
    const long v = u - base;
    const int r = (int)(v / upr);
    const long c = v - (long)r * upr;
    const long sr = p.src_row ? p.src_row[r] : r, dr = p.dst_row ? p.dst_row[r] : r;
    const uint8_t* s = (const uint8_t*)p.items[it].src + sr * rb;
    uint8_t* d = (uint8_t*)p.items[it].dst + dr * rb;
    // access width of this row: the widest at which source and destination share their misalignment
    const unsigned long delta = (unsigned long)(uintptr_t)s - (unsigned long)(uintptr_t)d;
    const long w = (delta & 15) == 0 ? 16 : (delta & 3) == 0 ? 4 : 1;
    long head = (w - (long)((uintptr_t)d & (unsigned long)(w - 1))) & (w - 1);      // bytes before the first aligned access
    if (head > rb) head = rb;
    // unit c is [lo, hi): every boundary inside the row sits at head + k * ROWS_UNIT, on the access width
    long lo = c * ROWS_UNIT + head, hi = (c + 1) * ROWS_UNIT + head;
    if (c == 0) lo = 0;
    if (lo > rb) lo = rb;
    if (hi > rb || c == upr - 1) hi = rb;
    long blo = c == 0 ? head : lo;        // the aligned body [blo, bhi); single bytes before (first unit) and after (last unit)
    if (blo > hi) blo = hi;
    const long bhi = blo + (hi - blo) / w * w;
    if (c == 0) copy_bytes(s, d, 0, blo);
    if (w == 16) copy_wide<uint4>(s, d, blo, bhi);
    else if (w == 4) copy_wide<uint32_t>(s, d, blo, bhi);
    copy_bytes(s, d, w == 1 ? blo : bhi, hi);
  }
}

}  // namespace

extern "C" int addk_gather_rows(const addk_gather_rows_args* a, void* stream) {
  ADDK_REQUIRE(a && a->items, "gather_rows: null arguments");
  ADDK_REQUIRE(a->nitems >= 1 && a->nitems <= ROWS_MAX_ITEMS && a->nrows >= 1, "gather_rows: nitems %d (1..%d), nrows %d (>= 1)",
               a->nitems, ROWS_MAX_ITEMS, a->nrows);
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  ADDK_REQUIRE(cap == hipStreamCaptureStatusNone, "gather_rows: the launch reads its item table back and cannot be captured");
  // the table is device memory: the sizes that decide the grid, and what must be refused, are only known after reading it back
  std::vector<addk_rows_item> items((size_t)a->nitems);
  hipError_t e = hipMemcpyAsync(items.data(), a->items, items.size() * sizeof(addk_rows_item), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    addk_set_error("gather_rows: reading the item table: %s", hipGetErrorString(e));
    return ADDK_ERR_HIP;
  }
  long total = 0;
  for (int i = 0; i < a->nitems; ++i) {
    ADDK_REQUIRE(items[i].src && items[i].dst && items[i].row_bytes >= 1, "gather_rows: item %d: null pointer or row_bytes %ld < 1", i,
                 (long)items[i].row_bytes);
    const long units = items[i].row_bytes / ROWS_UNIT + (items[i].row_bytes % ROWS_UNIT != 0);
    if (units <= 0x7fffffffL) total += (long)a->nrows * units;          // (neither the product nor the sum can wrap)
    ADDK_REQUIRE(units <= 0x7fffffffL && total <= 0x7fffffffL, "gather_rows: more than 2^31 - 1 units of %ld bytes", ROWS_UNIT);
  }
  RowsK k{a->items, a->nitems, a->src_row, a->dst_row, a->nrows, total};
  const long blocks = total < ROWS_MAX_BLOCKS ? total : ROWS_MAX_BLOCKS;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(ROWS_THREADS), 0, st, k);
  return addk_check_launch("gather_rows");
}
