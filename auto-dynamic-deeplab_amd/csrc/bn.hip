// BatchNorm statistics kernels (F.batch_norm training mode at every BatchNorm(...) call site of
// the path: operations.py:25,39,54,58,93; ADD.py:156,162,168,258; aspp_train.py:27-32; decoder.py:15,19).
// They only touch [rows][C][2] partial slabs written by the producing kernels and C-length vectors.
// Slabs are fp64 end to end (squares, partial sums, cross-block sums): the E[x^2]-E[x]^2 form must survive
// the 2-sample BatchNorm of the ASPP image-pool branch at bs=2 as ATen's fp64-accumulating CPU path does.
//
// THE SUMMATION ORDER of a slab (the contract that makes a hipGraph replay equal the eager run; tests/test_gpu_bn_slab_order.py pins it
// bit for bit).  Per slab [rows][C][2] and channel, for each of the two components:
//  1. walk: row group rg (0 .. 63) adds, to a running value that starts at +0.0, one batch after the other; batch i is the eight rows
//     rg + 512 i + 64 k (k = 0 .. 7, a row past the end counts as +0.0) summed as ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)); batches run
//     while 512 i < rows (a batch past the end for all 64 row groups would add +0.0 to a value that is never -0.0);
//  2. tree: for s = 32, 16, 8, 4, 2, 1 row group rg < s becomes (rg) + (rg + s); the slab's sum is row group 0's value;
//  3. bn_bwd adds the slabs' sums one after the other, in list order, to a value that starts at +0.0.
#include "common.h"

namespace {

// block = BN_CH channels x BN_RG row groups.  16 x 64 (1024 threads) put a 40-channel slab on 3 CUs, and a 9-slab bn_bwd list pulled
// 3.9 MB through them in nine dependent round trips: the kernels ran at the per-CU rate of the memory system on a handful of CUs.
// 4 x 64 (256 threads) spreads the same sums over 4x the CUs; a per-channel sum does not depend on BN_CH.
// -DADDK_BN_CH=2 / 8 build the widths 4 was timed against (scripts/bn_time.py, profiles/bn_slab_kernel_time.txt)
#ifndef ADDK_BN_CH
#define ADDK_BN_CH 4
#endif
constexpr int BN_CH = ADDK_BN_CH, BN_RG = 64, BN_T = BN_CH * BN_RG, BN_B = 8 * BN_RG;   // BN_B: rows one batch of a workgroup covers
constexpr int BN_KC = 40 / BN_CH;         // slabs of a bn_bwd list summed per pass: a 40 KB panel
static_assert(BN_CH == 2 || BN_CH == 4 || BN_CH == 8, "the tail works on whole 16-lane rows of whole waves, or on half of one wave");
typedef double2 (*bn_panel)[BN_RG][BN_CH];

struct SlabRef { const double* p; int rows; };
struct SlabBatch { double2 v[8]; int r0, rows; };

// rows r0 + k BN_RG (k < 8) of channel c; a row past the end reads row 0 (no branch around a load) and is masked when it is added
__device__ __forceinline__ void batch_load(SlabBatch& t, const SlabRef& s, int C, int c, int r0) {
  t.r0 = r0; t.rows = s.rows;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int rr = r0 + k * BN_RG;
    t.v[k] = *reinterpret_cast<const double2*>(s.p + ((long)(rr < s.rows ? rr : 0) * C + c) * 2);
  }
}
__device__ __forceinline__ void batch_add(const SlabBatch& t, double& a, double& b) {
  double2 v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool ok = t.r0 + k * BN_RG < t.rows;
    v[k].x = ok ? t.v[k].x : 0.0; v[k].y = ok ? t.v[k].y : 0.0;
  }
  a += ((v[0].x + v[1].x) + (v[2].x + v[3].x)) + ((v[4].x + v[5].x) + (v[6].x + v[7].x));
  b += ((v[0].y + v[1].y) + (v[2].y + v[3].y)) + ((v[4].y + v[5].y) + (v[6].y + v[7].y));
}

// v + (v of the lane the DPP control names), one 16-lane row at a time: no LDS round trip, unlike __shfl_xor on a double
template <int CTL>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTL, 0xF, 0xF, true);
  return v + __hiloint2double(hi, lo);
}

// The threads that hold a channel's sums after slab_sums: one per channel of the block, the first lane of a 16-lane row.
__device__ __forceinline__ bool bn_lead() { return threadIdx.x < 16 * BN_CH && threadIdx.x % 16 == 0; }
__device__ __forceinline__ int bn_lead_channel() { return blockIdx.x * BN_CH + threadIdx.x / 16; }

// Sums of the n <= BN_KC slabs slab_of(0 .. n-1) of the block's channels, added in list order to (dA, dB) of the bn_lead() threads.
//  * walk: thread (cl, rg) = (threadIdx.x % BN_CH, threadIdx.x / BN_CH).  The batches of ALL n slabs form one sequence, and the loads of
//    its next batch are issued before the adds of the current one: slab k + 1 is in flight while slab k is summed.  The partials of all
//    n slabs go to the panel [slab][rg][cl] and share the barriers of ONE tree.
//  * tree level 32 runs in the panel for all slabs, one barrier.  Level 16 is read from the panel by the first 16 BN_CH threads, thread
//    (channel threadIdx.x / 16, lane q of a 16-lane row) taking row group rg(q) = q0 q1 q3 q2 (bits of q, q0 the most significant bit of
//    rg): levels 8, 4, 2, 1 then pair lanes q ^ 1, q ^ 2, q ^ 8 and q ^ 4 of a row, which are DPP quad_perm [1,0,3,2], quad_perm
//    [2,3,0,1], row_ror:8 and row_ror:4 (q + 4 and q - 4 hold the same value once q ^ 8 has been added).  Every lane adds its partner
//    (fp64 addition commutes: the same pairs, the same bits), so all 16 lanes of a row end with the channel's sum.
// The caller puts a barrier between two calls on one panel.
template <class F>
__device__ __forceinline__ void slab_sums(F slab_of, int n, int C, bn_panel sh, double& dA, double& dB) {
  const int cl = threadIdx.x % BN_CH, rg = threadIdx.x / BN_CH;
  const int c = blockIdx.x * BN_CH + cl;
  const int cc = c < C ? c : C - 1;        // a thread past C walks the last channel; nobody reads its sums
  int k = 0, i = 0, k2 = 0, i2 = 0;         // the batch being summed: batch i of slab k; the one after it: batch i2 of slab k2
  SlabRef s = slab_of(0), s2 = s;
  double a = 0.0, b = 0.0;
  auto next = [&]() -> bool {               // is there a batch after (k, i)?
    k2 = k; i2 = i + 1; s2 = s;
    if ((long)i2 * BN_B >= s.rows) {
      k2 = k + 1; i2 = 0;
      if (k2 < n) s2 = slab_of(k2);
    }
    return k2 < n;
  };
  auto add = [&](const SlabBatch& cur) {    // sum batch (k, i); a slab's last batch sends its partial to the panel
    batch_add(cur, a, b);
    if (k2 != k) { sh[k][rg][cl] = make_double2(a, b); a = 0.0; b = 0.0; }
    k = k2; i = i2; s = s2;
  };
  SlabBatch t0, t1;
  batch_load(t0, s, C, cc, rg);
  for (;;) {                                // a load and the adds before it in ONE basic block: the adds wait for their own loads only
    if (!next()) { add(t0); break; }
    batch_load(t1, s2, C, cc, rg + i2 * BN_B); add(t0);
    if (!next()) { add(t1); break; }
    batch_load(t0, s2, C, cc, rg + i2 * BN_B); add(t1);
  }
  __syncthreads();
  if (rg < 32)
    for (int j = 0; j < n; ++j) {
      const double2 lo = sh[j][rg][cl], hi = sh[j][rg + 32][cl];
      sh[j][rg][cl] = make_double2(lo.x + hi.x, lo.y + hi.y);
    }
  __syncthreads();
  if (threadIdx.x < 16 * BN_CH) {
    const int q = threadIdx.x % 16, ch = threadIdx.x / 16;
    const int r = (q & 1) << 3 | (q & 2) << 1 | (q & 8) >> 2 | (q & 4) >> 2;
    for (int j = 0; j < n; ++j) {
      const double2 lo = sh[j][r][ch], hi = sh[j][r + 16][ch];
      double x = lo.x + hi.x, y = lo.y + hi.y;
      x = dpp_add_f64<0xB1>(x); y = dpp_add_f64<0xB1>(y);        // level 8: quad_perm [1,0,3,2]
      x = dpp_add_f64<0x4E>(x); y = dpp_add_f64<0x4E>(y);        // level 4: quad_perm [2,3,0,1]
      x = dpp_add_f64<0x128>(x); y = dpp_add_f64<0x128>(y);      // level 2: row_ror:8
      x = dpp_add_f64<0x124>(x); y = dpp_add_f64<0x124>(y);      // level 1: row_ror:4
      dA += x; dB += y;
    }
  }
}
// one slab: its sums, for the bn_lead() threads
__device__ __forceinline__ void slab_sum(const double* slab, int rows, int C, double& s0, double& s1, bn_panel sh) {
  s0 = 0.0; s1 = 0.0;
  slab_sums([&](int) { return SlabRef{slab, rows}; }, 1, C, sh, s0, s1);
}

__device__ __forceinline__ void bn_finalize_body(const addk_bn_finalize_args& p, bn_panel sh) {
  const int c = bn_lead_channel();
  double s0, s1;
  slab_sum((const double*)p.partial, p.rows, p.C, s0, s1, sh);
  if (bn_lead() && c < p.C) {
    double mean = s0 / p.count;
    double var = s1 / p.count - mean * mean;
    if (var < 0.0) var = 0.0;
    if (!(p.count > 1.0)) var = 0.0;     // one value per channel has no variance: what the subtraction leaves is the rounding of its fp32 square (bnfin.h)
    double invstd = 1.0 / sqrt(var + (double)p.eps);
    float g = p.gamma ? p.gamma[c] : 1.f, be = p.beta ? p.beta[c] : 0.f;
    float a = (float)(g * invstd);
    p.a[c] = a;
    p.b[c] = (float)(be - mean * (g * invstd));
    if (p.mean) p.mean[c] = (float)mean;
    if (p.invstd) p.invstd[c] = (float)invstd;
    if (p.running_mean) {
      double unb = p.count > 1.0 ? var * p.count / (p.count - 1.0) : var;
      p.running_mean[c] = (float)((1.0 - p.momentum) * p.running_mean[c] + p.momentum * mean);
      p.running_var[c] = (float)((1.0 - p.momentum) * p.running_var[c] + p.momentum * unb);
    }
  }
}
__global__ void __launch_bounds__(BN_T) bn_finalize_kernel(const addk_bn_finalize_args p) {
  __shared__ double2 sh[1][BN_RG][BN_CH];
  bn_finalize_body(p, sh);
}
// several independent BatchNorms in one launch: block (x, y) = channel block x of table entry y
__global__ void __launch_bounds__(BN_T) bn_finalize_batch_kernel(const addk_bn_finalize_args* __restrict__ tab) {
  __shared__ double2 sh[1][BN_RG][BN_CH];
  const addk_bn_finalize_args p = tab[blockIdx.y];
  if (blockIdx.x * BN_CH >= p.C) return;
  bn_finalize_body(p, sh);
}

__device__ __forceinline__ void slab_reduce_body(const addk_slab_reduce_item& it, bn_panel sh) {
  const int c = bn_lead_channel();
  double s0, s1;
  slab_sum(it.partial, it.rows, it.C, s0, s1, sh);
  if (bn_lead() && c < it.C) { it.out[2 * c] = s0; it.out[2 * c + 1] = s1; }
}
__global__ void __launch_bounds__(BN_T) slab_reduce_kernel(const addk_slab_reduce_item it) {
  __shared__ double2 sh[1][BN_RG][BN_CH];
  slab_reduce_body(it, sh);
}
__global__ void __launch_bounds__(BN_T) slab_reduce_batch_kernel(const addk_slab_reduce_item* __restrict__ tab) {
  __shared__ double2 sh[1][BN_RG][BN_CH];
  const addk_slab_reduce_item it = tab[blockIdx.y];
  if (blockIdx.x * BN_CH >= it.C) return;
  slab_reduce_body(it, sh);
}

// channels c0, c0 + step, ... of one eval-mode BatchNorm
__device__ __forceinline__ void bn_eval_body(const addk_bn_eval_item& e, int c0, int step) {
  for (int c = c0; c < e.C; c += step) {
    float g = e.gamma ? e.gamma[c] : 1.f, be = e.beta ? e.beta[c] : 0.f;
    float s = g / sqrtf(e.running_var[c] + e.eps);
    e.a[c] = s; e.b[c] = be - e.running_mean[c] * s;
  }
}
__global__ void bn_eval_affine_kernel(const addk_bn_eval_item e) {
  bn_eval_body(e, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
// all BatchNorms of a plan in one launch: block b handles table entry b
__global__ void bn_eval_affine_batch_kernel(const addk_bn_eval_item* __restrict__ tab) {
  const addk_bn_eval_item e = tab[blockIdx.x];
  bn_eval_body(e, threadIdx.x, blockDim.x);
}

__device__ __forceinline__ void bn_bwd_body(const addk_bn_bwd_args& p, bn_panel sh) {
  const int c = bn_lead_channel();
  double dA = 0.0, dB = 0.0;
  for (int k0 = 0; k0 < p.nslab; k0 += BN_KC) {
    const int n = p.nslab - k0 < BN_KC ? p.nslab - k0 : BN_KC;
    if (k0) __syncthreads();              // wave 0 has read the panel of the pass before
    slab_sums([&](int k) { return SlabRef{(const double*)p.slab[k0 + k], p.rows[k0 + k]}; }, n, p.C, sh, dA, dB);
  }
  if (bn_lead() && c < p.C) {
    double mean = p.mean[c], invstd = p.invstd[c], gamma = p.gamma ? p.gamma[c] : 1.0, a = p.a[c];
    double t = dA - mean * dB;
    double dgamma = invstd * t, dbeta = dB;
    double dvar = -0.5 * gamma * t * invstd * invstd * invstd;
    double dmean_tot = -a * dB - (p.centered ? 0.0 : 2.0 * mean * dvar);
    if (p.dgamma) p.dgamma[c] = (float)((p.accumulate ? (double)p.dgamma[c] : 0.0) + dgamma);
    if (p.dbeta) p.dbeta[c] = (float)((p.accumulate ? (double)p.dbeta[c] : 0.0) + dbeta);
    if (p.dmv) { p.dmv[2 * c] = (float)dmean_tot; p.dmv[2 * c + 1] = (float)dvar; }
    if (p.c1) { p.c1[c] = (float)(dmean_tot / p.count); p.c2[c] = (float)(2.0 * dvar / p.count); }
  }
}
__global__ void __launch_bounds__(BN_T) bn_bwd_kernel(const addk_bn_bwd_args p) {
  __shared__ double2 sh[BN_KC][BN_RG][BN_CH];
  bn_bwd_body(p, sh);
}
__global__ void __launch_bounds__(BN_T) bn_bwd_batch_kernel(const addk_bn_bwd_args* __restrict__ tab) {
  __shared__ double2 sh[BN_KC][BN_RG][BN_CH];
  const addk_bn_bwd_args& p = tab[blockIdx.y];
  if (blockIdx.x * BN_CH >= p.C) return;
  bn_bwd_body(p, sh);
}

__device__ __forceinline__ void bn_coeffs_body(const addk_bn_coeffs_item& it) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < it.C) { it.c1[c] = (float)((double)it.dmv[2 * c] / it.count); it.c2[c] = (float)(2.0 * (double)it.dmv[2 * c + 1] / it.count); }
}
__global__ void bn_coeffs_kernel(const addk_bn_coeffs_item it) { bn_coeffs_body(it); }
__global__ void bn_coeffs_batch_kernel(const addk_bn_coeffs_item* __restrict__ tab) {
  const addk_bn_coeffs_item it = tab[blockIdx.y];
  bn_coeffs_body(it);
}

}  // namespace

extern "C" int addk_bn_finalize(const addk_bn_finalize_args* a, void* stream) {
  ADDK_REQUIRE(a && a->partial && a->a && a->b && a->C > 0 && a->rows > 0 && a->count > 0, "bn_finalize: bad args");
  ADDK_REQUIRE((a->running_mean == nullptr) == (a->running_var == nullptr), "bn_finalize: running stats come together");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(a->C, BN_CH)), dim3(BN_T), 0, (hipStream_t)stream, *a);
  return addk_check_launch("bn_finalize");
}

extern "C" int addk_slab_reduce(const addk_slab_reduce_item* it, void* stream) {
  ADDK_REQUIRE(it && it->partial && it->out && it->rows > 0 && it->C > 0, "slab_reduce: bad args");
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(cdiv(it->C, BN_CH)), dim3(BN_T), 0, (hipStream_t)stream, *it);
  return addk_check_launch("slab_reduce");
}

extern "C" int addk_bn_eval_affine(const addk_bn_eval_item* it, void* stream) {
  ADDK_REQUIRE(it && it->running_mean && it->running_var && it->a && it->b && it->C > 0, "bn_eval_affine: bad args");
  hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(cdiv(it->C, 256)), dim3(256), 0, (hipStream_t)stream, *it);
  return addk_check_launch("bn_eval_affine");
}

extern "C" int addk_bn_bwd(const addk_bn_bwd_args* a, void* stream) {
  ADDK_REQUIRE(a && a->nslab >= 0 && a->nslab <= ADDK_MAX_SLAB && a->C > 0 && a->count > 0, "bn_bwd: bad args");
  ADDK_REQUIRE(a->mean && a->invstd && a->a, "bn_bwd: saved statistics missing");
  ADDK_REQUIRE((a->c1 == nullptr) == (a->c2 == nullptr) && (a->c1 || a->dmv), "bn_bwd: need c1/c2 or dmv");
  for (int i = 0; i < a->nslab; ++i) ADDK_REQUIRE(a->slab[i] && a->rows[i] > 0, "bn_bwd: bad slab %d", i);
  hipLaunchKernelGGL(bn_bwd_kernel, dim3(cdiv(a->C, BN_CH)), dim3(BN_T), 0, (hipStream_t)stream, *a);
  return addk_check_launch("bn_bwd");
}

extern "C" int addk_bn_bwd_coeffs(const addk_bn_coeffs_item* it, void* stream) {
  ADDK_REQUIRE(it && it->dmv && it->c1 && it->c2 && it->C > 0 && it->count > 0, "bn_bwd_coeffs: bad args");
  hipLaunchKernelGGL(bn_coeffs_kernel, dim3(cdiv(it->C, 256)), dim3(256), 0, (hipStream_t)stream, *it);
  return addk_check_launch("bn_bwd_coeffs");
}

extern "C" int addk_bn_eval_affine_batch(const addk_bn_eval_item* dev_table, int32_t n, void* stream) {
  ADDK_REQUIRE(dev_table && n > 0, "bn_eval_affine_batch: bad args");
  hipLaunchKernelGGL(bn_eval_affine_batch_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, dev_table);
  return addk_check_launch("bn_eval_affine_batch");
}

extern "C" int addk_bn_finalize_batch(const addk_bn_finalize_args* dev_table, int32_t n, int32_t max_C, void* stream) {
  ADDK_REQUIRE(dev_table && n > 0 && max_C > 0, "bn_finalize_batch: bad args");
  hipLaunchKernelGGL(bn_finalize_batch_kernel, dim3(cdiv(max_C, BN_CH), n), dim3(BN_T), 0, (hipStream_t)stream, dev_table);
  return addk_check_launch("bn_finalize_batch");
}
extern "C" int addk_bn_bwd_batch(const addk_bn_bwd_args* dev_table, int32_t n, int32_t max_C, void* stream) {
  ADDK_REQUIRE(dev_table && n > 0 && max_C > 0, "bn_bwd_batch: bad args");
  hipLaunchKernelGGL(bn_bwd_batch_kernel, dim3(cdiv(max_C, BN_CH), n), dim3(BN_T), 0, (hipStream_t)stream, dev_table);
  return addk_check_launch("bn_bwd_batch");
}

extern "C" int addk_slab_reduce_batch(const addk_slab_reduce_item* dev_table, int32_t n, int32_t max_C, void* stream) {
  ADDK_REQUIRE(dev_table && n > 0 && max_C > 0, "slab_reduce_batch: bad args");
  hipLaunchKernelGGL(slab_reduce_batch_kernel, dim3(cdiv(max_C, BN_CH), n), dim3(BN_T), 0, (hipStream_t)stream, dev_table);
  return addk_check_launch("slab_reduce_batch");
}
extern "C" int addk_bn_bwd_coeffs_batch(const addk_bn_coeffs_item* dev_table, int32_t n, int32_t max_C, void* stream) {
  ADDK_REQUIRE(dev_table && n > 0 && max_C > 0, "bn_bwd_coeffs_batch: bad args");
  hipLaunchKernelGGL(bn_coeffs_batch_kernel, dim3(cdiv(max_C, 256), n), dim3(256), 0, (hipStream_t)stream, dev_table);
  return addk_check_launch("bn_bwd_coeffs_batch");
}
