// The training head on the decoder's low-resolution logits: fused up-sampling + cross-entropy, forward and backward (ce_up_kernel of
// ce_up.h, in its plain, mining, distillation and soft-Dice forms; loss_shape.hip has the focal and label-smoothed ones), and the hard
// example mining that feeds it (ohem_*_kernel, addk_ohem_select).
#include <string>
#include "ce_up.h"

namespace {

// second stage of the distillation term: the KL partials in the order of sum_partials_kernel; kd = coef * Σ / n, exactly 0 when no pixel
// is valid.  kd_out is written (a replayed graph leaves the last step's value), the loss accumulates it.
__global__ void __launch_bounds__(256) kd_sum_kernel(const float* ws, int n, float coef, const float* nvalid, float* kd_out, float* loss_out) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += ws[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float nv = *nvalid;
    const float kd = nv > 0.f ? s * coef / nv : 0.f;
    *kd_out = kd;
    *loss_out += kd;
  }
}

// ---- online hard example mining for the fused loss head (addk_ohem_select) -------------------------------------------------------------
// Per exit: the per-pixel loss l = max(0, logsumexp(z) - z[target]) of every valid full-resolution pixel, the EXACT order statistic
// l_(min(K, n)) of the batch and tau = min(-log theta, l_(k)), all on the stream.  l >= 0, so its fp32 bit pattern orders like l: a
// three-pass most-significant-first radix select on the bits (11 + 11 + 10) finds the pattern of the k-th largest value.
//   ohem_loss_kernel     the walk of scu_walk (same tile, same interpolation); writes l (or -1: not valid) to the [N,OH,OW] map and bins
//                        bits 31..21 into a 2048-bin LDS histogram (a thread merges the run of equal bins of its column first), flushed
//                        with 32-bit integer atomics: order-independent, exact.
//   ohem_scan_kernel     ONE workgroup between the passes: walks a histogram from the top bin down to the bin that holds rank k, appends
//                        its index to the selected prefix and leaves the rank within that bin.  A launch of its own, not a scan at the
//                        top of every workgroup of the next pass: the refinement kernels stay pure streaming loops (no 8 KB histogram
//                        re-read and no block scan in ~1000 workgroups), at the price of three 1-workgroup launches per exit.
//   ohem_refine_kernel   streams the STORED map: pixels whose leading bits equal the prefix are binned on the next 11 / 10 bits.
//   ohem_keep_kernel     streams the stored map against tau: per workgroup the count of kept pixels and the sum of their weights;
//   ohem_keep_sum_kernel one workgroup adds the partials in a fixed order (the float sum as sum_partials_kernel does).
// Workspace (32-bit words): [0..2047] hist of pass 0, [2048..4095] pass 1, [4096..5119] pass 2, [5120] prefix, [5121] rank, then
// OHEM_KEEP_BLOCKS float weight partials and as many kept counts.  The first 5122 words are cleared by the launch sequence itself.
constexpr int OHEM_B0 = 2048, OHEM_B2 = 1024;
constexpr int OHEM_SEL = 2 * OHEM_B0 + OHEM_B2, OHEM_PART = OHEM_SEL + 2;
constexpr int OHEM_KEEP_BLOCKS = 1024;
constexpr unsigned OHEM_NONE = 0xffffffffu;                       // prefix of an empty selection (n == 0): no bit pattern matches it

__global__ void __launch_bounds__(256) ohem_clear_kernel(unsigned* ws) {
  for (int i = threadIdx.x; i < OHEM_PART; i += 256) ((gu32*)ws)[i] = 0u;
}

struct OhemLossK : UpSrc { const int64_t* target; int ignore; float* lmap; unsigned* hist; };

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) ohem_loss_kernel(const OhemLossK p) {
  __shared__ unsigned hist[OHEM_B0];
  const int t = threadIdx.x;
  for (int i = t; i < OHEM_B0; i += 256) hist[i] = 0u;
  __syncthreads();
  const int64_t __attribute__((address_space(1)))* tgt = (const int64_t __attribute__((address_space(1)))*)p.target;
  int key = -1; unsigned run = 0;                                // pending run of equal bins of this column
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    const long tg = tgt[pix];
    const bool valid = tg != p.ignore && tg >= 0 && tg < CC;
    float mx = -INFINITY, zt = 0.f;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      mx = fmaxf(mx, z[c]);
      if (c == tg) zt = z[c];
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < CC; ++c) se += __expf(z[c] - mx);
    const float l = valid ? fmaxf(0.f, logf(se) + mx - zt) : -1.f;
    ((gfloat*)p.lmap)[pix] = l;
    const int k = valid ? (int)(__float_as_uint(l) >> 21) : -1;
    run_count(hist, key, run, k);
  });
  run_flush(hist, key, run);
  __syncthreads();
  for (int i = t; i < OHEM_B0; i += 256) {
    const unsigned v = hist[i];
    if (v) atomicAdd(&p.hist[i], v);
  }
}

// One workgroup.  hist: NBIN = 256 * per counters of the pass; sel = {prefix, rank}.  pass 0 takes rank = min(K, n) with n the histogram's
// total (also written to counts[0]); the last pass turns the completed 32-bit pattern into tau = min(tau_theta, l_(k)).
__global__ void __launch_bounds__(256) ohem_scan_kernel(const unsigned* hist, int per, int bits, int pass, unsigned* sel, unsigned long long kmin,
                                                        float tau_theta, float* tau, long long* counts) {
  __shared__ unsigned sc[256];
  const int t = threadIdx.x, nbin = 256 * per;
  const gu32* h = (const gu32*)hist;
  // thread t owns the bins nbin-1 - t*per ... nbin - (t+1)*per, largest first
  unsigned c = 0;
  for (int j = 0; j < per; ++j) c += h[nbin - 1 - (t * per + j)];
  sc[t] = c;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {                            // inclusive scan over the threads
    const unsigned add = t >= d ? sc[t - d] : 0u;
    __syncthreads();
    sc[t] += add;
    __syncthreads();
  }
  const unsigned total = sc[255], above = sc[t] - c;
  unsigned prefix = 0u, k;
  if (pass == 0) {
    k = kmin < (unsigned long long)total ? (unsigned)kmin : total;
    if (t == 0) ((__attribute__((address_space(1))) long long*)counts)[0] = (long long)total;
  } else {
    prefix = ((const gu32*)sel)[0]; k = ((const gu32*)sel)[1];
  }
  __syncthreads();                                               // every thread has read sel before one rewrites it
  if (k == 0u || prefix == OHEM_NONE) {                          // nothing to select: n == 0
    if (t == 0) {
      ((gu32*)sel)[0] = OHEM_NONE; ((gu32*)sel)[1] = 0u;
      if (tau) *(gfloat*)tau = tau_theta;
    }
    return;
  }
  if (above < k && k <= above + c) {                             // exactly one thread: 1 <= k <= total
    unsigned a = above; int b = nbin - 1 - t * per;
    for (int j = 0; j < per; ++j, --b) {
      const unsigned v = h[b];
      if (k <= a + v) break;
      a += v;
    }
    const unsigned np = (prefix << bits) | (unsigned)b;
    ((gu32*)sel)[0] = np; ((gu32*)sel)[1] = k - a;
    if (tau) *(gfloat*)tau = fminf(tau_theta, __uint_as_float(np));
  }
}

// pixels of the stored map whose bits >> PS equal the selected prefix are binned on (bits >> BS) & (NBIN - 1)
template <int PS, int BS, int NBIN>
__global__ void __launch_bounds__(256) ohem_refine_kernel(const float* lmap, long n, const unsigned* sel, unsigned* hist) {
  __shared__ unsigned sh[NBIN];
  const int t = threadIdx.x;
  for (int i = t; i < NBIN; i += 256) sh[i] = 0u;
  __syncthreads();
  const unsigned prefix = ((const gu32*)sel)[0];
  if (prefix == OHEM_NONE) return;                               // uniform over the grid
  const gu32* m = (const gu32*)lmap;
  for (long i = (long)blockIdx.x * 256 + t; i < n; i += (long)gridDim.x * 256) {
    const unsigned b = m[i];
    if ((b >> PS) == prefix) atomicAdd(&sh[(b >> BS) & (NBIN - 1)], 1u);
  }
  __syncthreads();
  for (int i = t; i < NBIN; i += 256) {
    const unsigned v = sh[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

__global__ void __launch_bounds__(256) ohem_keep_kernel(const float* lmap, const int64_t* target, const float* cw, long n, const float* tau,
                                                        float* wpart, unsigned* kpart) {
  __shared__ float shs[4];
  __shared__ unsigned shk[4];
  const int t = threadIdx.x;
  const float ta = *(const gfloat*)tau;
  const gfloat* m = (const gfloat*)lmap;
  const int64_t __attribute__((address_space(1)))* tgt = (const int64_t __attribute__((address_space(1)))*)target;
  float s = 0.f; unsigned k = 0u;
  for (long i = (long)blockIdx.x * 256 + t; i < n; i += (long)gridDim.x * 256) {
    if (m[i] >= ta) {                                            // not valid: -1 < 0 <= tau
      ++k;
      s += cw ? ((const gfloat*)cw)[tgt[i]] : 1.f;
    }
  }
  s = block_sum(s, shs);
  for (int mk = 32; mk > 0; mk >>= 1) k += __shfl_xor(k, mk);
  if ((t & 63) == 0) shk[t >> 6] = k;
  __syncthreads();
  if (t == 0) { ((gfloat*)wpart)[blockIdx.x] = s; ((gu32*)kpart)[blockIdx.x] = shk[0] + shk[1] + shk[2] + shk[3]; }
}

__global__ void __launch_bounds__(256) ohem_keep_sum_kernel(const float* wpart, const unsigned* kpart, int n, float* wsum, long long* counts) {
  __shared__ float shs[4];
  __shared__ unsigned long long shk[4];
  const int t = threadIdx.x;
  float s = 0.f; unsigned long long k = 0ull;
  for (int i = t; i < n; i += 256) { s += ((const gfloat*)wpart)[i]; k += ((const gu32*)kpart)[i]; }
  s = block_sum(s, shs);
  for (int mk = 32; mk > 0; mk >>= 1) k += __shfl_xor(k, mk);
  if ((t & 63) == 0) shk[t >> 6] = k;
  __syncthreads();
  if (t == 0) {
    *(gfloat*)wsum = s;
    ((__attribute__((address_space(1))) long long*)counts)[1] = (long long)(shk[0] + shk[1] + shk[2] + shk[3]);
  }
}

bool ohem_ok(int N, int H, int W, int OH, int OW, int C) {
  return scu_head_ok(N, H, W, OH, OW, C) && (long)N * OH * OW < (1L << 31);
}
int ohem_stream_blocks(long n) { long b = cdiv(n, 256 * 16); if (b < 1) b = 1; if (b > OHEM_KEEP_BLOCKS) b = OHEM_KEEP_BLOCKS; return (int)b; }

// The training head's launches, all three entry points (`name`: the entry point's prefix in error texts and launch names): the stride and
// shape checks, one fill of the argument struct (CeUpKdK extends CeUpOhemK extends CeUpK: a plainer form takes its base), the
// instantiation by (mining: lmap / tau given, distillation: kd given, the teacher's loader), the loss partials' sum and, for a student,
// the KL partials' sum.  coef: the soft-Dice forms of the same instantiations.
int ceu_launch(const char* name, const addk_ce_upsample_args* a, const float* lmap, const float* tau, const addk_ce_upsample_kd_args* kd,
               hipStream_t st, const float* coef = nullptr) {
  ADDK_REQUIRE(a->ld >= a->C && a->ldg >= a->C && (!kd || kd->ld_teacher >= a->C), "%s: short stride", name);
  ADDK_REQUIRE(ceu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "%s: unsupported shape (%s, at most %d output rows per input row)", name,
               head_classes_text().c_str(), CEU_MAXBAND);
  CeUpKdK k{};
  const dim3 grid = ceu_fill(k, a, lmap, tau);
  const int nblk = (int)(grid.x * grid.y * grid.z);
  if (kd) {
    k.teacher = kd->teacher; k.ldt = kd->ld_teacher; k.nvalid = kd->nvalid; k.ws2 = a->ws + nblk;
    k.rT = 1.f / kd->temperature;
    k.kscale = a->scale * kd->alpha * kd->temperature;           // the gradient's factor before 1/n; the loss takes one more T
  }
  head_classes(a->C, [&](auto cc) {                               // ceu_ok: a->C is of the list
    constexpr int CC = decltype(cc)::value;
    const bool tvec = kd && px_vec_ok<CC>(kd->teacher, kd->ld_teacher);
    if (coef) {
      CeUpDiceK d{};
      static_cast<CeUpKdK&>(d) = k;
      d.coef = coef;
      if (kd && lmap) launch_vec(tvec, ce_up_kernel<CC, true, true, true, true>, ce_up_kernel<CC, true, true, false, true>, grid, st, d);
      else if (kd) launch_vec(tvec, ce_up_kernel<CC, false, true, true, true>, ce_up_kernel<CC, false, true, false, true>, grid, st, d);
      else if (lmap) hipLaunchKernelGGL((ce_up_kernel<CC, true, false, false, true>), grid, dim3(256), 0, st, d);
      else hipLaunchKernelGGL((ce_up_kernel<CC, false, false, false, true>), grid, dim3(256), 0, st, d);
    } else if (kd) {
      if (lmap) launch_vec(tvec, ce_up_kernel<CC, true, true, true>, ce_up_kernel<CC, true, true, false>, grid, st, k);
      else launch_vec(tvec, ce_up_kernel<CC, false, true, true>, ce_up_kernel<CC, false, true, false>, grid, st, k);
    } else if (lmap) {
      hipLaunchKernelGGL((ce_up_kernel<CC, true>), grid, dim3(256), 0, st, static_cast<const CeUpOhemK&>(k));
    } else {
      hipLaunchKernelGGL(ce_up_kernel<CC>, grid, dim3(256), 0, st, static_cast<const CeUpK&>(k));
    }
  });
  const std::string n(name);
  int rc = addk_check_launch(name);
  if (rc) return rc;
  hipLaunchKernelGGL(sum_partials_kernel<>, dim3(1), dim3(256), 0, st, a->ws, nblk, a->scale, a->wsum, a->loss_out, 1);
  rc = addk_check_launch((n + "_sum").c_str());
  if (rc || !kd) return rc;
  hipLaunchKernelGGL(kd_sum_kernel, dim3(1), dim3(256), 0, st, k.ws2, nblk, k.kscale * kd->temperature, kd->nvalid, kd->kd_out, a->loss_out);
  return addk_check_launch((n + "_kl_sum").c_str());
}

}  // namespace

extern "C" int addk_head_classes(int32_t* out, int32_t cap) { return classes_out<HeadClasses>(out, cap); }
extern "C" int addk_gate_head_classes(int32_t* out, int32_t cap) { return classes_out<GateClasses>(out, cap); }

extern "C" int addk_ce_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return ceu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_ce_upsample_ws_floats(int32_t N, int32_t H, int32_t W) {
  return (int64_t)N * cdiv(H, ceu_hb(H)) * cdiv(W, CEU_X - 1);
}
extern "C" int addk_ce_upsample_fwd_bwd(const addk_ce_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->wsum && a->loss_out && a->g && a->ws, "ce_upsample: null pointer");
  return ceu_launch("ce_upsample", a, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int addk_ce_upsample_ohem_fwd_bwd(const addk_ce_upsample_ohem_args* b, void* stream) {
  ADDK_REQUIRE(b, "ce_upsample_ohem: null pointer");
  const addk_ce_upsample_args* a = &b->ce;
  ADDK_REQUIRE(a->logits && a->target && a->wsum && a->loss_out && a->g && a->ws && b->pix_loss && b->tau, "ce_upsample_ohem: null pointer");
  return ceu_launch("ce_upsample_ohem", a, b->pix_loss, b->tau, nullptr, (hipStream_t)stream);
}

extern "C" int addk_ce_upsample_kd_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return ceu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_ce_upsample_kd_ws_floats(int32_t N, int32_t H, int32_t W) {
  return 2 * addk_ce_upsample_ws_floats(N, H, W);                // the loss partials, then the KL partials
}
extern "C" int addk_ce_upsample_kd_fwd_bwd(const addk_ce_upsample_kd_args* b, void* stream) {
  ADDK_REQUIRE(b, "ce_upsample_kd: null pointer");
  const addk_ce_upsample_args* a = &b->ce;
  ADDK_REQUIRE(a->logits && a->target && a->wsum && a->loss_out && a->g && a->ws && b->teacher && b->nvalid && b->kd_out, "ce_upsample_kd: null pointer");
  ADDK_REQUIRE((b->pix_loss == nullptr) == (b->tau == nullptr), "ce_upsample_kd: pix_loss and tau come together (both NULL: no mining)");
  ADDK_REQUIRE(b->teacher != a->logits, "ce_upsample_kd: the teacher must be another exit's logits");
  ADDK_REQUIRE(isfinite(b->alpha) && b->alpha > 0.f && isfinite(b->temperature) && b->temperature > 0.f,
               "ce_upsample_kd: alpha and temperature must be positive and finite");
  return ceu_launch("ce_upsample_kd", a, b->pix_loss, b->tau, b, (hipStream_t)stream);
}

extern "C" int addk_ce_upsample_dice_fwd_bwd(const addk_ce_upsample_dice_args* d, void* stream) {
  ADDK_REQUIRE(d, "ce_upsample_dice: null pointer");
  const addk_ce_upsample_kd_args* b = &d->kd;
  const addk_ce_upsample_args* a = &b->ce;
  ADDK_REQUIRE(a->logits && a->target && a->wsum && a->loss_out && a->g && a->ws && d->coef, "ce_upsample_dice: null pointer");
  ADDK_REQUIRE((b->pix_loss == nullptr) == (b->tau == nullptr), "ce_upsample_dice: pix_loss and tau come together (both NULL: no mining)");
  if (b->teacher) {
    ADDK_REQUIRE(b->nvalid && b->kd_out, "ce_upsample_dice: null pointer");
    ADDK_REQUIRE(b->teacher != a->logits, "ce_upsample_dice: the teacher must be another exit's logits");
    ADDK_REQUIRE(isfinite(b->alpha) && b->alpha > 0.f && isfinite(b->temperature) && b->temperature > 0.f,
                 "ce_upsample_dice: alpha and temperature must be positive and finite");
  }
  return ceu_launch("ce_upsample_dice", a, b->pix_loss, b->tau, b->teacher ? b : nullptr, (hipStream_t)stream, d->coef);
}

extern "C" int addk_ohem_select_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return ohem_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_ohem_select_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  return 4 * (int64_t)(OHEM_PART + 2 * OHEM_KEEP_BLOCKS);
}
extern "C" int addk_ohem_select(const addk_ohem_select_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->pix_loss && a->tau && a->wsum_kept && a->counts && a->ws, "ohem_select: null pointer");
  ADDK_REQUIRE(a->thresh > 0.f && a->thresh <= 1.f, "ohem_select: thresh must lie in (0, 1]");
  ADDK_REQUIRE(a->min_kept_total >= 1, "ohem_select: min_kept_total must be at least 1");
  ADDK_REQUIRE(a->ld >= a->C, "ohem_select: short stride");
  ADDK_REQUIRE(ohem_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "ohem_select: unsupported shape (%s, fewer than 2^31 pixels)",
               head_classes_text().c_str());
  unsigned* w = (unsigned*)a->ws;
  unsigned* sel = w + OHEM_SEL;
  float* wpart = (float*)(w + OHEM_PART);
  unsigned* kpart = w + OHEM_PART + OHEM_KEEP_BLOCKS;
  const float tau_theta = a->thresh >= 1.f ? 0.f : (float)(-log((double)a->thresh));
  const long npix = (long)a->N * a->OH * a->OW;
  const int nb = ohem_stream_blocks(npix);
  long long* counts = (long long*)a->counts;
  OhemLossK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.ignore = a->ignore_index; k.lmap = a->pix_loss; k.hist = w;
  hipStream_t st = (hipStream_t)stream;
  const dim3 one(1), blk(256);
  hipLaunchKernelGGL(ohem_clear_kernel, one, blk, 0, st, w);
  head_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), ohem_loss_kernel<CC, true>, ohem_loss_kernel<CC, false>, scu_grid(a->N, a->OH, a->OW), st, k);
  });
  hipLaunchKernelGGL(ohem_scan_kernel, one, blk, 0, st, w, OHEM_B0 / 256, 11, 0, sel, (unsigned long long)a->min_kept_total, tau_theta, (float*)nullptr, counts);
  hipLaunchKernelGGL((ohem_refine_kernel<21, 10, OHEM_B0>), dim3(nb), blk, 0, st, a->pix_loss, npix, sel, w + OHEM_B0);
  hipLaunchKernelGGL(ohem_scan_kernel, one, blk, 0, st, w + OHEM_B0, OHEM_B0 / 256, 11, 1, sel, 0ull, tau_theta, (float*)nullptr, counts);
  hipLaunchKernelGGL((ohem_refine_kernel<10, 0, OHEM_B2>), dim3(nb), blk, 0, st, a->pix_loss, npix, sel, w + 2 * OHEM_B0);
  hipLaunchKernelGGL(ohem_scan_kernel, one, blk, 0, st, w + 2 * OHEM_B0, OHEM_B2 / 256, 10, 2, sel, 0ull, tau_theta, a->tau, counts);
  hipLaunchKernelGGL(ohem_keep_kernel, dim3(nb), blk, 0, st, a->pix_loss, a->target, a->class_w, npix, a->tau, wpart, kpart);
  hipLaunchKernelGGL(ohem_keep_sum_kernel, one, blk, 0, st, wpart, kpart, nb, a->wsum_kept, counts);
  return addk_check_launch("ohem_select");
}
