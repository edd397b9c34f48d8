// The validation heads on the decoder's low-resolution logits: the scoring head (confusion matrix, loss, entropy: score_up_kernel) and
// the per-image exit profile, plain and tempered (profile_up_kernel).
#include "up.h"

namespace {

// ---- fused logits up-sampling + scoring of a validation pass (decoder.py:28 + train.py:268-285) --------------------------
// Confusion matrix, loss and entropy of one exit from the low-resolution NHWC logits, as a GATHER: a wave owns 64 consecutive
// columns X of the high-resolution grid and walks SCU_R rows; a thread keeps the two W-interpolated rows t0 = lw0*v(h0,w0) +
// lw1*v(h0,w1), t1 = (same on h1) of its column in registers and reloads them only when the (wave-uniform) pair (h0, h1)
// changes, so at the x8 of config 2 the four neighbours are read once per 8 pixels and a pixel costs CC x 3 flops of
// interpolation — z = lh0*t0 + lh1*t1 is the expression of resize_fwd_nchw_kernel / ce_up_kernel, operation for operation.
// One max/arg-max sweep, one exp sweep (Σe, Σe·d) serves loss and entropy.  HBM traffic: the target (coalesced 512 B per wave
// row) and the optional uint8 map; the logits (5 MB at config 2) stay in L2.  Counts go to a CC x CC LDS histogram (361 entries at 19 classes, 441 at 21) (a thread
// merges the run of equal (gt, pred) keys of its column first), flushed once per workgroup with 64-bit integer atomics:
// order-independent, exact.  Loss and entropy leave the workgroup as two partials reduced in a fixed order.
struct ScoreUpK : UpSrc {
  const int64_t* target; const float* cw; int ignore;
  unsigned long long* cm; uint8_t* pred;
  float* ws; int nblk;
};

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) score_up_kernel(const ScoreUpK p) {
  __shared__ unsigned hist[CC * CC];
  __shared__ float shs[4];
  const int t = threadIdx.x;
  for (int i = t; i < CC * CC; i += 256) hist[i] = 0u;
  __syncthreads();
  const int64_t __attribute__((address_space(1)))* tgt = (const int64_t __attribute__((address_space(1)))*)p.target;
  const gfloat* cw = (const gfloat*)p.cw;
  float lsum = 0.f, esum = 0.f;
  int key = -1; unsigned run = 0;                                // pending (gt, pred) run of this column
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    const long tg = tgt[pix];
    const bool valid = tg != p.ignore && tg >= 0 && tg < CC;
    float mx = -INFINITY, zt = 0.f; int am = 0;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (z[c] > mx) { mx = z[c]; am = c; }                      // strict: a tie keeps the lowest channel
      if (c == tg) zt = z[c];
    }
    float se, sx;
    exp_sweep<CC>(z, mx, se, sx);
    const float lse = logf(se);
    if (valid) lsum += (cw ? cw[tg] : 1.f) * (lse + mx - zt);
    esum += lse - sx / se;
    if (p.pred) p.pred[pix] = (uint8_t)am;
    const int k = (tg >= 0 && tg < CC) ? (int)tg * CC + am : -1;     // the evaluator's mask: labels in [0, C), whatever ignore_index is
    run_count(hist, key, run, k);
  });
  run_flush(hist, key, run);
  lsum = block_sum(lsum, shs);
  esum = block_sum(esum, shs);
  const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (t == 0) { ((gfloat*)p.ws)[blk] = lsum; ((gfloat*)p.ws)[p.nblk + blk] = esum; }
  __syncthreads();
  for (int i = t; i < CC * CC; i += 256) {
    const unsigned v = hist[i];
    if (v) atomicAdd(&p.cm[i], (unsigned long long)v);
  }
}

// second stage of score_up_kernel: block 0 finishes the loss (scale / wsum), block 1 the entropy, each in a fixed order
__global__ void __launch_bounds__(256) score_sum_kernel(const float* ws, int n, float scale, const float* wsum, float* loss_out, float* ent_out) {
  __shared__ float sh[4];
  const float* w = ws + (long)blockIdx.x * n;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += w[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) *loss_out += s * scale / *wsum;
    else *ent_out += s;
  }
}

// ---- fused logits up-sampling + per-image exit profile (decoder.py:28 + eval.py:195-230) --------------------------------------
// What the early-exit operating curve needs of one exit, PER IMAGE (grid z), in one walk: the gate kernel's normalised entropy, its
// share of pixels with top probability 1/se > thr[j] for up to PRU_NT thresholds at once (one register counter each: no atomics), and
// the scoring kernel's confusion matrix (same arg-max sweep, same LDS histogram, flushed into the image's own [CC,CC] block) and
// optional uint8 map.  No loss.  The per-pixel values are the two parents' operation for operation — the strict `>` sweep leaves the
// max that fmaxf leaves — and the tail is the gate's (up_finish), so entropy and shares carry the gate's bits and the matrix the scorer's.
constexpr int PRU_NT = 16;
struct ProfileUpK : UpSrc {
  const int64_t* target; const float* thr; int nthr;
  float* ent; float* share; unsigned long long* cm; uint8_t* pred;
  unsigned* counter; float* part; unsigned* cnt;          // ws: [ticket, 16 bytes][nblk floats][nblk x PRU_NT counts], image-major
  int nblk_img;
  double npix, ent_div;
};

// TEMP: the tempered launch (addk_profile_upsample_t) takes entropy and shares from softmax(z * *inv_temp); the word rides behind the
// untempered arguments, whose layout and kernels stay as they are
struct ProfileUpTK : ProfileUpK { const float* inv_temp; };
template <bool TEMP> struct ProfileUpArg { typedef ProfileUpK type; };
template <> struct ProfileUpArg<true> { typedef ProfileUpTK type; };

template <int CC, bool VEC, bool TEMP = false>
__global__ void __launch_bounds__(256) profile_up_kernel(const typename ProfileUpArg<TEMP>::type p) {
  __shared__ unsigned hist[CC * CC];
  const int t = threadIdx.x;
  for (int i = t; i < CC * CC; i += 256) hist[i] = 0u;
  __syncthreads();
  const int64_t __attribute__((address_space(1)))* tgt = (const int64_t __attribute__((address_space(1)))*)p.target;
  float thr[PRU_NT];                                             // wave-uniform; an unused slot never counts (1/se <= 1)
#pragma unroll
  for (int j = 0; j < PRU_NT; ++j) thr[j] = j < p.nthr ? ((const gfloat*)p.thr)[j] : INFINITY;
  float esum = 0.f; unsigned hit[PRU_NT];
#pragma unroll
  for (int j = 0; j < PRU_NT; ++j) hit[j] = 0u;
  float it = 1.f;
  if constexpr (TEMP) it = *(const gfloat*)p.inv_temp;
  int key = -1; unsigned run = 0;                                // pending (gt, pred) run of this column
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    const long tg = tgt[pix];
    float mx = -INFINITY; int am = 0;
#pragma unroll
    for (int c = 0; c < CC; ++c)
      if (z[c] > mx) { mx = z[c]; am = c; }                      // strict: a tie keeps the lowest channel
    float se, sx;
    if constexpr (TEMP) exp_sweep_t<CC>(z, mx, it, se, sx);
    else exp_sweep<CC>(z, mx, se, sx);
    esum += logf(se) - sx / se;
    const float pmax = 1.f / se;
#pragma unroll
    for (int j = 0; j < PRU_NT; ++j) hit[j] += (pmax > thr[j]) ? 1u : 0u;
    if (p.pred) p.pred[pix] = (uint8_t)am;
    const int k = (tg >= 0 && tg < CC) ? (int)tg * CC + am : -1;     // the evaluator's mask: labels in [0, C), whatever ignore_index is
    run_count(hist, key, run, k);
  });
  run_flush(hist, key, run);
  __syncthreads();
  unsigned long long* cm = p.cm + (long)blockIdx.z * (CC * CC);
  for (int i = t; i < CC * CC; i += 256) {
    const unsigned v = hist[i];
    if (v) atomicAdd(&cm[i], (unsigned long long)v);
  }
  up_finish<PRU_NT>(esum, hit, p.nthr, p.counter, p.part, p.cnt, p.N, p.nblk_img, false, [&](int img, double es, auto&& count) {
    ((gfloat*)p.ent)[img] = (float)(es / p.ent_div);
    for (int j = 0; j < p.nthr; ++j) ((gfloat*)p.share)[(long)img * p.nthr + j] = (float)((double)count(j) / p.npix);
  });
}

}  // namespace

extern "C" int addk_score_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return scu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_score_upsample_ws_floats(int32_t N, int32_t OH, int32_t OW) {
  return 2 * scu_blocks(N, OH, OW);
}
extern "C" int addk_score_upsample(const addk_score_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->wsum && a->loss_out && a->ent_out && a->cm && a->ws, "score_upsample: null pointer");
  ADDK_REQUIRE(a->ld >= a->C, "score_upsample: short stride");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "score_upsample: unsupported shape (%s)", gate_classes_text().c_str());
  const dim3 grid = scu_grid(a->N, a->OH, a->OW);
  ScoreUpK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.cw = a->class_w; k.ignore = a->ignore_index;
  k.cm = reinterpret_cast<unsigned long long*>(a->cm); k.pred = a->pred_out;
  k.ws = a->ws; k.nblk = (int)scu_blocks(a->N, a->OH, a->OW);
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), score_up_kernel<CC, true>, score_up_kernel<CC, false>, grid, st, k);
  });
  int rc = addk_check_launch("score_upsample");
  if (rc) return rc;
  hipLaunchKernelGGL(score_sum_kernel, dim3(2), dim3(256), 0, st, a->ws, k.nblk, a->scale, a->wsum, a->loss_out, a->ent_out);
  return addk_check_launch("score_upsample_sum");
}

extern "C" int addk_profile_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C, int32_t nthr) {
  return scu_ok(N, H, W, OH, OW, C) && nthr >= 0 && nthr <= PRU_NT ? 1 : 0;
}
extern "C" int64_t addk_profile_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  return up_ws_bytes(N, OH, OW, PRU_NT);
}
// the profile launch's arguments behind the UpSrc prefix (both of its forms)
static void profile_up_fill(ProfileUpK& k, const addk_profile_upsample_args* a) {
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.thr = a->thr; k.nthr = a->nthr;
  k.ent = a->ent_out; k.share = a->share_out; k.cm = reinterpret_cast<unsigned long long*>(a->cm); k.pred = a->pred_out;
  up_tail_fill(k, a->ws, a->N, a->OH, a->OW);
}
extern "C" int addk_profile_upsample(const addk_profile_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->ent_out && a->cm && a->ws, "profile_upsample: null pointer");
  ADDK_REQUIRE(addk_profile_upsample_supported(a->N, a->H, a->W, a->OH, a->OW, a->C, a->nthr) == 1,
               "profile_upsample: unsupported shape (%s, at most %d thresholds)", gate_classes_text().c_str(), PRU_NT);
  ADDK_REQUIRE(a->nthr == 0 || (a->thr && a->share_out), "profile_upsample: null pointer");
  ADDK_REQUIRE(a->ld >= a->C, "profile_upsample: short stride");
  ProfileUpK k;
  profile_up_fill(k, a);
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), profile_up_kernel<CC, true>, profile_up_kernel<CC, false>, scu_grid(a->N, a->OH, a->OW), st, k);
  });
  return addk_check_launch("profile_upsample");
}
extern "C" int addk_profile_upsample_t(const addk_profile_upsample_t_args* b, void* stream) {
  ADDK_REQUIRE(b, "profile_upsample_t: null pointer");
  const addk_profile_upsample_args* a = &b->profile;
  ADDK_REQUIRE(a->logits && a->target && a->ent_out && a->cm && a->ws && b->inv_temp, "profile_upsample_t: null pointer");
  ADDK_REQUIRE(addk_profile_upsample_supported(a->N, a->H, a->W, a->OH, a->OW, a->C, a->nthr) == 1,
               "profile_upsample_t: unsupported shape (%s, at most %d thresholds)", gate_classes_text().c_str(), PRU_NT);
  ADDK_REQUIRE(a->nthr == 0 || (a->thr && a->share_out), "profile_upsample_t: null pointer");
  ADDK_REQUIRE(a->ld >= a->C, "profile_upsample_t: short stride");
  ProfileUpTK k;
  profile_up_fill(k, a);
  k.inv_temp = b->inv_temp;
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), profile_up_kernel<CC, true, true>, profile_up_kernel<CC, false, true>, scu_grid(a->N, a->OH, a->OW), st, k);
  });
  return addk_check_launch("profile_upsample_t");
}
