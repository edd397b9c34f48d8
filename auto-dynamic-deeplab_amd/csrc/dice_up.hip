// The soft-Dice region term of the training head (addk_dice_stats): the per-class sums over the whole full-resolution batch that the term
// and its gradient need, straight from the decoder's low-resolution logits, and the coefficient table ce_up_kernel<..., DICE> (loss_up.hip)
// reads.  Semantics: include/addk.h.
//   dice_clear_kernel    zeroes the count table (32 words: one bin per class, CC <= 32): the launch sequence clears what it accumulates into.
//   dice_stats_kernel    the walk of scu_walk (the tile, grid and interpolation of ohem_loss_kernel): one softmax per valid pixel, I_c and
//                        P_c in registers (2*CC values), reduced over the workgroup (lanes by shuffle, the four waves in order) to one row
//                        of [blk][2*CC] fp32 partials; Y_c through an LDS histogram (run_count / run_flush) and 32-bit integer atomics.
//   dice_finish_kernel   ONE workgroup: thread t adds the partial rows t, t + 256, ... in fp64, then lanes, then the four waves in order
//                        (the order of up_finish); then D_c, A_c, B_c, m and the term in fp64, rounded once.
// Workspace (32-bit words): [0..CC-1] Y_c, [32..] I_c, [64..] P_c (left for inspection), from word 96 the partial rows, 2*CC words each.
// CC is the launch's class count (up.h: head_classes); the three tables hold up to 32 classes (static_assert below).
#include "up.h"

namespace {

constexpr int DICE_I = 32, DICE_P = 64, DICE_PART = 96;            // word offsets into the workspace
static_assert(HEAD_CMAX <= DICE_I && DICE_I + HEAD_CMAX <= DICE_P && DICE_P + HEAD_CMAX <= DICE_PART, "a class table of the dice workspace holds 32 classes");

__global__ void __launch_bounds__(64) dice_clear_kernel(unsigned* ws) {
  if (threadIdx.x < DICE_I) ((gu32*)ws)[threadIdx.x] = 0u;
}

struct DiceStatsK : UpSrc { const int64_t* target; int ignore; unsigned* hist; float* part; };

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) dice_stats_kernel(const DiceStatsK p) {
  __shared__ unsigned hist[32];
  __shared__ float red[SCU_WAVES][2 * CC];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 32) hist[t] = 0u;
  __syncthreads();
  const int64_t __attribute__((address_space(1)))* tgt = (const int64_t __attribute__((address_space(1)))*)p.target;
  float I[CC], P[CC];
#pragma unroll
  for (int c = 0; c < CC; ++c) { I[c] = 0.f; P[c] = 0.f; }
  int key = -1; unsigned run = 0;                                // pending run of equal classes of this column
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    const long tg = tgt[pix];
    const bool valid = tg != p.ignore && tg >= 0 && tg < CC;
    if (valid) {
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < CC; ++c) mx = fmaxf(mx, z[c]);
      float e[CC], se = 0.f;
#pragma unroll
      for (int c = 0; c < CC; ++c) { e[c] = __expf(z[c] - mx); se += e[c]; }
      const float rs = 1.f / se;
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        const float pc = e[c] * rs;
        P[c] += pc;
        I[c] += c == tg ? pc : 0.f;
      }
    }
    run_count(hist, key, run, valid ? (int)tg : -1);
  });
  run_flush(hist, key, run);
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    float a = I[c], b = P[c];
    for (int m = 32; m > 0; m >>= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); }
    if (lane == 0) { red[wv][c] = a; red[wv][CC + c] = b; }
  }
  __syncthreads();
  const long blk = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (t < 2 * CC) ((gfloat*)p.part)[blk * (2 * CC) + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (t < CC) {
    const unsigned v = hist[t];
    if (v) atomicAdd(&p.hist[t], v);
  }
}

template <int CC>
__global__ void __launch_bounds__(256) dice_finish_kernel(unsigned* ws, long nblk, float weight, float smooth, float scale,
                                                           float* coef, float* dice_out, float* loss_out) {
  __shared__ double shd[4][2 * CC];
  __shared__ double sD[CC];
  __shared__ int spres[CC];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const gfloat* part = (const gfloat*)((const float*)ws + DICE_PART);
  double s[2 * CC];
#pragma unroll
  for (int j = 0; j < 2 * CC; ++j) s[j] = 0.0;
  for (long i = t; i < nblk; i += 256) {
#pragma unroll
    for (int j = 0; j < 2 * CC; ++j) s[j] += (double)part[i * (2 * CC) + j];
  }
#pragma unroll
  for (int j = 0; j < 2 * CC; ++j) {
    double v = s[j];
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    if (lane == 0) shd[wv][j] = v;
  }
  __syncthreads();
  double Ic = 0.0, Pc = 0.0, den = 1.0;
  bool present = false;
  if (t < CC) {
    Ic = ((shd[0][t] + shd[1][t]) + shd[2][t]) + shd[3][t];
    Pc = ((shd[0][CC + t] + shd[1][CC + t]) + shd[2][CC + t]) + shd[3][CC + t];
    const unsigned Y = ((const gu32*)ws)[t];
    present = Y > 0u;
    den = Pc + (double)Y + (double)smooth;                        // Y >= 1 where it is used
    ((gfloat*)ws)[DICE_I + t] = (float)Ic;
    ((gfloat*)ws)[DICE_P + t] = (float)Pc;
    sD[t] = present ? (2.0 * Ic + (double)smooth) / den : 0.0;
    spres[t] = present ? 1 : 0;
  }
  __syncthreads();
  if (t < CC) {
    int m = 0;
    for (int c = 0; c < CC; ++c) m += spres[c];
    double A = 0.0, B = 0.0;
    if (present) {                                               // m >= 1 here
      const double k = (double)scale * (double)weight / (double)m;
      A = k * 2.0 / den;
      B = k * (2.0 * Ic + (double)smooth) / (den * den);
    }
    ((gfloat*)coef)[t] = (float)A;
    ((gfloat*)coef)[CC + t] = (float)B;
    ((gfloat*)dice_out)[1 + t] = present ? (float)sD[t] : -1.f;
    if (t == 0) {
      double sum = 0.0;
      for (int c = 0; c < CC; ++c) sum += sD[c];                 // absent classes hold 0
      const float dice = m > 0 ? (float)((double)scale * (double)weight * (1.0 - sum / (double)m)) : 0.f;
      ((gfloat*)dice_out)[0] = dice;
      *(gfloat*)loss_out += dice;
    }
  }
}

bool dice_ok(int N, int H, int W, int OH, int OW, int C) {
  return scu_head_ok(N, H, W, OH, OW, C) && (long)N * OH * OW < (1L << 31);
}

}  // namespace

extern "C" int addk_dice_stats_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return dice_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_dice_stats_ws_bytes_classes(int32_t N, int32_t OH, int32_t OW, int32_t C) {
  if (N <= 0 || OH <= 0 || OW <= 0 || !head_class_ok(C)) return 0;
  return 4 * ((int64_t)DICE_PART + 2 * C * (int64_t)scu_blocks(N, OH, OW));
}
// The query from before the class-count list: the FIRST count's size (19 classes) and no other.  A launch with more classes needs
// addk_dice_stats_ws_bytes_classes: its partial rows are 2 x C floats per workgroup, and addk_dice_stats cannot see how large ws is.
extern "C" int64_t addk_dice_stats_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  return addk_dice_stats_ws_bytes_classes(N, OH, OW, HeadClasses::v[0]);
}
extern "C" int addk_dice_stats(const addk_dice_stats_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->coef && a->dice_out && a->loss_out && a->ws, "dice_stats: null pointer");
  ADDK_REQUIRE(isfinite(a->weight) && a->weight > 0.f && isfinite(a->smooth) && a->smooth >= 0.f,
               "dice_stats: weight must be positive, smooth non-negative, both finite");
  ADDK_REQUIRE(a->ld >= a->C, "dice_stats: short stride");
  ADDK_REQUIRE(dice_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "dice_stats: unsupported shape (%s, fewer than 2^31 pixels)",
               head_classes_text().c_str());
  unsigned* w = (unsigned*)a->ws;
  DiceStatsK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.ignore = a->ignore_index; k.hist = w; k.part = (float*)(w + DICE_PART);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dice_clear_kernel, dim3(1), dim3(64), 0, st, w);
  head_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), dice_stats_kernel<CC, true>, dice_stats_kernel<CC, false>, scu_grid(a->N, a->OH, a->OW), st, k);
    hipLaunchKernelGGL(dice_finish_kernel<CC>, dim3(1), dim3(256), 0, st, w, scu_blocks(a->N, a->OH, a->OW), a->weight, a->smooth, a->scale,
                       a->coef, a->dice_out, a->loss_out);
  });
  return addk_check_launch("dice_stats");
}
