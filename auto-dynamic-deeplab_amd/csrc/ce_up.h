// The training head's kernel, ce_up_kernel, with what its launchers share: the argument structs of its forms, the index arithmetic of the
// gather and the shape check.  Two units instantiate it: loss_up.hip (the plain, mining, distillation and soft-Dice forms) and
// loss_shape.hip (the focal and label-smoothed forms).  Everything sits in the unit's anonymous namespace.
#pragma once
#include "up.h"

namespace {

// ---- fused logits up-sampling + cross-entropy, forward and backward (decoder.py:28 + train.py:70,231) -------------------
// The training step never needs the full-resolution logits: loss and gradient are computed straight from the low-resolution
// NHWC logits.  F.interpolate(mode='bilinear', align_corners=False) index arithmetic as in resize.hip (ATen's
// area_pixel_compute_source_index in fp32).  A high-resolution pixel (Y, X) reads the low-resolution rows h0(Y), h0+1 and
// columns w0(X), w0+1; it is OWNED by (h0, w0): thread (r, xl) of a block walks the pixels of row Y = first_row(h) + r whose
// w0 is its column, computes each pixel's softmax ONCE and accumulates the pixel's gradient into A0 (column w0) and A1
// (column w0 + 1).  A1 moves to the right neighbour lane, the 16 rows of the band are reduced through LDS in a fixed order
// with the row weights, and the part that belongs to row h + 1 is carried in registers to the next band: a gather with no
// atomics and no second pass over the 1.3 GB/exit of full-resolution logits and gradients the three-kernel form wrote and re-read.
// A block owns 31 output columns x HB output rows; it re-walks one band above (for the carry) and one column to the left
// (for A1): (HB+1)/HB * 32/31 redundant softmax work, counted once in the loss (own bands, xl >= 1).
//
struct CeUpK : UpSrc {
  const int64_t* target; const float* cw; int ignore;
  const float* wsum; float scale;
  float* g; int ldg; int accumulate;
  float* ws; int HB;
};

__host__ __device__ __forceinline__ int ce_idx0(int dst, float scale, int in) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  int i0 = (int)s;
  return i0 > in - 1 ? in - 1 : i0;
}
// smallest output index whose i0 is >= i (i0 is monotone in the output index)
__host__ __device__ __forceinline__ int ce_first_out(int i, float scale, int in, int out) {
  if (i <= 0) return 0;
  int g = (int)(((float)i + 0.5f) / scale - 0.5f);
  if (g < 0) g = 0;
  if (g > out) g = out;
  while (g > 0 && ce_idx0(g - 1, scale, in) >= i) --g;
  while (g < out && ce_idx0(g, scale, in) < i) ++g;
  return g;
}

constexpr int CEU_R = 8, CEU_X = 32;       // rows per pass / lanes per row (31 output columns + the left neighbour)
constexpr int CEU_MAXBAND = 16;            // high-resolution rows per low-resolution row the kernel takes (host check)

// OHEM (online hard example mining, addk_ce_upsample_ohem_fwd_bwd): the launch also gets the per-pixel loss map and the device word tau of
// addk_ohem_select; a pixel whose stored loss is below tau counts as not valid (weight 0), and p.wsum points at the kept weight sum.  The
// keep decision is READ, never recomputed: invalid pixels carry -1 in the map and tau >= 0.  OHEM = false is the plain kernel, token for token.
struct CeUpOhemK : CeUpK { const float* lmap; const float* tau; };
// KD (self-distillation from the last exit, addk_ce_upsample_kd_fwd_bwd): the launch also gets the teacher's low-resolution logits on the
// student's grid.  A thread keeps the teacher's four corner pixels beside the student's, samples z_t with the student's indices and
// expression, and per pixel adds one softmax pair at temperature T: e_s = exp(z_s/T - max), e_t likewise (1/T is rounded once on the
// host: z * rT), KL = (1/Σe_t) Σ e_t*(d_t - d_s) + log Σe_s - log Σe_t with d = z/T - max, and kg * (e_s/Σe_s - e_t/Σe_t) joins gz before the
// gather, kg = scale*alpha*T / n.  The plain predicate decides (a select, not a factor): mining never filters the term and class_w does not
// weigh it.  The KL partial leaves beside lsum (ws2, same ownership rule).  KD = false is the parent's kernel, instruction for instruction.
// TVEC: the teacher's loader, px_vec_ok on ITS base and stride, chosen by the host as for scu_walk — a second run-time loader switch
// would put the teacher's padding channels into scratch as the student's are (40 -> 72 bytes per lane).
struct CeUpKdK : CeUpOhemK { const float* teacher; int ldt; float rT, kscale; const float* nvalid; float* ws2; };
// DICE (the soft-Dice region term, addk_ce_upsample_dice_fwd_bwd): the launch also gets the coefficient table of addk_dice_stats (dice_up.hip),
// A_c then B_c, staged in LDS once per workgroup.  Per pixel, after the CE sweep has left e_c in z and Σe: rs = 1/Σe, one more sweep for
// dot = Σ_c p_c*G_c = rs*Σ_c e_c*B_c - p_t*A_t with p_c = e_c*rs and G_c = B_c - A_c*[t = c], B_c read from LDS (no G[] array), then the gather
// loop's gz gets p_j*(G_j - dot) under the plain predicate: mining never filters the term and class_w does not weigh it.  Every DICE form takes the widest struct; DICE = false is the
// parent's kernel, instruction for instruction.
struct CeUpDiceK : CeUpKdK { const float* coef; };
// SHAPE (the per-pixel loss shape, addk_ce_upsample_shaped_fwd_bwd; loss_shape.hip): what stands where the plain head has w_t * (-log p_t).
//   CE_FOCAL   w_t * (1 - p_t)^gamma * (-log p_t).  Its gradient is the plain one times F = (1 - p_t)^(gamma-1) * ((1 - p_t) + gamma * p_t * (-log p_t)),
//              so F multiplies the two per-pixel scalars k and kt and the gather loop is the plain one.  q = 1 - p_t is (Σ_{c != t} e_c) / Σe,
//              a sum of its own in the exp sweep: 1 - e_t/Σe has no bits left where the focal factor matters.  q^(gamma-1) = exp2((gamma-1) * log2 q);
//              gamma == 1 takes 1 (0^0 = 1), q == 0 with gamma > 1 gives exp2(-inf) = 0.
//   CE_SMOOTH  (1-eps) * w_t * (-log p_t) + (eps/C) * Σ_c w_c * (-log p_c): torch's cross_entropy(label_smoothing=eps).  Σ_c w_c * (-log p_c) =
//              W * (log Σe + max) - Σ_c w_c z_c with W = Σ_c w_c.  The gradient (1-eps) * w_t * (p_j - [j = t]) + (eps/C) * (p_j * W - w_j): the
//              first two parts change k and kt; the last is -w_j times a per-pixel scalar.  w_c comes from a per-workgroup LDS copy of the
//              class weights (ones where the launch has none), and both uses are linear, so the copy is read once per pass and never in
//              the pixel loop: Σ_c w_c z_c is sampled from the four corners' own sums, and the -w_j part is added to A0 / A1 behind the loop.
//              (Per-pixel reads, 2 x CC of them in flight beside the corners, cost 15 registers and the 21-class mining forms their
//              second wave.)
// Both keep the head's normaliser (p.wsum) and predicate, compose with OHEM and DICE, and have no KD form.  They take n == 0 (no valid
// pixel) as 1/n = 0: gradient 0, where the plain kernel leaves its own 0/0.  SHAPE = CE_PLAIN is the parent's kernel, instruction for instruction.
enum { CE_PLAIN = 0, CE_FOCAL = 1, CE_SMOOTH = 2 };
struct CeUpShapeK : CeUpDiceK { float gamma, eps; };
template <bool OHEM, bool KD = false, bool DICE = false, int SHAPE = CE_PLAIN> struct CeUpArg { typedef CeUpK type; };
template <> struct CeUpArg<true, false, false> { typedef CeUpOhemK type; };
template <bool OHEM> struct CeUpArg<OHEM, true, false> { typedef CeUpKdK type; };
template <bool OHEM, bool KD> struct CeUpArg<OHEM, KD, true> { typedef CeUpDiceK type; };
template <bool OHEM, bool KD, bool DICE> struct CeUpArg<OHEM, KD, DICE, CE_FOCAL> { typedef CeUpShapeK type; };
template <bool OHEM, bool KD, bool DICE> struct CeUpArg<OHEM, KD, DICE, CE_SMOOTH> { typedef CeUpShapeK type; };
template <int CC> __device__ __forceinline__ float* dice_coef_lds() { __shared__ float s[2 * CC]; return s; }
template <int CC> __device__ __forceinline__ float* smooth_w_lds() { __shared__ float s[CC]; return s; }
// An index offset of 0 the compiler cannot see through: a sweep that adds it to its table index READS the table where it uses it.  Plain
// reads are loop-invariant and the compiler keeps all CC B_c in registers across the pixel loop (the G[] array in another place): the plain
// form then needs 257 registers and drops to one wave per SIMD.  (No `valid ? f(B_c) : 0` per class either: the compiler turns a select
// whose operand hangs on a load into a branch around that load, CC branches and CC exposed LDS latencies per pixel.)
__device__ __forceinline__ int opaque_zero() { int o = 0; asm volatile("" : "+v"(o)); return o; }
// a value every lane of the wave holds, moved to a scalar register: W of the smooth form, which every lane adds up from LDS (values
// computed from kernel arguments are uniform to the compiler already)
__device__ __forceinline__ float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <int CC, bool OHEM = false, bool KD = false, bool TVEC = false, bool DICE = false, int SHAPE = CE_PLAIN>
__global__ void __launch_bounds__(256) ce_up_kernel(const typename CeUpArg<OHEM, KD, DICE, SHAPE>::type p) {
  static_assert(SHAPE == CE_PLAIN || !KD, "the shaped heads have no distillation form");
  constexpr int CP = cpad(CC);
  constexpr int NOUT = ((CEU_X - 1) * CC + 255) / 256;
  __shared__ float S0[CEU_R * CEU_X * CC], S1[CEU_R * CEU_X * CC];
  __shared__ float shs[4];
  const int t = threadIdx.x, xl = t & (CEU_X - 1), r = t / CEU_X;
  const int tx0 = blockIdx.x * (CEU_X - 1), hb = blockIdx.y * p.HB, n = blockIdx.z;
  const int x = tx0 - 1 + xl;                                   // the low-resolution column this thread owns as w0
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  float inv = p.scale / *(const gfloat*)p.wsum;
  if constexpr (SHAPE != CE_PLAIN) inv = *(const gfloat*)p.wsum > 0.f ? inv : 0.f;
  int xlo = 0, xhi = 0;
  if (x >= 0 && x < p.W) { xlo = ce_first_out(x, sw, p.W, p.OW); xhi = (x + 1 < p.W) ? ce_first_out(x + 1, sw, p.W, p.OW) : p.OW; }
  const bool xlast = x == p.W - 1;
  const int x1 = x + (x < p.W - 1 ? 1 : 0);
  const bool vec = (p.ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.x) & 15) == 0) && p.ld >= CP;      // px_vec_ok
  const int64_t __attribute__((address_space(1)))* tgt = (const int64_t __attribute__((address_space(1)))*)p.target;
  const gfloat* cw = (const gfloat*)p.cw;
  float tau = 0.f;
  if constexpr (OHEM) tau = *(const gfloat*)p.tau;
  [[maybe_unused]] float kg = 0.f, ksum = 0.f;
  if constexpr (KD) {
    kg = p.kscale / *(const gfloat*)p.nvalid;                  // n == 0: no pixel is valid and the select below never takes it
  }
  [[maybe_unused]] const float* sco = nullptr;              // A_c at [c], B_c at [CC + c]
  if constexpr (DICE) {
    float* stage = dice_coef_lds<CC>();
    if (t < 2 * CC) stage[t] = ((const gfloat*)p.coef)[t];
    sco = stage;
    __syncthreads();
  }
  [[maybe_unused]] const float* swl = nullptr;              // w_c, or 1
  [[maybe_unused]] float gm1 = 0.f, sW = 0.f, se1 = 0.f, sc = 0.f;
  if constexpr (SHAPE == CE_FOCAL) gm1 = p.gamma - 1.f;
  if constexpr (SHAPE == CE_SMOOTH) {
    float* stage = smooth_w_lds<CC>();
    if (t < CC) stage[t] = cw ? cw[t] : 1.f;
    swl = stage;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CC; ++c) sW += stage[c];               // W, every thread in class order
    sW = wave_uniform(sW); se1 = 1.f - p.eps; sc = p.eps / (float)CC;
  }
  float lsum = 0.f;
  float carry[NOUT];
#pragma unroll
  for (int k = 0; k < NOUT; ++k) carry[k] = 0.f;
  const int hstart = hb > 0 ? hb - 1 : 0;
  const int hend = hb + p.HB < p.H ? hb + p.HB : p.H;
  for (int h = hstart; h < hend; ++h) {
    const int ylo = ce_first_out(h, sh, p.H, p.OH);
    const int yhi = (h + 1 < p.H) ? ce_first_out(h + 1, sh, p.H, p.OH) : p.OH;
    const bool own = h >= hb;
    float b0[NOUT], b1[NOUT];
#pragma unroll
    for (int k = 0; k < NOUT; ++k) { b0[k] = 0.f; b1[k] = 0.f; }
    for (int yb = ylo; yb < yhi; yb += CEU_R) {                 // the band in passes of CEU_R rows (one pass at the x8 of config 2)
      const int Y = yb + r;
      float A0[CC], A1[CC];
#pragma unroll
      for (int c = 0; c < CC; ++c) { A0[c] = 0.f; A1[c] = 0.f; }
      float lh0 = 0.f, lh1 = 0.f;
      if (Y < yhi && xhi > xlo) {
        int h0, h1;
        src_index(Y, sh, p.H, h0, h1, lh0, lh1);
        const float* r0 = p.x + ((long)(n * p.H + h0) * p.W) * p.ld;
        const float* r1 = p.x + ((long)(n * p.H + h1) * p.W) * p.ld;
        float v00[CP], v01[CP], v10[CP], v11[CP];
        load_px<CC>(r0 + (long)x * p.ld, v00, vec); load_px<CC>(r0 + (long)x1 * p.ld, v01, vec);
        load_px<CC>(r1 + (long)x * p.ld, v10, vec); load_px<CC>(r1 + (long)x1 * p.ld, v11, vec);
        [[maybe_unused]] float u00[KD ? CP : 1], u01[KD ? CP : 1], u10[KD ? CP : 1], u11[KD ? CP : 1];      // the teacher's corners
        if constexpr (KD) {
          const float* q0 = p.teacher + ((long)(n * p.H + h0) * p.W) * p.ldt;
          const float* q1 = p.teacher + ((long)(n * p.H + h1) * p.W) * p.ldt;
          load_px<CC>(q0 + (long)x * p.ldt, u00, TVEC); load_px<CC>(q0 + (long)x1 * p.ldt, u01, TVEC);
          load_px<CC>(q1 + (long)x * p.ldt, u10, TVEC); load_px<CC>(q1 + (long)x1 * p.ldt, u11, TVEC);
        }
        // CE_SMOOTH, both by linearity and once per pass, not per pixel: Σ_c w_c z_c is the bilinear sample of the corners' own Σ_c w_c v_c
        // (s00 ... s11), and the gradient's -ksw * w_j leaves the pixel loop as T0 = Σ a0 * ksw, T1 = Σ a1 * ksw, times w_j behind it
        [[maybe_unused]] float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f, T0 = 0.f, T1 = 0.f;
        if constexpr (SHAPE == CE_SMOOTH) {
          const float* wl = swl + opaque_zero();
#pragma unroll
          for (int c = 0; c < CC; ++c) {
            const float wc = wl[c];
            s00 = fmaf(wc, v00[c], s00); s01 = fmaf(wc, v01[c], s01); s10 = fmaf(wc, v10[c], s10); s11 = fmaf(wc, v11[c], s11);
          }
        }
        const int64_t __attribute__((address_space(1)))* tp = tgt + ((long)n * p.OH + Y) * p.OW;
        for (int X = xlo; X < xhi; ++X) {
          int w0, w1; float lw0, lw1;
          src_index(X, sw, p.W, w0, w1, lw0, lw1);
          const long tg = tp[X];
          bool valid = tg != p.ignore && tg >= 0 && tg < CC;
          [[maybe_unused]] const bool pvalid = valid;            // the plain predicate: what the distillation term goes by
          if constexpr (OHEM) valid = valid && ((const gfloat*)p.lmap)[((long)n * p.OH + Y) * p.OW + X] >= tau;
          const float w = valid ? (cw ? cw[tg] : 1.f) : 0.f;
          float z[CC];
          float mx = -INFINITY, zt = 0.f;
#pragma unroll
          for (int c = 0; c < CC; ++c) {
            z[c] = lh0 * (lw0 * v00[c] + lw1 * v01[c]) + lh1 * (lw0 * v10[c] + lw1 * v11[c]);
            mx = fmaxf(mx, z[c]);
            if (c == tg) zt = z[c];
          }
          [[maybe_unused]] float D[KD ? CC : 1];                 // the distillation term's part of gz
          if constexpr (KD) {
            float et[CC];
            float mt = -INFINITY;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
              et[c] = (lh0 * (lw0 * u00[c] + lw1 * u01[c]) + lh1 * (lw0 * u10[c] + lw1 * u11[c])) * p.rT;
              mt = fmaxf(mt, et[c]);
            }
            const float ms = mx * p.rT;                           // rT > 0: the largest z * rT is (largest z) * rT
            float ses = 0.f, set = 0.f, kl = 0.f;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
              const float ds = z[c] * p.rT - ms, dt = et[c] - mt;
              const float es = __expf(ds), e = __expf(dt);
              ses += es; set += e;
              kl = fmaf(e, dt - ds, kl);
              D[c] = es; et[c] = e;
            }
            if (own && xl >= 1 && pvalid) ksum += kl / set + (logf(ses) - logf(set));
            const float ks = kg / ses, kt_ = kg / set;
#pragma unroll
            for (int c = 0; c < CC; ++c) D[c] = pvalid ? D[c] * ks - et[c] * kt_ : 0.f;
          }
          float se = 0.f;
          [[maybe_unused]] float so = 0.f;                       // Σ_{c != t} e_c
#pragma unroll
          for (int c = 0; c < CC; ++c) {
            z[c] = __expf(z[c] - mx); se += z[c];
            if constexpr (SHAPE == CE_FOCAL) so += c == tg ? 0.f : z[c];
          }
          [[maybe_unused]] float ksw = 0.f;                      // the smoothing part's coefficient of w_j
          float k, kt;
          if constexpr (SHAPE == CE_FOCAL) {
            // e_t once more from the bits of z[t], as the Dice sweep takes it; not valid: zt is no logit and exp(-max) may not be finite
            const float nll = logf(se) + mx - zt, q = so / se, pt = pvalid ? __expf(zt - mx) / se : 0.f;
            const float pw = gm1 == 0.f ? 1.f : exp2f(gm1 * log2f(q));
            if (own && xl >= 1 && valid) lsum += w * (pw * q * nll);
            const float wF = w * (pw * (q + p.gamma * pt * nll));
            k = wF * inv / se; kt = wF * inv;
          } else if constexpr (SHAPE == CE_SMOOTH) {
            const float lse = logf(se) + mx;
            const float swz = lh0 * (lw0 * s00 + lw1 * s01) + lh1 * (lw0 * s10 + lw1 * s11);      // Σ_c w_c z_c
            if (own && xl >= 1 && valid) lsum += se1 * w * (lse - zt) + sc * (sW * lse - swz);
            k = (valid ? se1 * w + sc * sW : 0.f) * inv / se; kt = se1 * w * inv;
            ksw = valid ? sc * inv : 0.f;
          } else {
            if (own && xl >= 1 && valid) lsum += w * (logf(se) + mx - zt);
            k = w * inv / se; kt = w * inv;
          }
          const float a0 = lw0 + (xlast ? lw1 : 0.f), a1 = xlast ? 0.f : lw1;
          // G_c = B_c - A_c*[t = c]: the sweeps take B_c from LDS, and the target's own p_t*A_t (e_t once more: the bits of z[t]) apart.
          // valid ? ... : 0 is a select on two per-pixel values, rsd and p_t*A_t; the gather loop then has the parent's select, on c == t
          [[maybe_unused]] float rsd = 0.f, ktp = 0.f, dot = 0.f;
          if constexpr (DICE) {
            const float rs = 1.f / se;
            const float* B = sco + CC + opaque_zero();
#pragma unroll
            for (int c = 0; c < CC; ++c) dot = fmaf(z[c], B[c], dot);
            const float ptA = pvalid ? (__expf(zt - mx) * rs) * sco[pvalid ? (int)tg : 0] : 0.f;
            dot = dot * rs - ptA;                               // Σ_c p_c*G_c
            rsd = pvalid ? rs : 0.f;
            ktp = (valid ? kt : 0.f) + ptA;
          }
          [[maybe_unused]] const float* B = DICE ? sco + CC + opaque_zero() : nullptr;
          if constexpr (SHAPE == CE_SMOOTH) { T0 = fmaf(a0, ksw, T0); T1 = fmaf(a1, ksw, T1); }
#pragma unroll
          for (int c = 0; c < CC; ++c) {
            float gz;
            if constexpr (DICE) gz = z[c] * fmaf(B[c] - dot, rsd, k) - (c == tg ? ktp : 0.f);     // e_c*(k + (B_c - dot)/Σe) - [t = c]*(kt + p_t*A_t)
            else gz = z[c] * k - ((valid && c == tg) ? kt : 0.f);
            if constexpr (KD) gz += D[c];
            A0[c] = fmaf(a0, gz, A0[c]); A1[c] = fmaf(a1, gz, A1[c]);
          }
        }
        if constexpr (SHAPE == CE_SMOOTH) {
          const float* wl = swl + opaque_zero();
#pragma unroll
          for (int c = 0; c < CC; ++c) {
            const float wc = wl[c];
            A0[c] = fmaf(-T0, wc, A0[c]); A1[c] = fmaf(-T1, wc, A1[c]);
          }
        }
      }
      // column w0 + 1 belongs to the right neighbour lane; then the rows of the pass go through LDS
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        float fromleft = __shfl_up(A1[c], 1, CEU_X);
        if (xl == 0) fromleft = 0.f;
        const float R = A0[c] + fromleft;
        S0[(r * CEU_X + xl) * CC + c] = lh0 * R;
        S1[(r * CEU_X + xl) * CC + c] = lh1 * R;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NOUT; ++k) {
        const int j = t + 256 * k;
        if (j < (CEU_X - 1) * CC) {
          const int off = CC + j;                               // (ox = 1 + j / CC, c = j % CC) -> ox * CC + c
#pragma unroll
          for (int rr = 0; rr < CEU_R; ++rr) { b0[k] += S0[rr * CEU_X * CC + off]; b1[k] += S1[rr * CEU_X * CC + off]; }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
      const int j = t + 256 * k;
      if (j < (CEU_X - 1) * CC) {
        const int ox = 1 + j / CC, c = j - (ox - 1) * CC;
        if (h == p.H - 1) { b0[k] += b1[k]; b1[k] = 0.f; }
        const float o = carry[k] + b0[k];
        carry[k] = b1[k];
        const int col = tx0 - 1 + ox;
        if (own && col < p.W) {
          gfloat* gp = (gfloat*)p.g + ((long)(n * p.H + h) * p.W + col) * p.ldg + c;
          *gp = p.accumulate ? *gp + o : o;
        }
      }
    }
  }
  lsum = block_sum(lsum, shs);
  if (t == 0) ((gfloat*)p.ws)[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = lsum;
  if constexpr (KD) {
    ksum = block_sum(ksum, shs);
    if (t == 0) ((gfloat*)p.ws2)[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ksum;
  }
}

int ceu_hb(int H) { return H >= 64 ? 4 : (H >= 16 ? 2 : 1); }
bool ceu_ok(int N, int H, int W, int OH, int OW, int C) {
  if (!head_class_ok(C) || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return false;
  const float sh = (float)H / (float)OH;
  for (int h = 0; h < H; ++h) {
    const int lo = ce_first_out(h, sh, H, OH), hi = h + 1 < H ? ce_first_out(h + 1, sh, H, OH) : OH;
    if (hi - lo > CEU_MAXBAND) return false;
  }
  return true;
}
// The kernel's arguments from the C ABI's block, every form: the plain head's fields, the kept set (both NULL: none), the launch grid
template <class K> dim3 ceu_fill(K& k, const addk_ce_upsample_args* a, const float* lmap, const float* tau) {
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.cw = a->class_w; k.ignore = a->ignore_index; k.wsum = a->wsum; k.scale = a->scale;
  k.g = a->g; k.ldg = a->ldg; k.accumulate = a->accumulate; k.ws = a->ws; k.HB = ceu_hb(a->H);
  k.lmap = lmap; k.tau = tau;
  return dim3(cdiv(a->W, CEU_X - 1), cdiv(a->H, k.HB), a->N);
}

}  // namespace
