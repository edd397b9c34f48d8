// Softmax cross-entropy on NCHW logits (nn.CrossEntropyLoss(weight, ignore_index=255), train.py:70,231),
// normalised Shannon entropy of the prediction (operations.py:161-170), argmax and the confusion matrix
// of the evaluator (utils/metrics.py:34-43), the entropy / top-probability gates of dynamic inference
// (operations.py:161-180) and the per-image exit profile (eval.py:195-230) from the low-resolution logits.  One thread per pixel; channel planes are contiguous along
// W so every per-channel access of a wave is one coalesced 256-B segment.
#include <math.h>
#include "common.h"
#include "bnfin.h"

namespace {


__device__ __forceinline__ float block_sum(float v, float* sh) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
  return s;
}

__global__ void __launch_bounds__(256) ce_count_kernel(const int64_t* target, long n, const float* cw, int ignore, int nc, float* ws) {
  __shared__ float sh[4];
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    long t = target[i];
    if (t != ignore && t >= 0 && t < nc) s += cw ? cw[t] : 1.f;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) sum_partials_kernel(const float* ws, int n, float scale, const float* denom, float* out, int accumulate) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += ws[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    float v = s * scale;
    if (denom) v /= *denom;
    *out = accumulate ? *out + v : v;
  }
}

// CC > 0: class count known at compile time, logits of a pixel live in registers (19 = Cityscapes);
// CC == 0: generic fallback that re-reads the (cache-resident) logits instead of indexing a register array.
template <int CC>
__global__ void __launch_bounds__(256) ce_kernel(const float* logits, const int64_t* target, int N, int C, long HW, const float* cw,
                                                int ignore, const float* wsum, float scale, float* dlogits, float* ws) {
  __shared__ float sh[4];
  const long total = (long)N * HW;
  const float inv = scale / *wsum;
  float lsum = 0.f;
  for (long pp = (long)blockIdx.x * 256 + threadIdx.x; pp < total; pp += (long)gridDim.x * 256) {
    int n = (int)(pp / HW); long i = pp - (long)n * HW;
    const float* lp = logits + (long)n * C * HW + i;
    long t = target[pp];
    const bool valid = t != ignore && t >= 0 && t < C;
    const float w = valid ? (cw ? cw[t] : 1.f) : 0.f;
    float* dp = dlogits ? dlogits + (long)n * C * HW + i : nullptr;
    if (CC > 0) {
      float v[CC > 0 ? CC : 1];
      float mx = -INFINITY, lt = 0.f;
#pragma unroll
      for (int c = 0; c < CC; ++c) { v[c] = lp[(long)c * HW]; mx = fmaxf(mx, v[c]); if (c == t) lt = v[c]; }
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < CC; ++c) { v[c] = expf(v[c] - mx); se += v[c]; }
      if (valid) lsum += w * (logf(se) + mx - lt);
      if (dp) {
        float k = w * inv / se;
#pragma unroll
        for (int c = 0; c < CC; ++c) dp[(long)c * HW] = v[c] * k - ((valid && c == t) ? w * inv : 0.f);
      }
    } else {
      float mx = -INFINITY;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, lp[(long)c * HW]);
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(lp[(long)c * HW] - mx);
      if (valid) lsum += w * (logf(se) + mx - lp[t * HW]);
      if (dp) {
        float k = w * inv / se;
        for (int c = 0; c < C; ++c) dp[(long)c * HW] = expf(lp[(long)c * HW] - mx) * k - ((valid && c == t) ? w * inv : 0.f);
      }
    }
  }
  lsum = block_sum(lsum, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = lsum;
}

__global__ void __launch_bounds__(256) entropy_kernel(const float* logits, int N, int C, long HW, float* ws) {
  __shared__ float sh[4];
  const long total = (long)N * HW;
  float s = 0.f;
  for (long pp = (long)blockIdx.x * 256 + threadIdx.x; pp < total; pp += (long)gridDim.x * 256) {
    int n = (int)(pp / HW); long i = pp - (long)n * HW;
    const float* lp = logits + (long)n * C * HW + i;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lp[(long)c * HW]);
    float se = 0.f, sx = 0.f;
    for (int c = 0; c < C; ++c) { float d = lp[(long)c * HW] - mx; float e = expf(d); se += e; sx += e * d; }
    // -sum p log p = log(se) - sx/se
    s += logf(se) - sx / se;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ void argmax_kernel(const float* logits, int N, int C, long HW, int64_t* out) {
  const long total = (long)N * HW;
  for (long pp = (long)blockIdx.x * blockDim.x + threadIdx.x; pp < total; pp += (long)gridDim.x * blockDim.x) {
    int n = (int)(pp / HW); long i = pp - (long)n * HW;
    const float* lp = logits + (long)n * C * HW + i;
    float best = lp[0]; int bi = 0;
    for (int c = 1; c < C; ++c) { float v = lp[(long)c * HW]; if (v > best) { best = v; bi = c; } }
    out[pp] = bi;
  }
}

__global__ void confusion_kernel(const int64_t* gt, const int64_t* pred, long n, int nc, unsigned long long* cm) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    long g = gt[i], p = pred[i];
    if (g >= 0 && g < nc && p >= 0 && p < nc) atomicAdd(&cm[g * nc + p], 1ULL);
  }
}


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
// What the three heads on the low-resolution logits share (this one, the scoring head and the exit gate below): the argument prefix
// UpSrc, the pixel loader load_px and its vector-load predicate px_vec_ok; the two gather heads also share their walk, scu_walk.
struct UpSrc { const float* x; int ld; int N, H, W, OH, OW; };      // NHWC logits, pixel stride ld, (H, W) -> (OH, OW)
template <class A> UpSrc up_src(const A* a) { return UpSrc{a->logits, a->ld, a->N, a->H, a->W, a->OH, a->OW}; }

constexpr int cpad(int cc) { return (cc + 3) / 4 * 4; }              // channels incl. the padding of a 16-byte-aligned pixel row
// 16-byte loads of a pixel's cpad(CC) channels: stride and base keep every pixel aligned and the padding exists.  The host's
// choice of a VEC kernel; ce_up_kernel evaluates the same three terms on the device
template <int CC> bool px_vec_ok(const float* x, int ld) { return ld % 4 == 0 && ld >= cpad(CC) && aligned16(x); }
// vec is a run-time value in ce_up_kernel and a compile-time constant in scu_walk, where the other branch folds away
template <int CC>
__device__ __forceinline__ void load_px(const float* q, float (&v)[cpad(CC)], bool vec) {
  if (vec) {
#pragma unroll
    for (int c = 0; c < cpad(CC); c += 4) { const float4 f = ld4(q + c); v[c] = f.x; v[c + 1] = f.y; v[c + 2] = f.z; v[c + 3] = f.w; }
  } else {
#pragma unroll
    for (int c = 0; c < CC; ++c) v[c] = ((const gfloat*)q)[c];
  }
}

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
template <bool OHEM, bool KD = false> struct CeUpArg { typedef CeUpK type; };
template <> struct CeUpArg<true, false> { typedef CeUpOhemK type; };
template <bool OHEM> struct CeUpArg<OHEM, true> { typedef CeUpKdK type; };

template <int CC, bool OHEM = false, bool KD = false, bool TVEC = false>
__global__ void __launch_bounds__(256) ce_up_kernel(const typename CeUpArg<OHEM, KD>::type p) {
  constexpr int CP = cpad(CC);
  constexpr int NOUT = ((CEU_X - 1) * CC + 255) / 256;
  __shared__ float S0[CEU_R * CEU_X * CC], S1[CEU_R * CEU_X * CC];
  __shared__ float shs[4];
  const int t = threadIdx.x, xl = t & (CEU_X - 1), r = t / CEU_X;
  const int tx0 = blockIdx.x * (CEU_X - 1), hb = blockIdx.y * p.HB, n = blockIdx.z;
  const int x = tx0 - 1 + xl;                                   // the low-resolution column this thread owns as w0
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  const float inv = p.scale / *(const gfloat*)p.wsum;
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
#pragma unroll
          for (int c = 0; c < CC; ++c) { z[c] = __expf(z[c] - mx); se += z[c]; }
          if (own && xl >= 1 && valid) lsum += w * (logf(se) + mx - zt);
          const float k = w * inv / se, kt = w * inv;
          const float a0 = lw0 + (xlast ? lw1 : 0.f), a1 = xlast ? 0.f : lw1;
#pragma unroll
          for (int c = 0; c < CC; ++c) {
            float gz = z[c] * k - ((valid && c == tg) ? kt : 0.f);
            if constexpr (KD) gz += D[c];
            A0[c] = fmaf(a0, gz, A0[c]); A1[c] = fmaf(a1, gz, A1[c]);
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

int ceu_hb(int H) { return H >= 64 ? 4 : (H >= 16 ? 2 : 1); }
bool ceu_ok(int N, int H, int W, int OH, int OW, int C) {
  if (C != 19 || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return false;
  const float sh = (float)H / (float)OH;
  for (int h = 0; h < H; ++h) {
    const int lo = ce_first_out(h, sh, H, OH), hi = h + 1 < H ? ce_first_out(h + 1, sh, H, OH) : OH;
    if (hi - lo > CEU_MAXBAND) return false;
  }
  return true;
}

// ---- fused logits up-sampling + scoring of a validation pass (decoder.py:28 + train.py:268-285) --------------------------
// Confusion matrix, loss and entropy of one exit from the low-resolution NHWC logits, as a GATHER: a wave owns 64 consecutive
// columns X of the high-resolution grid and walks SCU_R rows; a thread keeps the two W-interpolated rows t0 = lw0*v(h0,w0) +
// lw1*v(h0,w1), t1 = (same on h1) of its column in registers and reloads them only when the (wave-uniform) pair (h0, h1)
// changes, so at the x8 of config 2 the four neighbours are read once per 8 pixels and a pixel costs 19 x 3 flops of
// interpolation — z = lh0*t0 + lh1*t1 is the expression of resize_fwd_nchw_kernel / ce_up_kernel, operation for operation.
// One max/arg-max sweep, one exp sweep (Σe, Σe·d) serves loss and entropy.  HBM traffic: the target (coalesced 512 B per wave
// row) and the optional uint8 map; the logits (5 MB at config 2) stay in L2.  Counts go to a 361-entry LDS histogram (a thread
// merges the run of equal (gt, pred) keys of its column first), flushed once per workgroup with 64-bit integer atomics:
// order-independent, exact.  Loss and entropy leave the workgroup as two partials reduced in a fixed order.
constexpr int SCU_W = 64, SCU_WAVES = 4, SCU_R = 8;      // tile: 64 columns x (4 waves x 8 rows)

// The walk of a thread: its column X of the tile, SCU_R rows; pixel(pix, z) gets the flat index of each high-resolution pixel
// and its CC interpolated logits.  VEC: the loader's 16-byte form (host check px_vec_ok); a compile-time switch, so that no
// register array crosses a branch merge (the run-time form of ce_up_kernel keeps 40 bytes of scratch per lane for it)
template <int CC, bool VEC, class F>
__device__ __forceinline__ void scu_walk(const UpSrc& p, F&& pixel) {
  const int lane = threadIdx.x & (SCU_W - 1), wv = threadIdx.x / SCU_W;
  const int X = blockIdx.x * SCU_W + lane, n = blockIdx.z;
  if (X >= p.OW) return;
  const int ybeg = (blockIdx.y * SCU_WAVES + wv) * SCU_R;
  const int yend = ybeg + SCU_R < p.OH ? ybeg + SCU_R : p.OH;
  const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;
  int w0, w1; float lw0, lw1;
  src_index(X, sw, p.W, w0, w1, lw0, lw1);
  float t0[CC], t1[CC];
  int ph0 = -1, ph1 = -1;
  for (int Y = ybeg; Y < yend; ++Y) {
    int h0, h1; float lh0, lh1;
    src_index(Y, sh, p.H, h0, h1, lh0, lh1);
    if (h0 != ph0 || h1 != ph1) {                                // wave-uniform: Y is
      const float* r0 = p.x + ((long)(n * p.H + h0) * p.W) * p.ld;
      const float* r1 = p.x + ((long)(n * p.H + h1) * p.W) * p.ld;
      float a[cpad(CC)], b[cpad(CC)];
      load_px<CC>(r0 + (long)w0 * p.ld, a, VEC); load_px<CC>(r0 + (long)w1 * p.ld, b, VEC);
#pragma unroll
      for (int c = 0; c < CC; ++c) t0[c] = lw0 * a[c] + lw1 * b[c];
      load_px<CC>(r1 + (long)w0 * p.ld, a, VEC); load_px<CC>(r1 + (long)w1 * p.ld, b, VEC);
#pragma unroll
      for (int c = 0; c < CC; ++c) t1[c] = lw0 * a[c] + lw1 * b[c];
      ph0 = h0; ph1 = h1;
    }
    float z[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) z[c] = lh0 * t0[c] + lh1 * t1[c];
    pixel(((long)n * p.OH + Y) * p.OW + X, z);
  }
}
// se = Σe, sx = Σe·d over d = z - mx, e = exp(d): loss (log se) and entropy (log se - sx/se) of a pixel from one sweep
template <int CC>
__device__ __forceinline__ void exp_sweep(const float (&z)[CC], float mx, float& se, float& sx) {
  se = 0.f; sx = 0.f;
#pragma unroll
  for (int c = 0; c < CC; ++c) { const float d = z[c] - mx; const float e = __expf(d); se += e; sx += e * d; }
}

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
    if (k != key) {
      if (key >= 0) atomicAdd(&hist[key], run);
      key = k; run = 0;
    }
    ++run;
  });
  if (key >= 0) atomicAdd(&hist[key], run);
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

// the launch grid of the two gather heads (one workgroup per tile and image) and its workgroup count, which sizes their workspaces
dim3 scu_grid(int N, int OH, int OW) { return dim3(cdiv(OW, SCU_W), cdiv(OH, SCU_WAVES * SCU_R), N); }
long scu_blocks(int N, int OH, int OW) { const dim3 g = scu_grid(N, OH, OW); return (long)(int)g.z * (int)g.y * (int)g.x; }
bool scu_ok(int N, int H, int W, int OH, int OW, int C) {
  if (C != 19 || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return false;
  return N <= 65535 && scu_grid(N, OH, OW).y <= 65535 && scu_blocks(N, OH, OW) < (1L << 30);
}

// ---- fused logits up-sampling + label map (decoder.py:28 + eval.py:218-221) ------------------------------------------------------
// What inference keeps of an exit: the arg-max of the up-sampled logits, one byte per high-resolution pixel.  The walk is scu_walk
// (same tile, same interpolation), then the strict `>` arg-max sweep of score_up_kernel (a tie keeps the lowest channel) and one
// byte store — the class index, or lut[class] (train id -> Cityscapes labelId).  No exp, no LDS, no workspace; a wave row stores 64
// consecutive bytes.  label_px is also the store of the gate launch that leaves the map (gate_up_kernel<.., LABELS = true>).
typedef __attribute__((address_space(1))) uint8_t gu8;
__device__ __forceinline__ void label_px(const uint8_t* lut, uint8_t* labels, long pix, int am) {
  ((gu8*)labels)[pix] = lut ? ((const gu8*)lut)[am] : (uint8_t)am;
}

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
  if (nview < 1 || nview > ADDK_MAX_VIEWS || C != 19 || N <= 0 || OH <= 0 || OW <= 0) return false;
  const dim3 g = lvu_grid(N, OH, OW);
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
  double npix, ent_div;                                    // OH*OW and log(C) * OH*OW
};

// What a workgroup of a gate-style head does after its walk, shared by gate_up_kernel (NK = 1) and profile_up_kernel (NK = 16): its
// entropy partial (block_sum) and its first nk of NK pixel counts (wave shuffle, then LDS) leave write-through to part[blk] and
// cnt[blk * NK + j]; the workgroup that takes the LAST ticket adds each image's partials in a FIXED order — thread t the partials
// t, t + 256, ... in fp64, then lanes, then the four waves in order; the counts are integers — and calls write(img, es, ks) from thread 0;
// it then puts the ticket back to zero, after a system-scope fence when the writer stored to host memory.
template <int NK, class Wr>
__device__ __forceinline__ void up_finish(float esum, const unsigned (&hit)[NK], int nk, unsigned* counter, float* part, unsigned* cnt,
                                          int N, int nblk_img, bool host_fence, Wr&& write) {
  __shared__ float shs[4];
  __shared__ unsigned shc[4 * NK];
  __shared__ double shd[4];
  __shared__ unsigned long long shl[4 * NK];
  __shared__ unsigned flag;
  const int t = threadIdx.x, lane = t & (SCU_W - 1), wv = t / SCU_W;
  esum = block_sum(esum, shs);
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    if (j < nk) {
      unsigned h = hit[j];
      for (int m = 32; m > 0; m >>= 1) h += __shfl_xor(h, m);
      if (lane == 0) shc[wv * NK + j] = h;
    }
  }
  __syncthreads();
  const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (t == 0) __hip_atomic_store((gu32*)(part + blk), __float_as_uint(esum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t < nk)
    __hip_atomic_store((gu32*)(cnt + (long)blk * NK + t), shc[t] + shc[NK + t] + shc[2 * NK + t] + shc[3 * NK + t], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  if (!bnfin_arrive(counter, gridDim.x * gridDim.y * gridDim.z, &flag)) return;
  // ---- the last workgroup: thread t adds partials t, t + 256, ... of an image, then lanes and waves in a fixed order ----
  for (int img = 0; img < N; ++img) {
    double s = 0.0; unsigned long long k[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) k[j] = 0ull;
    const long base = (long)img * nblk_img;
    for (int i = t; i < nblk_img; i += 256) {
      s += (double)__uint_as_float(__hip_atomic_load((gu32*)(part + base + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
      for (int j = 0; j < NK; ++j)
        if (j < nk) k[j] += __hip_atomic_load((gu32*)(cnt + (base + i) * NK + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) shd[wv] = s;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      if (j < nk) {
        for (int m = 32; m > 0; m >>= 1) k[j] += __shfl_xor(k[j], m);
        if (lane == 0) shl[wv * NK + j] = k[j];
      }
    }
    __syncthreads();
    if (t == 0) {
      const double es = ((shd[0] + shd[1]) + shd[2]) + shd[3];
      write(img, es, [&](int j) { return shl[j] + shl[NK + j] + shl[2 * NK + j] + shl[3 * NK + j]; });
    }
    __syncthreads();
  }
  if (t == 0) {
    if (host_fence) __threadfence_system();
    __hip_atomic_store((gu32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// LABELS: the launch also leaves the label map of label_up_kernel, speculatively, for every image (one byte per pixel): the max sweep
// becomes the strict `>` arg-max sweep, which leaves the max that fmaxf leaves, so `out` / `out_host` carry the bits of the plain gate
struct GateLabelUpK : GateUpK { const uint8_t* lut; uint8_t* labels; };
template <bool LABELS> struct GateUpArg { typedef GateUpK type; };
template <> struct GateUpArg<true> { typedef GateLabelUpK type; };

template <int CC, bool VEC, bool LABELS = false>
__global__ void __launch_bounds__(256) gate_up_kernel(const typename GateUpArg<LABELS>::type p) {
  const float thr = *(const gfloat*)p.thr;
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
    exp_sweep<CC>(z, mx, se, sx);
    esum += logf(se) - sx / se;
    hit[0] += (1.f / se > thr) ? 1u : 0u;
  });
  up_finish<1>(esum, hit, 1, p.counter, p.part, p.cnt, p.N, p.nblk_img, p.out_host != nullptr, [&](int img, double es, auto&& count) {
    const float ent = (float)(es / p.ent_div), share = (float)((double)count(0) / p.npix);
    ((gfloat*)p.out)[2 * img] = ent; ((gfloat*)p.out)[2 * img + 1] = share;
    if (p.out_host) { p.out_host[2 * img] = ent; p.out_host[2 * img + 1] = share; }
  });
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

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) profile_up_kernel(const ProfileUpK p) {
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
  int key = -1; unsigned run = 0;                                // pending (gt, pred) run of this column
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    const long tg = tgt[pix];
    float mx = -INFINITY; int am = 0;
#pragma unroll
    for (int c = 0; c < CC; ++c)
      if (z[c] > mx) { mx = z[c]; am = c; }                      // strict: a tie keeps the lowest channel
    float se, sx;
    exp_sweep<CC>(z, mx, se, sx);
    esum += logf(se) - sx / se;
    const float pmax = 1.f / se;
#pragma unroll
    for (int j = 0; j < PRU_NT; ++j) hit[j] += (pmax > thr[j]) ? 1u : 0u;
    if (p.pred) p.pred[pix] = (uint8_t)am;
    const int k = (tg >= 0 && tg < CC) ? (int)tg * CC + am : -1;     // the evaluator's mask: labels in [0, C), whatever ignore_index is
    if (k != key) {
      if (key >= 0) atomicAdd(&hist[key], run);
      key = k; run = 0;
    }
    ++run;
  });
  if (key >= 0) atomicAdd(&hist[key], run);
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

// the gate launch's arguments behind the UpSrc prefix (both of its forms): outputs, workspace layout, normalisation
void gate_up_fill(GateUpK& k, const addk_gate_upsample_args* a) {
  const dim3 grid = scu_grid(a->N, a->OH, a->OW);
  static_cast<UpSrc&>(k) = up_src(a);
  k.thr = a->max_thr; k.out = a->out; k.out_host = a->out_host;
  k.nblk_img = (int)(grid.x * grid.y);
  k.counter = (unsigned*)a->ws;
  k.part = (float*)((char*)a->ws + 16);
  k.cnt = (unsigned*)(k.part + (long)a->N * k.nblk_img);
  k.npix = (double)a->OH * (double)a->OW; k.ent_div = log(19.0) * k.npix;
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
    if (k != key) {
      if (key >= 0) atomicAdd(&hist[key], run);
      key = k; run = 0;
    }
    ++run;
  });
  if (key >= 0) atomicAdd(&hist[key], run);
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
  return scu_ok(N, H, W, OH, OW, C) && (long)N * OH * OW < (1L << 31);
}
int ohem_stream_blocks(long n) { long b = cdiv(n, 256 * 16); if (b < 1) b = 1; if (b > OHEM_KEEP_BLOCKS) b = OHEM_KEEP_BLOCKS; return (int)b; }

int ce_blocks(long total) { long b = cdiv(total, 256 * 4); if (b < 1) b = 1; if (b > 1024) b = 1024; return (int)b; }

}  // namespace

extern "C" int64_t addk_ce_ws_floats(int32_t N, int64_t HW) { (void)N; (void)HW; return 1024; }

extern "C" int addk_ce_count(const int64_t* target, int64_t n, const float* class_w, int32_t ignore_index, int32_t num_classes,
                             float* wsum, float* ws, void* stream) {
  ADDK_REQUIRE(target && wsum && ws && n > 0 && num_classes > 0, "ce_count: bad args");
  hipStream_t st = (hipStream_t)stream;
  int b = ce_blocks(n);
  hipLaunchKernelGGL(ce_count_kernel, dim3(b), dim3(256), 0, st, target, (long)n, class_w, ignore_index, num_classes, ws);
  int rc = addk_check_launch("ce_count");
  if (rc) return rc;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, ws, b, 1.f, (const float*)nullptr, wsum, 0);
  return addk_check_launch("ce_count_sum");
}

extern "C" int addk_ce_fwd_bwd(const float* logits, const int64_t* target, int32_t N, int32_t C, int64_t HW, const float* class_w,
                               int32_t ignore_index, const float* wsum, float scale, float* loss_out, float* dlogits, float* ws,
                               void* stream) {
  ADDK_REQUIRE(logits && target && wsum && loss_out && ws && N > 0 && C > 0 && HW > 0, "ce_fwd_bwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  int b = ce_blocks((long)N * HW);
  if (C == 19)
    hipLaunchKernelGGL(ce_kernel<19>, dim3(b), dim3(256), 0, st, logits, target, N, C, (long)HW, class_w, ignore_index, wsum, scale, dlogits, ws);
  else
    hipLaunchKernelGGL(ce_kernel<0>, dim3(b), dim3(256), 0, st, logits, target, N, C, (long)HW, class_w, ignore_index, wsum, scale, dlogits, ws);
  int rc = addk_check_launch("ce");
  if (rc) return rc;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, ws, b, scale, wsum, loss_out, 1);
  return addk_check_launch("ce_sum");
}


extern "C" int addk_ce_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return ceu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_ce_upsample_ws_floats(int32_t N, int32_t H, int32_t W) {
  return (int64_t)N * cdiv(H, ceu_hb(H)) * cdiv(W, CEU_X - 1);
}
extern "C" int addk_ce_upsample_fwd_bwd(const addk_ce_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->wsum && a->loss_out && a->g && a->ws, "ce_upsample: null pointer");
  ADDK_REQUIRE(a->ld >= a->C && a->ldg >= a->C, "ce_upsample: short stride");
  ADDK_REQUIRE(ceu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "ce_upsample: unsupported shape (19 classes, at most %d output rows per input row)", CEU_MAXBAND);
  CeUpK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.cw = a->class_w; k.ignore = a->ignore_index; k.wsum = a->wsum; k.scale = a->scale;
  k.g = a->g; k.ldg = a->ldg; k.accumulate = a->accumulate; k.ws = a->ws; k.HB = ceu_hb(a->H);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(a->W, CEU_X - 1), cdiv(a->H, k.HB), a->N);
  hipLaunchKernelGGL(ce_up_kernel<19>, grid, dim3(256), 0, st, k);
  int rc = addk_check_launch("ce_upsample");
  if (rc) return rc;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, a->ws, (int)(grid.x * grid.y * grid.z), a->scale, a->wsum, a->loss_out, 1);
  return addk_check_launch("ce_upsample_sum");
}

extern "C" int addk_ce_upsample_ohem_fwd_bwd(const addk_ce_upsample_ohem_args* b, void* stream) {
  ADDK_REQUIRE(b, "ce_upsample_ohem: null pointer");
  const addk_ce_upsample_args* a = &b->ce;
  ADDK_REQUIRE(a->logits && a->target && a->wsum && a->loss_out && a->g && a->ws && b->pix_loss && b->tau, "ce_upsample_ohem: null pointer");
  ADDK_REQUIRE(a->ld >= a->C && a->ldg >= a->C, "ce_upsample_ohem: short stride");
  ADDK_REQUIRE(ceu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "ce_upsample_ohem: unsupported shape (19 classes, at most %d output rows per input row)", CEU_MAXBAND);
  CeUpOhemK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.cw = a->class_w; k.ignore = a->ignore_index; k.wsum = a->wsum; k.scale = a->scale;
  k.g = a->g; k.ldg = a->ldg; k.accumulate = a->accumulate; k.ws = a->ws; k.HB = ceu_hb(a->H);
  k.lmap = b->pix_loss; k.tau = b->tau;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(a->W, CEU_X - 1), cdiv(a->H, k.HB), a->N);
  hipLaunchKernelGGL((ce_up_kernel<19, true>), grid, dim3(256), 0, st, k);
  int rc = addk_check_launch("ce_upsample_ohem");
  if (rc) return rc;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, a->ws, (int)(grid.x * grid.y * grid.z), a->scale, a->wsum, a->loss_out, 1);
  return addk_check_launch("ce_upsample_ohem_sum");
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
  ADDK_REQUIRE(a->ld >= a->C && a->ldg >= a->C && b->ld_teacher >= a->C, "ce_upsample_kd: short stride");
  ADDK_REQUIRE(isfinite(b->alpha) && b->alpha > 0.f && isfinite(b->temperature) && b->temperature > 0.f,
               "ce_upsample_kd: alpha and temperature must be positive and finite");
  ADDK_REQUIRE(ceu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "ce_upsample_kd: unsupported shape (19 classes, at most %d output rows per input row)", CEU_MAXBAND);
  CeUpKdK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.cw = a->class_w; k.ignore = a->ignore_index; k.wsum = a->wsum; k.scale = a->scale;
  k.g = a->g; k.ldg = a->ldg; k.accumulate = a->accumulate; k.ws = a->ws; k.HB = ceu_hb(a->H);
  k.lmap = b->pix_loss; k.tau = b->tau;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(a->W, CEU_X - 1), cdiv(a->H, k.HB), a->N);
  const int nblk = (int)(grid.x * grid.y * grid.z);
  k.teacher = b->teacher; k.ldt = b->ld_teacher; k.nvalid = b->nvalid; k.ws2 = a->ws + nblk;
  k.rT = 1.f / b->temperature;
  k.kscale = a->scale * b->alpha * b->temperature;              // the gradient's factor before 1/n; the loss takes one more T
  const bool tvec = px_vec_ok<19>(b->teacher, b->ld_teacher);
  if (b->pix_loss) {
    if (tvec) hipLaunchKernelGGL((ce_up_kernel<19, true, true, true>), grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((ce_up_kernel<19, true, true, false>), grid, dim3(256), 0, st, k);
  } else {
    if (tvec) hipLaunchKernelGGL((ce_up_kernel<19, false, true, true>), grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((ce_up_kernel<19, false, true, false>), grid, dim3(256), 0, st, k);
  }
  int rc = addk_check_launch("ce_upsample_kd");
  if (rc) return rc;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, a->ws, nblk, a->scale, a->wsum, a->loss_out, 1);
  rc = addk_check_launch("ce_upsample_kd_sum");
  if (rc) return rc;
  hipLaunchKernelGGL(kd_sum_kernel, dim3(1), dim3(256), 0, st, k.ws2, nblk, k.kscale * b->temperature, b->nvalid, b->kd_out, a->loss_out);
  return addk_check_launch("ce_upsample_kd_kl_sum");
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
  ADDK_REQUIRE(ohem_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "ohem_select: unsupported shape (19 classes, fewer than 2^31 pixels)");
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
  if (px_vec_ok<19>(a->logits, a->ld))
    hipLaunchKernelGGL((ohem_loss_kernel<19, true>), scu_grid(a->N, a->OH, a->OW), blk, 0, st, k);
  else
    hipLaunchKernelGGL((ohem_loss_kernel<19, false>), scu_grid(a->N, a->OH, a->OW), blk, 0, st, k);
  hipLaunchKernelGGL(ohem_scan_kernel, one, blk, 0, st, w, OHEM_B0 / 256, 11, 0, sel, (unsigned long long)a->min_kept_total, tau_theta, (float*)nullptr, counts);
  hipLaunchKernelGGL((ohem_refine_kernel<21, 10, OHEM_B0>), dim3(nb), blk, 0, st, a->pix_loss, npix, sel, w + OHEM_B0);
  hipLaunchKernelGGL(ohem_scan_kernel, one, blk, 0, st, w + OHEM_B0, OHEM_B0 / 256, 11, 1, sel, 0ull, tau_theta, (float*)nullptr, counts);
  hipLaunchKernelGGL((ohem_refine_kernel<10, 0, OHEM_B2>), dim3(nb), blk, 0, st, a->pix_loss, npix, sel, w + 2 * OHEM_B0);
  hipLaunchKernelGGL(ohem_scan_kernel, one, blk, 0, st, w + 2 * OHEM_B0, OHEM_B2 / 256, 10, 2, sel, 0ull, tau_theta, a->tau, counts);
  hipLaunchKernelGGL(ohem_keep_kernel, dim3(nb), blk, 0, st, a->pix_loss, a->target, a->class_w, npix, a->tau, wpart, kpart);
  hipLaunchKernelGGL(ohem_keep_sum_kernel, one, blk, 0, st, wpart, kpart, nb, a->wsum_kept, counts);
  return addk_check_launch("ohem_select");
}

extern "C" int addk_score_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return scu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_score_upsample_ws_floats(int32_t N, int32_t OH, int32_t OW) {
  return 2 * scu_blocks(N, OH, OW);
}
extern "C" int addk_score_upsample(const addk_score_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->wsum && a->loss_out && a->ent_out && a->cm && a->ws, "score_upsample: null pointer");
  ADDK_REQUIRE(a->ld >= a->C, "score_upsample: short stride");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "score_upsample: unsupported shape (19 classes)");
  const dim3 grid = scu_grid(a->N, a->OH, a->OW);
  ScoreUpK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.cw = a->class_w; k.ignore = a->ignore_index;
  k.cm = reinterpret_cast<unsigned long long*>(a->cm); k.pred = a->pred_out;
  k.ws = a->ws; k.nblk = (int)scu_blocks(a->N, a->OH, a->OW);
  hipStream_t st = (hipStream_t)stream;
  if (px_vec_ok<19>(a->logits, a->ld))
    hipLaunchKernelGGL((score_up_kernel<19, true>), grid, dim3(256), 0, st, k);
  else
    hipLaunchKernelGGL((score_up_kernel<19, false>), grid, dim3(256), 0, st, k);
  int rc = addk_check_launch("score_upsample");
  if (rc) return rc;
  hipLaunchKernelGGL(score_sum_kernel, dim3(2), dim3(256), 0, st, a->ws, k.nblk, a->scale, a->wsum, a->loss_out, a->ent_out);
  return addk_check_launch("score_upsample_sum");
}

extern "C" int addk_gate_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return scu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int64_t addk_gate_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  return 16 + 8 * scu_blocks(N, OH, OW);
}
extern "C" int addk_gate_upsample(const addk_gate_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->max_thr && a->out && a->ws, "gate_upsample: null pointer");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "gate_upsample: unsupported shape (19 classes)");
  ADDK_REQUIRE(a->ld >= a->C, "gate_upsample: short stride");
  GateUpK k;
  gate_up_fill(k, a);
  hipStream_t st = (hipStream_t)stream;
  if (px_vec_ok<19>(a->logits, a->ld))
    hipLaunchKernelGGL((gate_up_kernel<19, true>), scu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, k);
  else
    hipLaunchKernelGGL((gate_up_kernel<19, false>), scu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, k);
  return addk_check_launch("gate_upsample");
}
extern "C" int addk_gate_label_upsample(const addk_gate_label_upsample_args* b, void* stream) {
  ADDK_REQUIRE(b, "gate_label_upsample: null pointer");
  const addk_gate_upsample_args* a = &b->gate;
  ADDK_REQUIRE(a->logits && a->max_thr && a->out && a->ws && b->labels, "gate_label_upsample: null pointer");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "gate_label_upsample: unsupported shape (19 classes)");
  ADDK_REQUIRE(a->ld >= a->C, "gate_label_upsample: short stride");
  GateLabelUpK k;
  gate_up_fill(k, a);
  k.lut = b->lut256; k.labels = b->labels;
  hipStream_t st = (hipStream_t)stream;
  if (px_vec_ok<19>(a->logits, a->ld))
    hipLaunchKernelGGL((gate_up_kernel<19, true, true>), scu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, k);
  else
    hipLaunchKernelGGL((gate_up_kernel<19, false, true>), scu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, k);
  return addk_check_launch("gate_label_upsample");
}

extern "C" int addk_label_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return scu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}
extern "C" int addk_label_upsample(const addk_label_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->labels, "label_upsample: null pointer");
  ADDK_REQUIRE(scu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "label_upsample: unsupported shape (19 classes)");
  ADDK_REQUIRE(a->ld >= a->C, "label_upsample: short stride");
  LabelUpK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.lut = a->lut256; k.labels = a->labels;
  hipStream_t st = (hipStream_t)stream;
  if (px_vec_ok<19>(a->logits, a->ld))
    hipLaunchKernelGGL((label_up_kernel<19, true>), scu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, k);
  else
    hipLaunchKernelGGL((label_up_kernel<19, false>), scu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, k);
  return addk_check_launch("label_upsample");
}

extern "C" int addk_label_views_upsample_supported(int32_t nview, int32_t N, int32_t OH, int32_t OW, int32_t C) {
  return lvu_ok(nview, N, OH, OW, C) ? 1 : 0;
}
extern "C" int addk_label_views_upsample(const addk_label_views_args* a, void* stream) {
  ADDK_REQUIRE(a && a->labels, "label_views_upsample: null pointer");
  ADDK_REQUIRE(lvu_ok(a->nview, a->N, a->OH, a->OW, a->C), "label_views_upsample: unsupported shape (1..%d views, 19 classes)", ADDK_MAX_VIEWS);
  bool vec = true;
  for (int v = 0; v < a->nview; ++v) {
    const addk_view& w = a->view[v];
    ADDK_REQUIRE(w.logits, "label_views_upsample: null pointer (view %d)", v);
    ADDK_REQUIRE(w.H > 0 && w.W > 0 && w.n0 >= 0 && w.ld >= a->C, "label_views_upsample: bad size, image offset or stride (view %d)", v);
    ADDK_REQUIRE(w.weight > 0.f && isfinite(w.weight), "label_views_upsample: a weight must be positive and finite (view %d)", v);
    vec = vec && px_vec_ok<19>(w.logits, w.ld);
  }
  hipStream_t st = (hipStream_t)stream;
  if (vec)                                                         // 16-byte pixel loads only where every view allows them
    hipLaunchKernelGGL((label_views_kernel<19, true>), lvu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, *a);
  else
    hipLaunchKernelGGL((label_views_kernel<19, false>), lvu_grid(a->N, a->OH, a->OW), dim3(256), 0, st, *a);
  return addk_check_launch("label_views_upsample");
}

extern "C" int addk_profile_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C, int32_t nthr) {
  return scu_ok(N, H, W, OH, OW, C) && nthr >= 0 && nthr <= PRU_NT ? 1 : 0;
}
extern "C" int64_t addk_profile_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  return 16 + (4 + 4 * PRU_NT) * scu_blocks(N, OH, OW);
}
extern "C" int addk_profile_upsample(const addk_profile_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->ent_out && a->cm && a->ws, "profile_upsample: null pointer");
  ADDK_REQUIRE(addk_profile_upsample_supported(a->N, a->H, a->W, a->OH, a->OW, a->C, a->nthr) == 1,
               "profile_upsample: unsupported shape (19 classes, at most %d thresholds)", PRU_NT);
  ADDK_REQUIRE(a->nthr == 0 || (a->thr && a->share_out), "profile_upsample: null pointer");
  ADDK_REQUIRE(a->ld >= a->C, "profile_upsample: short stride");
  const dim3 grid = scu_grid(a->N, a->OH, a->OW);
  ProfileUpK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.thr = a->thr; k.nthr = a->nthr;
  k.ent = a->ent_out; k.share = a->share_out; k.cm = reinterpret_cast<unsigned long long*>(a->cm); k.pred = a->pred_out;
  k.nblk_img = (int)(grid.x * grid.y);
  k.counter = (unsigned*)a->ws;
  k.part = (float*)((char*)a->ws + 16);
  k.cnt = (unsigned*)(k.part + (long)a->N * k.nblk_img);
  k.npix = (double)a->OH * (double)a->OW; k.ent_div = log(19.0) * k.npix;
  hipStream_t st = (hipStream_t)stream;
  if (px_vec_ok<19>(a->logits, a->ld))
    hipLaunchKernelGGL((profile_up_kernel<19, true>), grid, dim3(256), 0, st, k);
  else
    hipLaunchKernelGGL((profile_up_kernel<19, false>), grid, dim3(256), 0, st, k);
  return addk_check_launch("profile_upsample");
}

extern "C" int addk_entropy_sum(const float* logits, int32_t N, int32_t C, int64_t HW, float* out1, float* ws, void* stream) {
  ADDK_REQUIRE(logits && out1 && ws && N > 0 && C > 0 && HW > 0, "entropy_sum: bad args");
  hipStream_t st = (hipStream_t)stream;
  int b = ce_blocks((long)N * HW);
  hipLaunchKernelGGL(entropy_kernel, dim3(b), dim3(256), 0, st, logits, N, C, (long)HW, ws);
  int rc = addk_check_launch("entropy");
  if (rc) return rc;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, ws, b, 1.f, (const float*)nullptr, out1, 0);
  return addk_check_launch("entropy_sum");
}

extern "C" int addk_argmax_nchw(const float* logits, int32_t N, int32_t C, int64_t HW, int64_t* out, void* stream) {
  ADDK_REQUIRE(logits && out && N > 0 && C > 0 && HW > 0, "argmax: bad args");
  long b = cdiv((long)N * HW, 256); if (b > 8192) b = 8192;
  hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, logits, N, C, (long)HW, out);
  return addk_check_launch("argmax");
}

extern "C" int addk_confusion(const int64_t* gt, const int64_t* pred, int64_t n, int32_t num_class, int64_t* cm, void* stream) {
  ADDK_REQUIRE(gt && pred && cm && n > 0 && num_class > 0, "confusion: bad args");
  long b = cdiv(n, 256); if (b > 4096) b = 4096;
  hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, gt, pred, (long)n, num_class,
                     reinterpret_cast<unsigned long long*>(cm));
  return addk_check_launch("confusion");
}
