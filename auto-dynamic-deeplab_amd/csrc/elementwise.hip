// Elementwise / channel-reducing kernels of the path (all HBM-bound, 16 B per lane):
//   affine_sum      — the branch sum of a cell block (ADD.py:108) with the branches' BatchNorms applied on
//                     the fly, written into the block's slot of the cell concat buffer (ADD.py:112)
//   affine_sum_bwd  — its gradient + the per-channel sums that drive the branches' BN backward
//   bn_bwd_apply    — dy = g + c1 + c2*(x - mean) (training-mode BatchNorm backward on the raw conv output)
//   sgd_step, fill
//
// Thread map (EwMap): a 256-thread block is npl pixel lanes x nq channel quads, thread = pl * nq + q, and keeps its quad c = 4q.
// Every element keeps ONE expression whichever kernel form computes it: bn_bwd_apply g + fmaf(c2, x - mean, c1); affine_sum
// fmaf(a, x, b) (ReLU), the terms added in term order to 0, ReLU, then + out when accumulating.  The vector-aligned affine_sum forms walk two
// pixels per trip with every load of both requested before anything is used; a missing second pixel re-reads the first and is not
// stored (a branch round a load makes the compiler drain every load in flight at the join).
//
// Order of the fp64 sums of affine_sum_bwd (dab row blockIdx.x, [C][2] = (sum dm*x, sum dm); generic and vector forms, bit for bit):
//   1. a thread's pixels ascend from blockIdx.x * npl + pl in steps of gridDim.x * npl (gridDim.x = ew_rows(P, C));
//   2. each thread adds its pixels' terms, in that order, to a double that starts at 0 (products of two floats are exact in double);
//   3. the block sum starts at 0 and adds the pixel lanes pl = 0 .. npl-1 in that order.
// The vector form keeps 3 while reading the lanes' values from LDS in unrolled groups: the reads of a group are requested together,
// the adds stay one after the other in lane order.
#include "common.h"

namespace {

struct SumK {
  addk_src term[ADDK_MAX_TERMS]; int nterm;
  long P; int C;
  float* out; int ldo; int relu_out; int accumulate;
  const float* dout; int lddo;
  const float* fout; int ldfo;
  float* g[ADDK_MAX_TERMS]; int ldg[ADDK_MAX_TERMS]; int acc[ADDK_MAX_TERMS];
  double* dab[ADDK_MAX_TERMS];
  int nq, npl, vec;
};

__global__ void __launch_bounds__(256) affine_sum_fwd_kernel(const SumK p) {
  const int q = threadIdx.x % p.nq, pl = threadIdx.x / p.nq;
  if (pl >= p.npl) return;
  const int c = 4 * q, nrem = p.C - c;
  float4 av[ADDK_MAX_TERMS], bv[ADDK_MAX_TERMS];
#pragma unroll
  for (int i = 0; i < ADDK_MAX_TERMS; ++i) {
    av[i] = make_float4(1.f, 1.f, 1.f, 1.f); bv[i] = zero4();
    if (i < p.nterm && p.term[i].a) { av[i] = ld4g(p.term[i].a + c, nrem, p.vec); bv[i] = ld4g(p.term[i].b + c, nrem, p.vec); }
  }
  for (long pp = (long)blockIdx.x * p.npl + pl; pp < p.P; pp += (long)gridDim.x * p.npl) {
    float4 s = zero4();
#pragma unroll
    for (int i = 0; i < ADDK_MAX_TERMS; ++i) {
      if (i < p.nterm) {
        float4 x = ld4g(p.term[i].x + pp * p.term[i].ld + c, nrem, p.vec);
        float4 z = make_float4(fmaf(av[i].x, x.x, bv[i].x), fmaf(av[i].y, x.y, bv[i].y), fmaf(av[i].z, x.z, bv[i].z), fmaf(av[i].w, x.w, bv[i].w));
        if (p.term[i].relu) { z.x = fmaxf(z.x, 0.f); z.y = fmaxf(z.y, 0.f); z.z = fmaxf(z.z, 0.f); z.w = fmaxf(z.w, 0.f); }
        s.x += z.x; s.y += z.y; s.z += z.z; s.w += z.w;
      }
    }
    if (p.relu_out) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f); }
    float* op = p.out + pp * p.ldo + c;
    if (p.accumulate) { float4 o = ld4g(op, nrem, p.vec); s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w; }
    st4g(op, s, nrem, p.vec);
  }
}

// Vector-aligned form of affine_sum_fwd_kernel with the term count a template parameter: plain 16-byte loads, two pixels per trip, the
// `accumulate` read of out requested with the terms' loads.  Same expression per element as the generic kernel: bit-identical results.
template <int NT>
__global__ void __launch_bounds__(256) affine_sum_fwd_vec_kernel(const SumK p) {
  const int q = threadIdx.x % p.nq, pl = threadIdx.x / p.nq;
  if (pl >= p.npl) return;
  const int c = 4 * q;
  float4 av[NT], bv[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    av[i] = make_float4(1.f, 1.f, 1.f, 1.f); bv[i] = zero4();
    if (p.term[i].a) { av[i] = ld4(p.term[i].a + c); bv[i] = ld4(p.term[i].b + c); }
  }
  auto sum = [&](const float4 (&x)[NT], const float4 o) {
    float4 s = zero4();
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      float4 z = make_float4(fmaf(av[i].x, x[i].x, bv[i].x), fmaf(av[i].y, x[i].y, bv[i].y), fmaf(av[i].z, x[i].z, bv[i].z), fmaf(av[i].w, x[i].w, bv[i].w));
      if (p.term[i].relu) { z.x = fmaxf(z.x, 0.f); z.y = fmaxf(z.y, 0.f); z.z = fmaxf(z.z, 0.f); z.w = fmaxf(z.w, 0.f); }
      s.x += z.x; s.y += z.y; s.z += z.z; s.w += z.w;
    }
    if (p.relu_out) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f); }
    if (p.accumulate) { s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w; }
    return s;
  };
  // no load behind a run-time condition (see affine_sum_bwd_vec_kernel): without `accumulate` the read of out falls on term 0 and is not used
  const float* ob = p.accumulate ? p.out : p.term[0].x; const long ldob = p.accumulate ? p.ldo : p.term[0].ld;
  const long stride = (long)gridDim.x * p.npl;
  for (long p0 = (long)blockIdx.x * p.npl + pl; p0 < p.P; p0 += 2 * stride) {
    const long p1 = p0 + stride;
    const bool ok1 = p1 < p.P;
    const long q1 = ok1 ? p1 : p0;
    float4 x0[NT], x1[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) { x0[i] = ld4(p.term[i].x + p0 * p.term[i].ld + c); x1[i] = ld4(p.term[i].x + q1 * p.term[i].ld + c); }
    const float4 o0 = ld4(ob + p0 * ldob + c), o1 = ld4(ob + q1 * ldob + c);
    st4(p.out + p0 * p.ldo + c, sum(x0, o0));
    if (ok1) st4(p.out + p1 * p.ldo + c, sum(x1, o1));
  }
}

__global__ void __launch_bounds__(256) affine_sum_bwd_kernel(const SumK p) {
  extern __shared__ double redt[];       // [C4][2]
  const int q = threadIdx.x % p.nq, pl = threadIdx.x / p.nq;
  const bool active = pl < p.npl;
  const int c = 4 * q, nrem = p.C - c;
  float4 av[ADDK_MAX_TERMS], bv[ADDK_MAX_TERMS];
  double sA[ADDK_MAX_TERMS][4], sB[ADDK_MAX_TERMS][4];
#pragma unroll
  for (int i = 0; i < ADDK_MAX_TERMS; ++i) {
    av[i] = make_float4(1.f, 1.f, 1.f, 1.f); bv[i] = zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) { sA[i][e] = 0.0; sB[i][e] = 0.0; }
    if (active && i < p.nterm && p.term[i].a) { av[i] = ld4g(p.term[i].a + c, nrem, p.vec); bv[i] = ld4g(p.term[i].b + c, nrem, p.vec); }
  }
  if (active) {
    for (long pp = (long)blockIdx.x * p.npl + pl; pp < p.P; pp += (long)gridDim.x * p.npl) {
      float4 d = ld4g(p.dout + pp * p.lddo + c, nrem, p.vec);
      if (p.relu_out) {
        float4 o = ld4g(p.fout + pp * p.ldfo + c, nrem, p.vec);
        if (!(o.x > 0.f)) d.x = 0.f; if (!(o.y > 0.f)) d.y = 0.f; if (!(o.z > 0.f)) d.z = 0.f; if (!(o.w > 0.f)) d.w = 0.f;
      }
#pragma unroll
      for (int i = 0; i < ADDK_MAX_TERMS; ++i) {
        if (i < p.nterm && (p.g[i] || p.dab[i])) {
          float4 x = ld4g(p.term[i].x + pp * p.term[i].ld + c, nrem, p.vec);
          float4 dm = d;
          if (p.term[i].relu) {
            if (!(fmaf(av[i].x, x.x, bv[i].x) > 0.f)) dm.x = 0.f;
            if (!(fmaf(av[i].y, x.y, bv[i].y) > 0.f)) dm.y = 0.f;
            if (!(fmaf(av[i].z, x.z, bv[i].z) > 0.f)) dm.z = 0.f;
            if (!(fmaf(av[i].w, x.w, bv[i].w) > 0.f)) dm.w = 0.f;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) { sA[i][e] += (double)get4(dm, e) * (double)get4(x, e); sB[i][e] += (double)get4(dm, e); }
          if (p.g[i]) {
            float4 gv = make_float4(dm.x * av[i].x, dm.y * av[i].y, dm.z * av[i].z, dm.w * av[i].w);
            float* gp = p.g[i] + pp * p.ldg[i] + c;
            if (p.acc[i]) { float4 o = ld4g(gp, nrem, p.vec); gv.x += o.x; gv.y += o.y; gv.z += o.z; gv.w += o.w; }
            st4g(gp, gv, nrem, p.vec);
          }
        }
      }
    }
  }
  // Block reduction over the pixel lanes through an [npl][C4][2] fp64 panel: one barrier, then one thread per (channel, A|B)
  // adds the npl rows in fixed order (the former lane-after-lane accumulation cost npl barrier rounds per term).
  const int C4 = p.nq * 4;
#pragma unroll
  for (int i = 0; i < ADDK_MAX_TERMS; ++i) {
    if (i < p.nterm && p.dab[i]) {          // block-uniform
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { redt[((pl * C4) + c + e) * 2] = sA[i][e]; redt[((pl * C4) + c + e) * 2 + 1] = sB[i][e]; }
      }
      __syncthreads();
      for (int k = threadIdx.x; k < p.C * 2; k += 256) {
        const int ch = k >> 1, ab = k & 1;
        double acc = 0.0;
        for (int r = 0; r < p.npl; ++r) acc += redt[((r * C4) + ch) * 2 + ab];
        p.dab[i][(long)blockIdx.x * p.C * 2 + k] = acc;
      }
      __syncthreads();
    }
  }
}

// Vector-aligned form of affine_sum_bwd_kernel with the term count a template parameter: plain 16-byte loads, PX pixels per trip with every load of
// all of them requested before anything is used (the generic kernel's 2-3 trips per thread were 2-3 dependent round trips on launches that move 15-30 MB).
// Same per-thread pixel order and arithmetic as the generic kernel: bit-identical results.
// Block sums: every term's lane sums go into ONE fp64 panel [NT][npl][C4] of (A, B) pairs (npl * C4 <= 1024: 16 KB per term), one barrier, then the
// NT * 2C sums are spread over the 256 threads; a thread requests the npl values of its sum in groups of EW_RED_GROUP and adds them in lane order.
// EXTRA = the launch masks by the forward output (relu_out) or adds to a g already there: the plain launches carry no registers for those loads, which
// with the cap of 128 VGPRs at 1-2 terms keeps all four workgroups per CU of a 1024-row grid resident (152 VGPRs admitted three).
// Pixels per trip: four at two terms need 199 VGPRs (two workgroups per CU); three fit 128 and measure no faster than two (profiles/ew_kernel_time.txt).
constexpr int EW_RED_GROUP = 8, EW_BWD_PX = 2;
template <int NT, bool EXTRA>
__global__ void __launch_bounds__(256, (NT <= 2 && !EXTRA) ? 4 : 1) affine_sum_bwd_vec_kernel(const SumK p) {
  extern __shared__ double redt[];       // [NT][npl][C4][2]
  const int q = threadIdx.x % p.nq, pl = threadIdx.x / p.nq;
  const bool active = pl < p.npl;
  constexpr int PX = EW_BWD_PX;
  const bool relu_out = EXTRA && p.relu_out;
  const int c = 4 * q;
  float4 av[NT], bv[NT];
  double sA[NT][4], sB[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    av[i] = make_float4(1.f, 1.f, 1.f, 1.f); bv[i] = zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) { sA[i][e] = 0.0; sB[i][e] = 0.0; }
    if (active && p.term[i].a) { av[i] = ld4(p.term[i].a + c); bv[i] = ld4(p.term[i].b + c); }
  }
  if (active) {
    const long stride = (long)gridDim.x * p.npl;
    // (a term with neither g nor dab is summed like the others, into sums nobody writes out: a use behind a run-time condition takes its load with it)
    auto finish = [&](long pp, float4 d, const float4 o, const float4 (&x)[NT], const float4 (&gold)[NT]) {
      d.x = relu_out && !(o.x > 0.f) ? 0.f : d.x; d.y = relu_out && !(o.y > 0.f) ? 0.f : d.y;       // selects, not branches: o and gold are used on every path
      d.z = relu_out && !(o.z > 0.f) ? 0.f : d.z; d.w = relu_out && !(o.w > 0.f) ? 0.f : d.w;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        float4 dm = d;
        if (p.term[i].relu) {
          if (!(fmaf(av[i].x, x[i].x, bv[i].x) > 0.f)) dm.x = 0.f;
          if (!(fmaf(av[i].y, x[i].y, bv[i].y) > 0.f)) dm.y = 0.f;
          if (!(fmaf(av[i].z, x[i].z, bv[i].z) > 0.f)) dm.z = 0.f;
          if (!(fmaf(av[i].w, x[i].w, bv[i].w) > 0.f)) dm.w = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { sA[i][e] += (double)get4(dm, e) * (double)get4(x[i], e); sB[i][e] += (double)get4(dm, e); }
        if (p.g[i]) {
          float4 gv = make_float4(dm.x * av[i].x, dm.y * av[i].y, dm.z * av[i].z, dm.w * av[i].w);
          if (EXTRA) {
            const bool old = p.acc[i];
            gv.x = old ? gv.x + gold[i].x : gv.x; gv.y = old ? gv.y + gold[i].y : gv.y; gv.z = old ? gv.z + gold[i].z : gv.z; gv.w = old ? gv.w + gold[i].w : gv.w;
          }
          st4(p.g[i] + pp * p.ldg[i] + c, gv);
        }
      }
    };
    // No load sits behind a run-time condition (the compiler branches round such a load and drains every load in flight where the paths join): what a
    // launch does not need is read from dout instead, the pixel's line the trip fetches anyway, and not used.
    const float* ob = relu_out ? p.fout : p.dout; const long ldob = relu_out ? p.ldfo : p.lddo;
    const float* xb[NT]; const float* gb[NT]; long ldxb[NT], ldgb[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const bool used = p.g[i] || p.dab[i], old = EXTRA && p.g[i] && p.acc[i];
      xb[i] = used ? p.term[i].x : p.dout; ldxb[i] = used ? p.term[i].ld : p.lddo;
      gb[i] = old ? p.g[i] : p.dout; ldgb[i] = old ? p.ldg[i] : p.lddo;
    }
    for (long p0 = (long)blockIdx.x * p.npl + pl; p0 < p.P; p0 += PX * stride) {
      long pp[PX], qq[PX];                                 // (a missing pixel's loads fall on the trip's first)
#pragma unroll
      for (int j = 0; j < PX; ++j) { pp[j] = p0 + j * stride; qq[j] = pp[j] < p.P ? pp[j] : p0; }
      float4 d[PX], o[PX], x[PX][NT], g[PX][NT];
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        d[j] = ld4(p.dout + qq[j] * p.lddo + c);
        o[j] = EXTRA ? ld4(ob + qq[j] * ldob + c) : zero4();
      }
#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int j = 0; j < PX; ++j) {
          x[j][i] = ld4(xb[i] + qq[j] * ldxb[i] + c);
          g[j][i] = EXTRA ? ld4(gb[i] + qq[j] * ldgb[i] + c) : zero4();
        }
      }
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (j == 0 || pp[j] < p.P) finish(pp[j], d[j], o[j], x[j], g[j]);
    }
  }
  const int C4 = p.nq * 4;
  double2* pan = reinterpret_cast<double2*>(redt);
  if (active) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      if (p.dab[i]) {          // block-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) pan[(i * p.npl + pl) * C4 + c + e] = make_double2(sA[i][e], sB[i][e]);
      }
    }
  }
  __syncthreads();
  const int C2 = 2 * p.C, rs = 2 * C4;                    // sums per term; doubles per panel row
  for (int k = threadIdx.x; k < NT * C2; k += 256) {
    const int i = k / C2, k2 = k - i * C2;                // k2 = 2 * channel + (0: A, 1: B)
    double* dst = nullptr;
#pragma unroll
    for (int t = 0; t < NT; ++t) if (t == i) dst = p.dab[t];
    if (!dst) continue;
    const double* src = redt + (long)i * p.npl * rs + k2;
    double acc = 0.0;
    int r = 0;
    for (; r + EW_RED_GROUP <= p.npl; r += EW_RED_GROUP) {
      double v[EW_RED_GROUP];
#pragma unroll
      for (int j = 0; j < EW_RED_GROUP; ++j) v[j] = src[(r + j) * rs];
#pragma unroll
      for (int j = 0; j < EW_RED_GROUP; ++j) acc += v[j];
    }
    if (r < p.npl) {                                       // the last, partial group: reads past npl-1 fall on row npl-1 and are not added
      double v[EW_RED_GROUP - 1];
#pragma unroll
      for (int j = 0; j < EW_RED_GROUP - 1; ++j) v[j] = src[(r + j < p.npl ? r + j : p.npl - 1) * rs];
#pragma unroll
      for (int j = 0; j < EW_RED_GROUP - 1; ++j) if (r + j < p.npl) acc += v[j];
    }
    dst[(long)blockIdx.x * C2 + k2] = acc;
  }
}

// vector-aligned items (16-byte pointers, ld % 4 == 0, C = 4 nq): the blocks of gridDim.x stride over the item's pixels.  Every load is a
// plain 16-byte load; coefficients and the first pixel are one round trip, and the next pixel is requested before the current one is
// stored.  HAS_C: the item has c1 / c2 (and so x); the loop holds no condition on them (a load behind a run-time condition makes the
// compiler wait, where the paths join, for every load in flight: the next pixel would be awaited before the current one is stored).
template <bool HAS_C>
__device__ __forceinline__ void bn_bwd_apply_vec_body(const addk_bn_apply_item& it, int nq, int npl) {
  const int q = threadIdx.x % nq, pl = threadIdx.x / nq;
  if (pl >= npl) return;
  const int c = 4 * q, p0 = blockIdx.x * npl + pl;          // p0 < 2^31: the launchers cap the grid, npl <= 256
  long pp = p0;
  if (pp >= it.P) return;
  const long step = (long)gridDim.x * npl;
  const float4 k1 = HAS_C ? ld4(it.c1 + c) : zero4(), k2 = HAS_C ? ld4(it.c2 + c) : zero4();
  float4 mu = ld4((it.mean ? it.mean : it.g) + c);          // NULL: g's first row is read and not used (no load behind a condition)
  mu = it.mean ? mu : zero4();
  // the three pointers walk: one 32 x 32-bit multiply each for the first pixel, none per pixel after it
  const float* gp = it.g + (long)p0 * it.ldg + c; const float* xp = HAS_C ? it.x + (long)p0 * it.ldx + c : it.g; float* op = it.out + (long)p0 * it.ldo + c;
  const long sg = step * it.ldg, sx = step * it.ldx, so = step * it.ldo;
  float4 gv = ld4(gp), xv = HAS_C ? ld4(xp) : zero4();
  auto dy = [&]() {
    return make_float4(gv.x + fmaf(k2.x, xv.x - mu.x, k1.x), gv.y + fmaf(k2.y, xv.y - mu.y, k1.y),
                       gv.z + fmaf(k2.z, xv.z - mu.z, k1.z), gv.w + fmaf(k2.w, xv.w - mu.w, k1.w));
  };
  for (;;) {                                // the next pixel's loads and the store before them in ONE basic block: the store does not wait for them
    pp += step; gp += sg; xp += sx;
    if (pp >= it.P) { st4(op, dy()); break; }
    const float4 gn = ld4(gp), xn = HAS_C ? ld4(xp) : zero4();
    st4(op, dy());
    op += so; gv = gn; xv = xn;
  }
}
template <bool HAS_C>
__global__ void __launch_bounds__(256) bn_bwd_apply_vec_kernel(const addk_bn_apply_item it, int nq, int npl) {
  bn_bwd_apply_vec_body<HAS_C>(it, nq, npl);
}
// several independent tensors in one launch: block (x, y) strides over the pixels of item y
__global__ void __launch_bounds__(256) bn_bwd_apply_batch_kernel(const addk_bn_apply_item* __restrict__ tab) {
  const addk_bn_apply_item it = tab[blockIdx.y];
  const int nq = it.C >> 2;
  if (it.c2) bn_bwd_apply_vec_body<true>(it, nq, 256 / nq);          // uniform
  else bn_bwd_apply_vec_body<false>(it, nq, 256 / nq);
}

// any alignment, any C <= 1024 (the lone entry only): guarded loads and stores
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const addk_bn_apply_item it, int nq, int npl, int vec) {
  const int q = threadIdx.x % nq, pl = threadIdx.x / nq;
  if (pl >= npl) return;
  const int c = 4 * q, nrem = it.C - c;
  float4 mu = it.mean ? ld4g(it.mean + c, nrem, vec) : zero4();
  float4 k1 = it.c1 ? ld4g(it.c1 + c, nrem, vec) : zero4();
  float4 k2 = it.c2 ? ld4g(it.c2 + c, nrem, vec) : zero4();
  for (long pp = (long)blockIdx.x * npl + pl; pp < it.P; pp += (long)gridDim.x * npl) {
    float4 gv = ld4g(it.g + pp * it.ldg + c, nrem, vec);
    float4 xv = it.c2 ? ld4g(it.x + pp * it.ldx + c, nrem, vec) : zero4();
    float4 o = make_float4(gv.x + fmaf(k2.x, xv.x - mu.x, k1.x), gv.y + fmaf(k2.y, xv.y - mu.y, k1.y),
                           gv.z + fmaf(k2.z, xv.z - mu.z, k1.z), gv.w + fmaf(k2.w, xv.w - mu.w, k1.w));
    st4g(it.out + pp * it.ldo + c, o, nrem, vec);
  }
}

__global__ void fill_kernel(float* p, long n, float v) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

__global__ void sgd_kernel(float* p, const float* g, float* buf, long n, const float* lr_dev, float mom, float wd,
                           int nesterov, int first, float gscale) {
  const float lr = *lr_dev;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float w = p[i];
    float d = fmaf(wd, w, g[i] * gscale);
    float b = first ? d : fmaf(mom, buf[i], d);
    buf[i] = b;
    float step = nesterov ? fmaf(mom, b, d) : b;
    p[i] = w - lr * step;
  }
}

int ew_blocks(long P, int npl) {
  long b = cdiv(P, (long)npl);
  if (b < 1) b = 1;
  if (b > 8192) b = 8192;
  return (int)b;
}
// grid of affine_sum_fwd_vec_kernel: two pixels per thread, at most 8 workgroups per CU (all resident at <= 64 VGPRs)
int ew_stream_blocks(long P, int npl) {
  long b = cdiv(P, 2L * npl);
  if (b < 1) b = 1;
  if (b > 2048) b = 2048;
  return (int)b;
}

}  // namespace

extern "C" int addk_ew_rows(int64_t P, int32_t C) { return ew_rows(P, C); }

extern "C" int addk_affine_sum_fwd(const addk_affine_sum_args* a, void* stream) {
  ADDK_REQUIRE(a && a->nterm >= 1 && a->nterm <= ADDK_MAX_TERMS && a->P > 0 && a->C > 0 && a->C <= 1024, "affine_sum: bad args");
  ADDK_REQUIRE(a->out && a->ldo >= a->C, "affine_sum: bad output");
  SumK k{};
  k.vec = aligned16(a->out) && a->ldo % 4 == 0;
  for (int i = 0; i < a->nterm; ++i) {
    ADDK_REQUIRE(a->term[i].x && a->term[i].ld >= a->C && a->term[i].C == a->C, "affine_sum: bad term %d", i);
    ADDK_REQUIRE((a->term[i].a == nullptr) == (a->term[i].b == nullptr), "affine_sum: a/b must come together");
    k.term[i] = a->term[i];
    if (!src_vec_ok(a->term[i])) k.vec = 0;
  }
  k.nterm = a->nterm; k.P = a->P; k.C = a->C; k.out = a->out; k.ldo = a->ldo; k.relu_out = a->relu_out; k.accumulate = a->accumulate;
  EwMap m = ew_map(a->C); k.nq = m.nq; k.npl = m.npl;
  if (k.vec && a->C == m.nq * 4) {          // src_vec_ok: every x, a, b 16-byte aligned, ld % 4 == 0, C % 4 == 0
    const dim3 grid(ew_stream_blocks(a->P, m.npl));
    switch (a->nterm) {
      case 1: hipLaunchKernelGGL(affine_sum_fwd_vec_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, k); break;
      case 2: hipLaunchKernelGGL(affine_sum_fwd_vec_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, k); break;
      case 3: hipLaunchKernelGGL(affine_sum_fwd_vec_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, k); break;
      default: hipLaunchKernelGGL(affine_sum_fwd_vec_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, k); break;
    }
    return addk_check_launch("affine_sum_fwd");
  }
  hipLaunchKernelGGL(affine_sum_fwd_kernel, dim3(ew_blocks(a->P, m.npl)), dim3(256), 0, (hipStream_t)stream, k);
  return addk_check_launch("affine_sum_fwd");
}

extern "C" int addk_affine_sum_bwd(const addk_affine_sum_bwd_args* a, void* stream) {
  ADDK_REQUIRE(a && a->nterm >= 1 && a->nterm <= ADDK_MAX_TERMS && a->P > 0 && a->C > 0 && a->C <= 1024, "affine_sum_bwd: bad args");
  ADDK_REQUIRE(a->dout && a->lddo >= a->C && (!a->relu_out || (a->out && a->ldo >= a->C)), "affine_sum_bwd: bad dout/out");
  SumK k{};
  k.vec = aligned16(a->dout) && a->lddo % 4 == 0 && (!a->relu_out || (aligned16(a->out) && a->ldo % 4 == 0));
  for (int i = 0; i < a->nterm; ++i) {
    ADDK_REQUIRE(a->term[i].x && a->term[i].ld >= a->C && a->term[i].C == a->C, "affine_sum_bwd: bad term %d", i);
    k.term[i] = a->term[i]; k.g[i] = a->g[i]; k.ldg[i] = a->ldg[i]; k.acc[i] = a->accumulate[i]; k.dab[i] = (double*)a->dab[i];
    ADDK_REQUIRE(!a->g[i] || a->ldg[i] >= a->C, "affine_sum_bwd: short ldg %d", i);
    if (!src_vec_ok(a->term[i]) || (a->g[i] && (!aligned16(a->g[i]) || a->ldg[i] % 4))) k.vec = 0;
  }
  k.nterm = a->nterm; k.P = a->P; k.C = a->C; k.dout = a->dout; k.lddo = a->lddo; k.fout = a->out; k.ldfo = a->ldo; k.relu_out = a->relu_out;
  EwMap m = ew_map(a->C); k.nq = m.nq; k.npl = m.npl;
  size_t sh = (size_t)m.npl * m.nq * 4 * 2 * sizeof(double);
  const int vec2 = 1;
  bool vec_ok = vec2 && k.vec && a->C % 4 == 0 && a->C == m.nq * 4;
  for (int i = 0; i < a->nterm && vec_ok; ++i) if (a->term[i].a && (!aligned16(a->term[i].a) || !aligned16(a->term[i].b))) vec_ok = false;
  const dim3 grid(ew_rows(a->P, a->C));
  if (vec_ok) {
    const size_t shv = sh * a->nterm;       // one panel for all terms: 64 KB at most (4 terms x 16 KB)
    bool extra = a->relu_out != 0;
    for (int i = 0; i < a->nterm; ++i) extra = extra || (a->g[i] && a->accumulate[i]);
    auto launch = [&](auto plain, auto full) {
      if (extra) hipLaunchKernelGGL(full, grid, dim3(256), shv, (hipStream_t)stream, k);
      else hipLaunchKernelGGL(plain, grid, dim3(256), shv, (hipStream_t)stream, k);
    };
    switch (a->nterm) {
      case 1: launch(affine_sum_bwd_vec_kernel<1, false>, affine_sum_bwd_vec_kernel<1, true>); break;
      case 2: launch(affine_sum_bwd_vec_kernel<2, false>, affine_sum_bwd_vec_kernel<2, true>); break;
      case 3: launch(affine_sum_bwd_vec_kernel<3, false>, affine_sum_bwd_vec_kernel<3, true>); break;
      default: launch(affine_sum_bwd_vec_kernel<4, false>, affine_sum_bwd_vec_kernel<4, true>); break;
    }
    return addk_check_launch("affine_sum_bwd");
  }
  hipLaunchKernelGGL(affine_sum_bwd_kernel, grid, dim3(256), sh, (hipStream_t)stream, k);
  return addk_check_launch("affine_sum_bwd");
}

extern "C" int addk_bn_bwd_apply(const addk_bn_apply_item* it, void* stream) {
  ADDK_REQUIRE(it && it->g && it->out && it->P > 0 && it->C > 0 && it->C <= 1024 && it->ldg >= it->C && it->ldo >= it->C &&
               (!it->c2 || (it->x && it->ldx >= it->C)), "bn_bwd_apply: bad args");
  ADDK_REQUIRE((it->c1 == nullptr) == (it->c2 == nullptr), "bn_bwd_apply: c1/c2 come together");
  int vec = aligned16(it->g) && aligned16(it->out) && it->ldg % 4 == 0 && it->ldo % 4 == 0 && it->C % 4 == 0 &&
            (!it->x || (aligned16(it->x) && it->ldx % 4 == 0)) && (!it->mean || aligned16(it->mean)) &&
            (!it->c1 || (aligned16(it->c1) && aligned16(it->c2)));
  EwMap m = ew_map(it->C);
  const dim3 grid(ew_blocks(it->P, m.npl));
  if (vec && it->C == m.nq * 4 && it->c2) hipLaunchKernelGGL(bn_bwd_apply_vec_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *it, m.nq, m.npl);
  else if (vec && it->C == m.nq * 4) hipLaunchKernelGGL(bn_bwd_apply_vec_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *it, m.nq, m.npl);
  else hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, *it, m.nq, m.npl, vec);
  return addk_check_launch("bn_bwd_apply");
}

extern "C" int addk_fill(float* p, int64_t n, float v, void* stream) {
  ADDK_REQUIRE(p && n >= 0, "fill: bad args");
  if (n == 0) return 0;
  int b = cdiv(n, 1024); if (b > 2048) b = 2048;
  hipLaunchKernelGGL(fill_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, p, (long)n, v);
  return addk_check_launch("fill");
}

extern "C" int addk_sgd_step(float* p, const float* g, float* buf, int64_t n, const float* lr_dev, float momentum, float weight_decay,
                             int32_t nesterov, int32_t first, float gscale, void* stream) {
  ADDK_REQUIRE(p && g && buf && lr_dev && n > 0, "sgd_step: bad args");
  int b = cdiv(n, 1024); if (b > 4096) b = 4096;
  hipLaunchKernelGGL(sgd_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, p, g, buf, (long)n, lr_dev, momentum, weight_decay, nesterov,
                     first, gscale);
  return addk_check_launch("sgd_step");
}

// every item must be vector-aligned (include/addk.h)
extern "C" int addk_bn_bwd_apply_batch(const addk_bn_apply_item* dev_table, int32_t n, int64_t max_P, void* stream) {
  ADDK_REQUIRE(dev_table && n > 0 && max_P > 0, "bn_bwd_apply_batch: bad args");
  long b = cdiv(max_P, 6); if (b > 2048) b = 2048; if (b < 1) b = 1;
  hipLaunchKernelGGL(bn_bwd_apply_batch_kernel, dim3((unsigned)b, n), dim3(256), 0, (hipStream_t)stream, dev_table);
  return addk_check_launch("bn_bwd_apply_batch");
}
