// Device and host code that more than one family of logits heads uses (ce_up.h: the training head's kernel, instantiated by loss_up.hip, with
// hard example mining, and by loss_shape.hip, the focal and label-smoothed forms;
// dice_up.hip: the soft-Dice term's reduction; score_up.hip: the validation scoring head and the exit profile; label_up.hip: the
// label-map heads and the exit gate; calib_up.hip: the calibration head; loss.hip: the drop-in criterion): the block sum and the second-stage sum of partials, the argument prefix and pixel loader of the decoder's
// low-resolution NHWC logits, the up-sampling walk of the gather heads with its grid, the label store, and the last-arriver tail of
// the gate-style heads.  Everything sits in the unit's anonymous namespace.
#pragma once
#include <math.h>
#include <string>
#include <type_traits>
#include "common.h"
#include "bnfin.h"

namespace {

// The class counts the heads are compiled for, one list per group of heads.  Every head kernel is a template on the class count CC; the
// dispatchers below turn a run-time C into it, and a further count is one more entry of a list.
//   HeadClasses: the training heads (ce_up_kernel in all its forms, ohem_loss_kernel, the Dice reduction), the label head and the compile-time
//                form of ce_kernel: Cityscapes (19) and Pascal VOC (21), the reference's two datasets.
//   GateClasses: the scoring, profile, calibration, gate and multi-view heads: 19 (DESIGN section 27 says why not yet 21).
struct HeadClasses { static constexpr int v[] = {19, 21}; };
struct GateClasses { static constexpr int v[] = {19}; };
template <class L> constexpr int nclasses() { return sizeof(L::v) / sizeof(L::v[0]); }
template <class L> constexpr int cmax(int i = 0) { return i == nclasses<L>() ? 0 : (L::v[i] > cmax<L>(i + 1) ? L::v[i] : cmax<L>(i + 1)); }
constexpr int HEAD_CMAX = cmax<HeadClasses>();                    // what a fixed-size class table has to hold (dice_up.hip asserts it)
// f(cc) with decltype(cc)::value == C for a C of the list L (true), or nothing (false): the one place where a launcher gets its CC
template <class L, int I = 0, class F>
bool classes_of(int C, F&& f) {
  if constexpr (I < nclasses<L>()) {
    if (C == L::v[I]) { f(std::integral_constant<int, L::v[I]>{}); return true; }
    return classes_of<L, I + 1>(C, f);
  } else {
    return false;
  }
}
template <class F> bool head_classes(int C, F&& f) { return classes_of<HeadClasses>(C, f); }
template <class F> bool gate_classes(int C, F&& f) { return classes_of<GateClasses>(C, f); }
bool head_class_ok(int C) { return head_classes(C, [](auto) {}); }
bool gate_class_ok(int C) { return gate_classes(C, [](auto) {}); }
// "19 classes (or 21)": a list as the error texts name it, here and in Python (_lib.head_classes_text builds the same words from the
// exported list: addk_head_classes, addk_gate_head_classes)
template <class L> std::string classes_text() {
  std::string s = std::to_string(L::v[0]) + " classes";
  for (int i = 1; i < nclasses<L>(); ++i) s += (i == 1 ? " (or " : ", ") + std::to_string(L::v[i]);
  return nclasses<L>() > 1 ? s + ")" : s;
}
template <class L> int classes_out(int32_t* out, int32_t cap) {
  for (int i = 0; out && i < nclasses<L>() && i < cap; ++i) out[i] = L::v[i];
  return nclasses<L>();
}
std::string head_classes_text() { return classes_text<HeadClasses>(); }
std::string gate_classes_text() { return classes_text<GateClasses>(); }

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

// second stage of a loss-style head: the partials of one launch in a fixed order.  A template only so that a unit emits it when it
// launches it (loss.hip, loss_up.hip): a kernel of the anonymous namespace is otherwise compiled into every unit that includes this header
template <int = 0>
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

// What every head on the low-resolution logits shares (the loss head, the scoring head, the exit gate and those that followed): the
// argument prefix UpSrc, the pixel loader load_px and its vector-load predicate px_vec_ok; the gather heads also share their walk, scu_walk.
struct UpSrc { const float* x; int ld; int N, H, W, OH, OW; };      // NHWC logits, pixel stride ld, (H, W) -> (OH, OW)
template <class A> UpSrc up_src(const A* a) { return UpSrc{a->logits, a->ld, a->N, a->H, a->W, a->OH, a->OW}; }

constexpr int cpad(int cc) { return (cc + 3) / 4 * 4; }              // channels incl. the padding of a 16-byte-aligned pixel row
// 16-byte loads of a pixel's cpad(CC) channels: stride and base keep every pixel aligned and the padding exists.  The host's
// choice of a VEC kernel; ce_up_kernel evaluates the same three terms on the device
template <int CC> bool px_vec_ok(const float* x, int ld) { return ld % 4 == 0 && ld >= cpad(CC) && aligned16(x); }
// The host's VEC choice: the two instantiations of a head have one signature, the predicate's result picks (workgroups of 256)
template <class A>
void launch_vec(bool vec, void (*kv)(A), void (*ks)(A), dim3 grid, hipStream_t st, const A& a) {
  hipLaunchKernelGGL(vec ? kv : ks, grid, dim3(256), 0, st, a);
}
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
// The LDS histogram of a head that walks columns: a thread merges the run of equal keys of its column (key < 0: not counted) before
// it touches LDS, and after the walk it flushes the run that is still pending
__device__ __forceinline__ void run_flush(unsigned* hist, int key, unsigned run) { if (key >= 0) atomicAdd(&hist[key], run); }
__device__ __forceinline__ void run_count(unsigned* hist, int& key, unsigned& run, int k) {
  if (k != key) { run_flush(hist, key, run); key = k; run = 0; }
  ++run;
}
// se = Σe, sx = Σe·d over d = z - mx, e = exp(d): loss (log se) and entropy (log se - sx/se) of a pixel from one sweep
template <int CC>
__device__ __forceinline__ void exp_sweep(const float (&z)[CC], float mx, float& se, float& sx) {
  se = 0.f; sx = 0.f;
#pragma unroll
  for (int c = 0; c < CC; ++c) { const float d = z[c] - mx; const float e = __expf(d); se += e; sx += e * d; }
}
// the sweep of the tempered heads, softmax(z·it): d = (z - mx)·it, the rest as above, so it = 1.0f leaves exp_sweep's bits
template <int CC>
__device__ __forceinline__ void exp_sweep_t(const float (&z)[CC], float mx, float it, float& se, float& sx) {
  se = 0.f; sx = 0.f;
#pragma unroll
  for (int c = 0; c < CC; ++c) { const float d = (z[c] - mx) * it; const float e = __expf(d); se += e; sx += e * d; }
}

// the launch grid of the two gather heads (one workgroup per tile and image) and its workgroup count, which sizes their workspaces
dim3 scu_grid(int N, int OH, int OW) { return dim3(cdiv(OW, SCU_W), cdiv(OH, SCU_WAVES * SCU_R), N); }
long scu_blocks(int N, int OH, int OW) { const dim3 g = scu_grid(N, OH, OW); return (long)(int)g.z * (int)g.y * (int)g.x; }
// the walk's limits alone, then with the class count of a head of either list
bool scu_geom_ok(int N, int H, int W, int OH, int OW) {
  if (N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return false;
  return N <= 65535 && scu_grid(N, OH, OW).y <= 65535 && scu_blocks(N, OH, OW) < (1L << 30);
}
bool scu_ok(int N, int H, int W, int OH, int OW, int C) { return gate_class_ok(C) && scu_geom_ok(N, H, W, OH, OW); }
bool scu_head_ok(int N, int H, int W, int OH, int OW, int C) { return head_class_ok(C) && scu_geom_ok(N, H, W, OH, OW); }

typedef __attribute__((address_space(1))) uint8_t gu8;
__device__ __forceinline__ void label_px(const uint8_t* lut, uint8_t* labels, long pix, int am) {
  ((gu8*)labels)[pix] = lut ? ((const gu8*)lut)[am] : (uint8_t)am;
}

// The workspace of a gate-style head with nk counts per workgroup, [ticket, 16 bytes][nblk floats][nblk x nk counts], image-major, and
// what both heads' argument structs say about it and about the normalisation.  The divisor is log 19 at EVERY class count, not log C:
// the reference calls normalized_shannon_entropy without num_class (modeling/ADD.py:474), so its gate divides by log 19 whatever the
// dataset, and so does the stand-alone path (heads._gate_alone)
int64_t up_ws_bytes(int N, int OH, int OW, int nk) { return 16 + (4 + 4 * (int64_t)nk) * scu_blocks(N, OH, OW); }
template <class K> void up_tail_fill(K& k, void* ws, int N, int OH, int OW) {
  const dim3 grid = scu_grid(N, OH, OW);
  k.nblk_img = (int)(grid.x * grid.y);
  k.counter = (unsigned*)ws;
  k.part = (float*)((char*)ws + 16);
  k.cnt = (unsigned*)(k.part + (long)N * k.nblk_img);
  k.npix = (double)OH * (double)OW; k.ent_div = log(19.0) * k.npix;
}

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

}  // namespace
