// wgrad.h — what the weight-gradient kernels share (wgrad_pix.hip, wgrad_h3.hip, wgrad_hk.hip, wgrad_rs.hip; host side and reduce
// kernels: wgrad.hip): the launch descriptor, the work-list prologue, the tile and LDS image geometry, the split-precision arithmetic with its
// running scales, and the transposed fragment read, product terms and input prologue of the split-precision halo-patch kernels.
//     dW[co][tap][c] = sum_p dy[p, co] * Z[p @ tap, c],   Z = relu?(a*x+b) recomputed on the fly.
#pragma once
#include <string.h>
#include "common.h"

struct WgK {
  const float* dy; int lddy; int Cout;
  int N, H, W, OH, OW, KH, KW, stride, pad, dil;
  addk_src src;
  float* ws;
  int taps, nzt, nyt;      // tiles: taps, z (input-channel) tiles, y (output-channel) tiles
  int splits; int P; int chunkP;
  int vecY, vecZ;
  // reduction target (used by the batched reduce)
  float* dw; int ldw, cin_total, w_choff, accumulate;
};

// The kernel of a launch key (kind, cty, ctz) in a precision mode.  Every family file exposes its instantiations through plain functions
// (wg_variant_*), so no kernel symbol crosses files.
typedef void (*WgFn)(const WgK, const WgK*, const int4*);
struct WgVariant { WgFn fn; unsigned threads; size_t lds; };
WgVariant wg_variant_pix(bool batch, int cty, int ctz);              // wgrad_pix.hip: wgrad_kernel<cty, ctz>
WgVariant wg_variant_os(bool batch, int ty);                         //   wgrad_os_kernel<ty, 2 / 3 / 2> for ty = 4 / 3 / 2
WgVariant wg_variant_st(bool batch);                                 //   wgrad_st_kernel
WgVariant wg_variant_h3(bool batch, int cty, int ctz, int np);       // wgrad_h3.hip: wgrad_h3_kernel<cty / 4> (np = 0), wgrad_h3b_kernel<cty / 4, np, ctz>
WgVariant wg_variant_h1(bool batch, int np);                         //   wgrad_h1b_kernel<np>
WgVariant wg_variant_hk(bool batch, int cty, int ctz, int np);       // wgrad_hk.hip: wgrad_hk_kernel<ctz, cty> (np = 0), wgrad_hkb_kernel<ctz, cty, np>
WgVariant wg_variant_rs(bool batch, int cty, int ctz, int mode);     // wgrad_rs.hip: wgrad_rs_kernel<cty, ctz>, the split-fp16 form in mode 1

namespace {

template <WgFn F> WgVariant wg_dyn_lds(unsigned threads, size_t lds) {
  addk_dyn_lds<F>();
  return {F, threads, lds};
}

// Descriptor of this block's convolution, BY VALUE (scalar registers, loaded once): either the kernel argument or the
// batch table's entry with its pointers declared global (common.h, gptr).
template <bool BATCH>
__device__ __forceinline__ WgK wg_desc(const WgK& pv, const WgK* __restrict__ ops, int op) {
  if (!BATCH) return pv;
  WgK k = ops[op];
  k.dy = gptr(k.dy); k.src.x = gptr(k.src.x); k.src.a = gptr(k.src.a); k.src.b = gptr(k.src.b); k.ws = gptr(k.ws); k.dw = gptr(k.dw);
  return k;
}

// Work-list prologue of every main-loop kernel.  Batched form: `work[b] = (op, bx, by, -)` lets ONE launch cover the weight gradients of many
// convolutions (they are mutually independent and individually too small to fill 256 CUs); the plain launch takes its block from the grid.
template <bool BATCH>
__device__ __forceinline__ WgK wg_block(const WgK& pv, const WgK* __restrict__ ops, const int4* __restrict__ work, int& op, int& blk_x, int& blk_y) {
  op = 0; blk_x = blockIdx.x; blk_y = blockIdx.y;
  if (BATCH) {      // wave-uniform: keep the descriptor in scalar registers like a kernel argument
    const int4 wk = work[blockIdx.x];
    op = __builtin_amdgcn_readfirstlane(wk.x); blk_x = __builtin_amdgcn_readfirstlane(wk.y); blk_y = __builtin_amdgcn_readfirstlane(wk.z);
  }
  return wg_desc<BATCH>(pv, ops, op);
}

constexpr int KP = 64;
constexpr int ldpad(int bc) { return (bc % 32 == 16) ? bc : bc + 16; }
constexpr int H3_KP = 64;
constexpr int H3_ZW = H3_KP + 2 * 18;       // widest patch row (dilation 18)
constexpr int H1_TP = 4;
constexpr int HK_ZW = H3_KP + 4 * 2;       // widest patch row: 5x5, dilation 2
constexpr int HKB_ZWP = 72;                 // patch row pitch in pixels: 64 + 4 * 2 (5x5, dilation 2), a multiple of 8
constexpr int RS_T = 64;             // LDS tile edge for the cross-wave combine (channels)
constexpr int RS_U = 4;              // k-steps per unrolled batch

typedef short wg_s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) wg_s16x4 wg_lds_s16x4;
__device__ __forceinline__ unsigned wg_bf16_hi(float x) { return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float wg_bf16_f(unsigned b) { return __uint_as_float(b << 16); }
typedef float wg_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 wg_bf16x2 __attribute__((ext_vector_type(2)));
// two fp32 -> one packed bf16 pair (round to nearest even): a single v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned wg_cvt2(float a, float b) {
  const wg_f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, wg_bf16x2));
}
// [r5] NP = 2 is the split-fp16 form (common.h / conv3b.h): both operands of a weight gradient are activations, so BOTH carry a running power-of-two scale
// per workgroup — the largest magnitude of each staged segment goes through LDS in front of the barrier that ends the matrix phase (wg_publish_max), behind it
// every thread folds the waves' maxima into the two scales and, when a larger segment arrives, multiplies the accumulators by the exact ratio (wg_rescale).
// The partial tiles leave the kernel unscaled.
struct WgScale { int kfy, kfz; };
__device__ __forceinline__ void wg_publish_max(unsigned* wmx, int nw, int wave, int lane, unsigned my, unsigned mz) {
  my = wave_umax(my); mz = wave_umax(mz);
  if (lane == 0) { wmx[wave] = my; wmx[nw + wave] = mz; }
}
// returns the factor for the accumulators (1 = unchanged)
__device__ __forceinline__ float wg_rescale(const unsigned* wmx, int nw, WgScale& sc) {
  unsigned my = 0, mz = 0;
  for (int w = 0; w < nw; ++w) { const unsigned a = wmx[w], b = wmx[nw + w]; my = a > my ? a : my; mz = b > mz ? b : mz; }
  const int wy = f16_scale_field(my), wz = f16_scale_field(mz);
  int sh = 0;
  if (sc.kfy == 0) sc.kfy = wy; else if (wy < sc.kfy) { sh += wy - sc.kfy; sc.kfy = wy; }
  if (sc.kfz == 0) sc.kfz = wz; else if (wz < sc.kfz) { sh += wz - sc.kfz; sc.kfz = wz; }
  if (sh == 0) return 1.f;
  const int rf = 127 + sh;
  return rf > 0 ? __uint_as_float((unsigned)rf << 23) : 0.f;
}
__device__ __forceinline__ float wg_pow2(int field) { return __uint_as_float((unsigned)field << 23); }
__device__ __forceinline__ float4 wg_mul4(float4 v, float s) { v.x *= s; v.y *= s; v.z *= s; v.w *= s; return v; }
template <int NP>
__device__ __forceinline__ void wg_split4(const float4 v, uint2 (&pl)[NP]) {
  if constexpr (NP == 2) { split4h(v, pl); return; }
  float a = v.x, b = v.y, c = v.z, d = v.w;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const unsigned p0 = wg_cvt2(a, b), p1 = wg_cvt2(c, d);
    pl[k] = make_uint2(p0, p1);
    if (k + 1 < NP) {
      a -= __uint_as_float(p0 << 16); b -= __uint_as_float(p0 & 0xffff0000u);
      c -= __uint_as_float(p1 << 16); d -= __uint_as_float(p1 & 0xffff0000u);
    }
  }
}
// byte offset of pixel row p inside a [pixel][16 ch] bf16 tile image
__device__ __forceinline__ int wg_prow(int p) { return (p << 5) ^ (((p >> 3) & 1) << 7); }

// ---- pieces of the split-precision halo-patch kernels (wgrad_h3b / h1b / hkb) ----
// The MFMA's K axis is the PIXEL index here, while both operands arrive pixel-major ([pixel][channel] rows from NHWC
// memory): the staged LDS images stay pixel-major — per 16-channel tile [pixel][16 ch] bf16, 32-byte rows, 8-byte writes —
// and the fragments are fetched with the hardware transposing read ds_read_b64_tr_b16 (a 16-lane group reads a
// 4-pixel x 16-channel block and every lane receives ITS channel's four pixels): two reads give a lane the 8 consecutive
// pixels of its channel that the 16x16x32 operand wants, for dy and for every tap-shifted window of the activation rows
// alike (any pixel shift is a row offset: always aligned).  A pixel's row sits at 32*p with the two 128-byte halves of
// every 8-pixel block swapped when bit 3 of p is set: the two groups of a half-wave (pixels p..p+3 and p+8..p+11) then hit
// disjoint banks for every shift (scripts/tr_read_probe.hip checks the lane map and the operand on the device).
// Lane 16 kq + 4 tq + tp supplies (pixel row tq of the block, channels 4 tp .. 4 tp + 3); lrow = 8 kq + tq is the lane's pixel row inside a 32-pixel k-step.
// Fragment of one 32-pixel k-step: 8 consecutive pixels of this lane's channel = two transposed reads, per plane.
template <int NP>
__device__ __forceinline__ void wg_tr_read(const unsigned char* base, int plane_bytes, int pix0, int lrow, int tp, wg_bf16x8* f) {
  const int o0 = wg_prow(pix0 + lrow) + 8 * tp, o1 = wg_prow(pix0 + lrow + 4) + 8 * tp;
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    const wg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4*)(base + m * plane_bytes + o0));
    const wg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4*)(base + m * plane_bytes + o1));
    // whole-register reinterpretation: building the fragment element by element from the two results is miscompiled by
    // hipcc 7.2 (it drops the upper dword of each 64-bit result: scripts/tr_read_probe.hip)
    struct { wg_s16x4 a, b; } pr = {lo, hi};
    f[m] = __builtin_bit_cast(wg_bf16x8, pr);
  }
}
// The product terms of accumulator column j (one tap or input tile), smallest first, the NT accumulator chains interleaved term by term:
// NP = 2 (fp16 planes) (1,0) (0,1) (0,0); NP = 3 (bf16 planes) (2,0) (0,2) (1,1) (1,0) (0,1) (0,0).
template <int NP, int NT, int NJ>
__device__ __forceinline__ void wg_terms(f32x4 (&c)[NT][NJ], int j, const wg_bf16x8 (&y)[NT][NP], const wg_bf16x8* z) {
#define WG_TERM(YI, ZI) _Pragma("unroll") for (int i = 0; i < NT; ++i) c[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y[i][YI], z[ZI], c[i][j], 0, 0, 0);
#define WG_TERMH(YI, ZI) _Pragma("unroll") for (int i = 0; i < NT; ++i) c[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, y[i][YI]), __builtin_bit_cast(f16x8, z[ZI]), c[i][j], 0, 0, 0);
  if constexpr (NP == 2) { WG_TERMH(1, 0) WG_TERMH(0, 1) WG_TERMH(0, 0) } else {
  if (NP == 3) { WG_TERM(2, 0) WG_TERM(0, 2) WG_TERM(1, 1) }
  WG_TERM(1, 0) WG_TERM(0, 1) WG_TERM(0, 0) }
#undef WG_TERM
#undef WG_TERMH
}
// NP = 2: every accumulator times wg_rescale's factor (exact) when a larger segment arrived
template <int NI, int NJ>
__device__ __forceinline__ void wg_acc_rescale(f32x4 (&acc)[NI][NJ], float r) {
  if (r != 1.f) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] *= r;
  }
}
// the activation on its way in: lazy affine (BatchNorm), ReLU, then the validity mask (zero padding comes after both)
__device__ __forceinline__ float4 wg_zpro(float4 v, const float4 za, const float4 zb, bool zaff, bool zrelu, bool ok) {
  if (zaff) { v.x = fmaf(za.x, v.x, zb.x); v.y = fmaf(za.y, v.y, zb.y); v.z = fmaf(za.z, v.z, zb.z); v.w = fmaf(za.w, v.w, zb.w); }
  if (zrelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
  return v;
}
constexpr size_t wg_h1b_lds(int np) { return (size_t)np * ((128 / 16) + H1_TP) * (H3_KP * 32 + 32) + 64; }      // + the waves' maxima (NP = 2)
constexpr size_t wg_h3b_lds(int nt, int np, int ng) { return (size_t)np * ((64 * nt / 16) * (H3_KP * 32 + 32) + ng * (3 * 104 * 32 + (ng > 1 ? 64 : 0))) + 64; }      // + the waves' maxima (NP = 2)
constexpr size_t wg_hkb_lds(int ks, int ct, int np) { return (size_t)np * ((size_t)ct * (H3_KP * 32 + 32) + (size_t)ks * HKB_ZWP * 32) + 64; }      // + the waves' maxima (NP = 2)

// operand fragment of the register-streaming kernels (wgrad_rs_kernel; wgrad_st_kernel loads its dy with it): LAY components of one vector load
template <int LAY> struct RsFrag { float v[LAY]; };

template <int LAY>
__device__ __forceinline__ RsFrag<LAY> rs_load(const float* base, int li, bool ok4, bool ok2, bool ok1) {
  RsFrag<LAY> f;
  if (LAY == 4) {
    const float4 x = ld4(base + (ok4 ? 4 * li : 0));
    f.v[0] = ok4 ? x.x : 0.f; f.v[1] = ok4 ? x.y : 0.f; f.v[2] = ok4 ? x.z : 0.f; f.v[3 % LAY] = ok4 ? x.w : 0.f;
  } else {
    typedef float rs_f32x2 __attribute__((ext_vector_type(2)));
    const rs_f32x2 x = *(const __attribute__((address_space(1))) rs_f32x2*)(base + (ok2 ? 2 * li : 0));
    const float y = ((const gfloat*)base)[ok1 ? 32 + li : 0];
    f.v[0] = ok2 ? x.x : 0.f; f.v[1] = ok2 ? x.y : 0.f; f.v[2] = ok1 ? y : 0.f;
  }
  return f;
}

}  // namespace
