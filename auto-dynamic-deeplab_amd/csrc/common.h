// Shared device/host helpers for the addk gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "addk.h"

void addk_set_error(const char* fmt, ...);
int addk_check_launch(const char* what);
int addk_env(const char* name, int dflt);      // util.cpp: the library's only getenv (integer switches, read once under a lock)
int addk_env_math(int dflt);

#define ADDK_REQUIRE(cond, ...)                    \
  do {                                             \
    if (!(cond)) {                                 \
      addk_set_error(__VA_ARGS__);                 \
      return ADDK_ERR_INVALID;                     \
    }                                              \
  } while (0)

// arithmetic of the halo-patch convolutions when neither ADDK_MATH nor addk_set_conv_precision says otherwise (conv.hip)
#ifndef ADDK_DEFAULT_PRECISION
#define ADDK_DEFAULT_PRECISION 1
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// A source can use 16-byte accesses when its base, pixel stride and channel count allow it.
static inline bool src_vec_ok(const addk_src& s) {
  return aligned16(s.x) && (s.ld % 4 == 0) && (s.C % 4 == 0) && (!s.a || aligned16(s.a)) && (!s.b || aligned16(s.b));
}

// Pointers that reach a kernel through a descriptor TABLE in device memory (the batched launches) carry no address-space
// information: the compiler emits flat_load / flat_store for them, which count on lgkmcnt together with the LDS traffic
// (every wait for a fragment read then also waits for the global loads in flight) and probe the apertures.  gptr() states
// that a pointer is global memory; ld4 / st4 (and everything built on them) are GLOBAL accesses — LDS staging uses
// lds_ld4 / lds_st4.
// gfloat* / gdouble*: explicitly-global views for the scalar accesses.
template <class T> __device__ __forceinline__ T* gptr(T* p) { return (T*)(__attribute__((address_space(1))) T*)p; }
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) double gdouble;
typedef float addk_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p) {
  const addk_f32x4 v = *(const __attribute__((address_space(1))) addk_f32x4*)p;
  return make_float4(v.x, v.y, v.z, v.w);
}
// 16-byte load at a 32-bit BYTE offset from a wave-uniform base: the `global_load_dwordx4 v, v_off, s[base]` form (one address register, no 64-bit
// vector arithmetic) — for loops whose base moves in scalar registers while every thread's offset stays put
__device__ __forceinline__ float4 ld4so(const float* sbase, unsigned byte_off) {
  const addk_f32x4 v = *(const __attribute__((address_space(1))) addk_f32x4*)((const __attribute__((address_space(1))) char*)sbase + byte_off);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float* p, float4 v) {
  const addk_f32x4 t = {v.x, v.y, v.z, v.w};
  *(__attribute__((address_space(1))) addk_f32x4*)p = t;
}
// Write-through 16-byte store (`sc1`: the bytes leave the XCD's L2 as they are written instead of waiting, dirty, for the end-of-kernel
// write-back — MI355X_MICROARCH.md, 'stores of each flavour' / 'publish-large').  For launches whose output is consumed by the NEXT kernel
// (another XCD's L2 never sees it anyway).  Measured on the fused SepConv half: 0.5-0.9 us per launch (profiles/r04_sepf_phases.txt); as a
// blanket replacement of st4 it was slower (36.0 vs 35.6 ms per step: profiles/r04_ab_store_wt_global_rejected.txt) — only sepf.hip uses it.
// The "memory" clobber is what keeps the compiler from moving dependent memory operations across a store it cannot see.
__device__ __forceinline__ void st4_wt(float* p, float4 v) {
  const addk_f32x4 t = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"((__attribute__((address_space(1))) addk_f32x4*)p), "v"(t) : "memory");
}
__device__ __forceinline__ float4 lds_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void lds_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// guarded 4-element load: elements with index >= n read as 0
__device__ __forceinline__ float4 ld4g(const float* p, int n, bool vec) {
  if (vec && n >= 4) return ld4(p);
  float4 v = zero4();
  const gfloat* g = (const gfloat*)p;
  if (n > 0) v.x = g[0];
  if (n > 1) v.y = g[1];
  if (n > 2) v.z = g[2];
  if (n > 3) v.w = g[3];
  return v;
}
__device__ __forceinline__ void st4g(float* p, float4 v, int n, bool vec) {
  if (vec && n >= 4) { st4(p, v); return; }
  gfloat* g = (gfloat*)p;
  if (n > 0) g[0] = v.x;
  if (n > 1) g[1] = v.y;
  if (n > 2) g[2] = v.z;
  if (n > 3) g[3] = v.w;
}

// lazy prologue z = relu?(a*x+b) on 4 channels; lanes >= n stay 0
__device__ __forceinline__ float4 prologue4(float4 x, const float* a, const float* b, int c, int n, bool relu, bool vec) {
  if (a) {
    float4 av = ld4g(a + c, n, vec), bv = ld4g(b + c, n, vec);
    x.x = fmaf(av.x, x.x, bv.x); x.y = fmaf(av.y, x.y, bv.y);
    x.z = fmaf(av.z, x.z, bv.z); x.w = fmaf(av.w, x.w, bv.w);
  }
  if (relu) { x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f); }
  if (n < 4) { if (n < 1) x.x = 0.f; if (n < 2) x.y = 0.f; if (n < 3) x.z = 0.f; x.w = 0.f; }
  return x;
}

// Bilinear source index of F.interpolate(mode='bilinear', align_corners=False) in fp32, as ATen's area_pixel_compute_source_index:
//     scale = in/out;  src = max(0, scale*(dst+0.5)-0.5);  i0 = floor(src); i1 = min(i0+1, in-1); l1 = src-i0.
// One definition for the stand-alone resize kernels (resize.hip) and for the 1x1 convolutions that sample their input on the fly
// (pw.hip, addk_src.rs_hw): the two forms are bit-identical by construction.
__device__ __forceinline__ void src_index(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}
__device__ __forceinline__ float4 lerp4(float4 v00, float4 v01, float4 v10, float4 v11, float lh0, float lh1, float lw0, float lw1) {
  float4 o;
  o.x = lh0 * (lw0 * v00.x + lw1 * v01.x) + lh1 * (lw0 * v10.x + lw1 * v11.x);
  o.y = lh0 * (lw0 * v00.y + lw1 * v01.y) + lh1 * (lw0 * v10.y + lw1 * v11.y);
  o.z = lh0 * (lw0 * v00.z + lw1 * v01.z) + lh1 * (lw0 * v10.z + lw1 * v11.z);
  o.w = lh0 * (lw0 * v00.w + lw1 * v01.w) + lh1 * (lw0 * v10.w + lw1 * v11.w);
  return o;
}

__device__ __forceinline__ float get4(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ void set4(float4& v, int e, float f) { if (e == 0) v.x = f; else if (e == 1) v.y = f; else if (e == 2) v.z = f; else v.w = f; }

// ---- split-fp16 arithmetic ("f16x3": conv3b.h, wgrad.hip) -------------------------------------------------------------------------------------
// x = h + l with h = fp16(x), l = fp16(x - h); products as l*wh + h*wl + h*wh on the fp16 matrix pipe; operands scaled by exact powers of two into fp16's range
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split4h(const float4 v, uint2 (&pl)[2]) {
  const f16x2 h01 = {(_Float16)v.x, (_Float16)v.y}, h23 = {(_Float16)v.z, (_Float16)v.w};
  const f16x2 l01 = {(_Float16)(v.x - (float)h01[0]), (_Float16)(v.y - (float)h01[1])}, l23 = {(_Float16)(v.z - (float)h23[0]), (_Float16)(v.w - (float)h23[1])};
  pl[0] = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
  pl[1] = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
}
// 8 scaled floats -> the two fp16 planes of a packed weight fragment (16 bytes each)
__device__ __forceinline__ void split8h(const float (&v)[8], uint4& ph, uint4& pl) {
  uint2 a[2], b[2];
  split4h(make_float4(v[0], v[1], v[2], v[3]), a); split4h(make_float4(v[4], v[5], v[6], v[7]), b);
  ph = make_uint4(a[0].x, a[0].y, b[0].x, b[0].y); pl = make_uint4(a[1].x, a[1].y, b[1].x, b[1].y);
}
// largest of a non-negative bit pattern (|x| as unsigned: order-preserving) over the 64 lanes, wave-uniform: two quad steps and two row rotations on the DPP
// path, then the four rows by readlane
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
  auto mx = [](unsigned a, int b) { return a > (unsigned)b ? a : (unsigned)b; };
  v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));       // quad_perm [1, 0, 3, 2]
  v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));       // quad_perm [2, 3, 0, 1]
  v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, true));      // row_ror:4
  v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true));      // row_ror:8
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
  const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}
// ---- statistics tail of the forward kernels (sepf.hip, pw.hip): totals of V per-lane values over the 16 pixel lanes of a DPP row ----------------
// The all-reduce butterfly these kernels ended in computes, per value, T1[i] = x[i] + x[i^1], T2[i] = T1[i] + T1[i^2], T3[i] = T2[i] + T2[i^4],
// T4 = T3[i] + T3[i^8] in every lane i, and lane 0 kept T4.  IEEE addition is commutative, so every lane of a 2^m-lane group holds the same
// bits at level m and any lane that adds the same two partial sums gets them too.  rs16() is the reduce-scatter of that tree: at each level a
// lane keeps half of its remaining values and adds the partner's partial sums of those — 12 + 6 + 3 + 2 exchanges for 24 values where the
// butterfly takes 96, each a DPP move (two for a double) instead of an LDS permute.  Which half a lane keeps:
//   level 1 (partner li ^ 1, quad_perm [1,0,3,2]): the upper half if bit 0 ^ bit 2 of li is set
//   level 2 (partner li ^ 2, quad_perm [2,3,0,1]): the upper half if bit 1 ^ bit 2 is set
//   level 3 (partner li ^ 7, row_half_mirror):     the upper half if bit 2 is set.  Bit 2 flips the choices of levels 1 and 2, so the mirrored
//            lane of the other quad holds the same values as li ^ 4 would in a plain layout: the quad sums T2 of both quads meet, as in the tree
//   level 4 (partner li ^ 8, row_ror:8):           the upper half if bit 3 is set
// An odd count leaves one value without a sibling: both lanes add it (a plain butterfly step) and the lane that keeps the lower half owns it.
// Written as unrolled templates with constant indices: as a loop over the levels the value array lands in scratch (conv3b.h, rs32).
template <int CTL>
__device__ __forceinline__ float rs16_from(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTL, 0xF, 0xF, true)); }
template <int CTL>
__device__ __forceinline__ double rs16_from(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
template <int NIN, int CTL, typename T>
__device__ __forceinline__ void rs16_step(const T (&in)[NIN], T (&out)[(NIN + 1) / 2], const bool upper) {
  constexpr int NOUT = (NIN + 1) / 2;
#pragma unroll
  for (int i = 0; i < NOUT; ++i) {
    if (i + NOUT < NIN) {
      T lo = in[i], hi = in[i + NOUT];
      asm("" : "+v"(lo), "+v"(hi));              // two values, then two selects: without this the compiler selects the INDEX and walks the array with compares
      const T keep = upper ? hi : lo, send = upper ? lo : hi;
      out[i] = keep + rs16_from<CTL>(send);
    } else {
      out[i] = in[i] + rs16_from<CTL>(in[i]);
    }
  }
}
template <int V>
struct Rs16 { static constexpr int N1 = (V + 1) / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2, NF = (N3 + 1) / 2; };   // values a lane holds after each level
template <int V, typename T>
__device__ __forceinline__ void rs16(const T (&v)[V], T (&tot)[Rs16<V>::NF], const int li) {      // (a step writes a new array: in place, one instantiation kept its values in scratch)
  const bool q = (li & 4) != 0;
  T t1[Rs16<V>::N1], t2[Rs16<V>::N2], t3[Rs16<V>::N3];
  rs16_step<V, 0xB1>(v, t1, ((li & 1) != 0) != q);
  rs16_step<Rs16<V>::N1, 0x4E>(t1, t2, ((li & 2) != 0) != q);
  rs16_step<Rs16<V>::N2, 0x141>(t2, t3, q);
  rs16_step<Rs16<V>::N3, 0x128>(t3, tot, (li & 8) != 0);
}
// the value whose row total tot[j] of lane li is after rs16(), -1: a copy that another lane owns
template <int V>
__device__ __forceinline__ int rs16_index(const int j, const int li) {
  int idx = j; bool own = true;
  auto up = [&](const int nin, const bool upper) {
    const int nout = (nin + 1) / 2;
    if (upper) { if (idx + nout < nin) idx += nout; else own = false; }
  };
  const bool q = (li & 4) != 0;
  up(Rs16<V>::N3, (li & 8) != 0); up(Rs16<V>::N2, q); up(Rs16<V>::N1, ((li & 2) != 0) != q); up(V, ((li & 1) != 0) != q);
  return own ? idx : -1;
}

__device__ __forceinline__ unsigned absbits4(const float4 v) {
  return __float_as_uint(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}
// exponent field of the power of two that takes a tensor / chunk of largest magnitude `amax_bits` into [2^14, 2^15): 268 - exponent field, kept in [13, 253]
// (zero / denormal maxima: 2^126; Inf / NaN: 2^-114) so that the scale and its inverse (field 254 - k) are normal numbers
__device__ __forceinline__ int f16_scale_field(unsigned amax_bits) {
  const int want = 268 - (int)(amax_bits >> 23);
  return want > 253 ? 253 : want;
}


// Thread mapping for channel-reducing elementwise kernels: a 256-thread block is viewed as
// npl "pixel lanes" x nq channel quads; a thread keeps its quad for the whole kernel so that
// per-channel sums stay in registers.
struct EwMap { int nq, npl; };
static inline EwMap ew_map(int C) {
  EwMap m; m.nq = (C + 3) / 4; if (m.nq > 256) m.nq = 256; m.npl = 256 / m.nq; if (m.npl < 1) m.npl = 1; return m;
}
// workgroups of such a kernel over P pixels = rows of its partial-sum slabs and workspaces (addk_ew_rows, addk_dw_rows): every block walks at least two
// pixels per lane (>= 4 resident blocks per CU on the level-1 maps), 1024 rows at most
static inline int ew_rows(long P, int C) {
  const long r = P / ((long)ew_map(C).npl * 2);
  return (int)(r < 1 ? 1 : r > 1024 ? 1024 : r);
}

// ---- table-driven batches (the *_batch_prepare entry points of pw.hip, dw.hip, sepf.hip, sepb.hip, resize.hip) ---------------------------------
// The caller asks for the blob size (host_blob = NULL), then has the blob filled: n descriptors `Desc`, one per args[i].  `item` turns one argument struct into its
// descriptor and what the merged launch needs of it (false: not a launch of the batched kernel); every item has item 0's key.  meta[0..3] = key, n, largest grid x,
// largest grid y; *lds = largest dynamic LDS size.  Returns the blob size in bytes.
struct BatchItem { int key, gx, gy; size_t lds; };
template <typename Desc, typename Args, typename Item>
int64_t batch_prepare(const char* what, const Args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta, Item item, size_t* lds = nullptr) {
  if (!a || n <= 0 || !meta) { addk_set_error("%s: bad args", what); return ADDK_ERR_INVALID; }
  const int64_t total = (int64_t)n * sizeof(Desc);
  if (host_blob && blob_bytes < total) { addk_set_error("%s: blob too small", what); return ADDK_ERR_INVALID; }
  BatchItem mx{-1, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    Desc d{}; BatchItem b{};
    if (!item(&a[i], d, b)) { addk_set_error("%s: launch %d does not run on the batched kernel", what, i); return ADDK_ERR_INVALID; }
    if (i == 0) mx.key = b.key;
    if (b.key != mx.key) { addk_set_error("%s: mixed kernel variants", what); return ADDK_ERR_INVALID; }
    if (b.gx > mx.gx) mx.gx = b.gx;
    if (b.gy > mx.gy) mx.gy = b.gy;
    if (b.lds > mx.lds) mx.lds = b.lds;
    if (host_blob) memcpy(static_cast<char*>(host_blob) + (size_t)i * sizeof(Desc), &d, sizeof(Desc));
  }
  meta[0] = mx.key; meta[1] = n; meta[2] = mx.gx; meta[3] = mx.gy;
  if (lds) *lds = mx.lds;
  return total;
}

// Kernels that ask for more than the default 64 KB of dynamic LDS: addk_dyn_lds<kernel>(bytes) raises the kernel's limit before its first launch,
// once per kernel and thread-safely (a function-local static per instantiation).
constexpr int ADDK_MAX_DYN_LDS = 160 * 1024 - 64;
template <auto F> void addk_dyn_lds(int bytes = ADDK_MAX_DYN_LDS) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(F), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)attr;
}
