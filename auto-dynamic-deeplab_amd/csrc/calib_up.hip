// The calibration head on the decoder's low-resolution logits: reliability bins and NLL of one exit at up to 8 temperatures
// (calib_up_kernel).
#include "up.h"

namespace {

// ---- fused logits up-sampling + calibration statistics (temperature scaling, Guo et al. 2017) --------------------------------------
// What the reliability diagram, the ECE and the fit of one temperature per exit need, for CAL_T temperatures in one walk.  The walk is
// scu_walk (same tile, same interpolation z = lh0*t0 + lh1*t1), then the strict `>` arg-max sweep of score_up_kernel; d = z - mx is
// formed once and every temperature j runs its own exp sweep over d * it[j]: CAL_T x CC exponentials per pixel, so the kernel is bound
// by the transcendental rate, not by memory (the target, 8 bytes per pixel, is the only HBM stream).  it[], the NLL partials and
// the pending runs stay in registers (the temperature loop is fully unrolled behind a wave-uniform `j < nt`).
// Bins: on real data most pixels of a tile fall into the top bin, so nothing reaches LDS per pixel.  A thread merges the run of equal
// bins along its column (run_count's idea: count | hits << 16 in one word — a column has 8 pixels — and the confidence sum in units of
// 2^-24 in another); a run that ends mid-column goes to LDS with two atomics; what is pending after the walk is first summed over the
// wave when every lane that holds something holds the same bin (the common case: one LDS atomic pair per wave and temperature instead
// of 64 serialised on one address).  LDS holds [CAL_T][CAL_B] x (count | hits << 16: a workgroup has 2048 pixels; 64-bit confidence
// sum) and is flushed once per workgroup with 64-bit integer atomics, zeros skipped: order-independent, exact.  The flush does not go
// to `bins` itself: a thousand workgroups adding to the same 48 words queue up behind one another at the memory side (measured: 40 us
// of an 82 us launch at one temperature), so workgroup blk adds to replica blk % CAL_REP of the bins in the workspace, and the last
// workgroup sums the replicas, adds the launch's totals to `bins` once per word and leaves the replicas at zero.
// NLL: one fp32 partial per workgroup and temperature, write-through; the workgroup that takes the LAST ticket (csrc/bnfin.h, as
// up_finish) adds the partials of each temperature in a FIXED order in fp64 — thread t the partials t, t + 256, ..., then lanes, then
// the four waves in order — adds the launch's sum to nll[j] once and puts the ticket back to zero.  No floating-point atomics.
constexpr int CAL_T = ADDK_CALIB_MAX_T, CAL_B = ADDK_CALIB_BINS, CAL_REP = 32, CAL_WORDS = CAL_T * CAL_B * 3;
struct CalibUpK : UpSrc {
  const int64_t* target; const float* it; int nt;
  unsigned long long* bins; double* nll;
  unsigned* counter; float* part; unsigned long long* rep; // ws: [ticket, 16 bytes][nblk x CAL_T floats][CAL_REP x CAL_WORDS counters]
};

__device__ __forceinline__ void cal_flush(unsigned* hc, unsigned long long* hq, int slot, unsigned rc, unsigned long long rq) {
  atomicAdd(&hc[slot], rc);
  atomicAdd(&hq[slot], rq);
}

template <int CC, bool VEC>
__global__ void __launch_bounds__(256) calib_up_kernel(const CalibUpK p) {
  __shared__ unsigned hc[CAL_T * CAL_B];
  __shared__ unsigned long long hq[CAL_T * CAL_B];
  __shared__ float shn[4 * CAL_T];
  __shared__ double shd[4];
  __shared__ unsigned flag;
  const int t = threadIdx.x, lane = t & (SCU_W - 1), wv = t / SCU_W;
  if (t < CAL_T * CAL_B) { hc[t] = 0u; hq[t] = 0ull; }
  __syncthreads();
  const int64_t __attribute__((address_space(1)))* tgt = (const int64_t __attribute__((address_space(1)))*)p.target;
  float it[CAL_T], nsum[CAL_T];                                  // wave-uniform inverse temperatures; this thread's NLL sums
  int key[CAL_T]; unsigned rc[CAL_T], rq[CAL_T];                 // pending run of this column: bin, count | hits << 16, Σ conf·2^24
#pragma unroll
  for (int j = 0; j < CAL_T; ++j) {
    it[j] = j < p.nt ? ((const gfloat*)p.it)[j] : 0.f;
    nsum[j] = 0.f; key[j] = -1; rc[j] = 0u; rq[j] = 0u;
  }
  scu_walk<CC, VEC>(p, [&](long pix, const float (&z)[CC]) {
    const long tg = tgt[pix];
    if (tg < 0 || tg >= CC) return;                              // the evaluator's mask: labels in [0, C), whatever ignore_index is
    float mx = -INFINITY, zt = 0.f; int am = 0;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      if (z[c] > mx) { mx = z[c]; am = c; }                      // strict: a tie keeps the lowest channel
      if (c == tg) zt = z[c];
    }
    float d[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) d[c] = z[c] - mx;
    const float dt = zt - mx;
    const unsigned one = am == tg ? 0x10001u : 1u;
#pragma unroll
    for (int j = 0; j < CAL_T; ++j) {
      if (j < p.nt) {                                            // wave-uniform
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < CC; ++c) se += __expf(d[c] * it[j]);
        nsum[j] += logf(se) - dt * it[j];
        const float conf = 1.f / se;
        const int b = min(CAL_B - 1, (int)(conf * (float)CAL_B));
        if (b != key[j]) {
          if (key[j] >= 0) cal_flush(hc, hq, j * CAL_B + key[j], rc[j], rq[j]);
          key[j] = b; rc[j] = 0u; rq[j] = 0u;
        }
        rc[j] += one;
        rq[j] += (unsigned)llrintf(conf * 16777216.f);
      }
    }
  });
  // what is still pending: one bin over the whole wave (lanes without a pixel aside) is summed over the wave first
#pragma unroll
  for (int j = 0; j < CAL_T; ++j) {
    if (j < p.nt) {
      const bool has = key[j] >= 0;
      const unsigned long long m = __ballot(has);
      if (m != 0ull) {                                           // wave-uniform, as is `same`
        const int k0 = __shfl(key[j], __ffsll((long long)m) - 1);
        const bool same = __all(!has || key[j] == k0);
        if (same) {
          unsigned c = has ? rc[j] : 0u;
          unsigned long long q = has ? rq[j] : 0ull;
          for (int s = 32; s > 0; s >>= 1) { c += __shfl_xor(c, s); q += __shfl_xor(q, s); }
          if (lane == 0) cal_flush(hc, hq, j * CAL_B + k0, c, q);
        } else if (has) {
          cal_flush(hc, hq, j * CAL_B + key[j], rc[j], rq[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CAL_T; ++j) {
    float v = nsum[j];
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    if (lane == 0) shn[wv * CAL_T + j] = v;
  }
  __syncthreads();
  const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int nblk = gridDim.x * gridDim.y * gridDim.z;
  if (t < CAL_T * CAL_B) {
    const unsigned c = hc[t];
    if (c) {                                                     // rows j >= nt are never touched
      unsigned long long* o = p.rep + (long)(blk % CAL_REP) * CAL_WORDS + (long)t * 3;
      atomicAdd(o, (unsigned long long)(c & 0xffffu));
      if (c >> 16) atomicAdd(o + 1, (unsigned long long)(c >> 16));
      atomicAdd(o + 2, hq[t]);
    }
  }
  if (t < CAL_T)
    __hip_atomic_store((gu32*)(p.part + (long)blk * CAL_T + t),
                       __float_as_uint(((shn[t] + shn[CAL_T + t]) + shn[2 * CAL_T + t]) + shn[3 * CAL_T + t]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  if (!bnfin_arrive(p.counter, nblk, &flag)) return;
  // ---- the last workgroup: the replicas of every word (integers: any order) into bins, nothing written beyond bins[nt] ----
  for (int e = t; e < p.nt * CAL_B * 3; e += 256) {
    unsigned long long s = 0ull;
    for (int r = 0; r < CAL_REP; ++r) {
      gu64* w = (gu64*)(p.rep + (long)r * CAL_WORDS + e);
      const unsigned long long v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v) { s += v; __hip_atomic_store(w, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
    if (s) p.bins[e] += s;
  }
  // ---- per temperature, thread t adds partials t, t + 256, ..., then lanes and waves in a fixed order ----
  for (int j = 0; j < p.nt; ++j) {
    double s = 0.0;
    for (int i = t; i < nblk; i += 256)
      s += (double)__uint_as_float(__hip_atomic_load((gu32*)(p.part + (long)i * CAL_T + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) shd[wv] = s;
    __syncthreads();
    if (t == 0) p.nll[j] += ((shd[0] + shd[1]) + shd[2]) + shd[3];
    __syncthreads();
  }
  if (t == 0) __hip_atomic_store((gu32*)p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int addk_calib_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C, int32_t nt) {
  return scu_ok(N, H, W, OH, OW, C) && nt >= 1 && nt <= CAL_T ? 1 : 0;
}
extern "C" int64_t addk_calib_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return 0;
  return 16 + 4 * (int64_t)CAL_T * scu_blocks(N, OH, OW) + 8 * (int64_t)CAL_REP * CAL_WORDS;
}
extern "C" int addk_calib_upsample(const addk_calib_upsample_args* a, void* stream) {
  ADDK_REQUIRE(a && a->logits && a->target && a->inv_temp && a->bins && a->nll && a->ws, "calib_upsample: null pointer");
  ADDK_REQUIRE(addk_calib_upsample_supported(a->N, a->H, a->W, a->OH, a->OW, a->C, a->nt) == 1,
               "calib_upsample: unsupported shape (%s, 1..%d temperatures)", gate_classes_text().c_str(), CAL_T);
  ADDK_REQUIRE(a->ld >= a->C, "calib_upsample: short stride");
  CalibUpK k;
  static_cast<UpSrc&>(k) = up_src(a);
  k.target = a->target; k.it = a->inv_temp; k.nt = a->nt;
  k.bins = reinterpret_cast<unsigned long long*>(a->bins); k.nll = a->nll;
  k.counter = (unsigned*)a->ws; k.part = (float*)((char*)a->ws + 16);
  k.rep = (unsigned long long*)(k.part + (long)CAL_T * scu_blocks(a->N, a->OH, a->OW));      // 8-byte aligned: 16 + 32 x nblk
  hipStream_t st = (hipStream_t)stream;
  gate_classes(a->C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    launch_vec(px_vec_ok<CC>(a->logits, a->ld), calib_up_kernel<CC, true>, calib_up_kernel<CC, false>, scu_grid(a->N, a->OH, a->OW), st, k);
  });
  return addk_check_launch("calib_upsample");
}
