/*
 * addk — C ABI of the MI355X (gfx950) kernels behind the Auto-Dynamic-DeepLab hot path.
 *
 * The reference has no native interface: its boundary is a Python object protocol
 * (SURVEY.md §8b).  Each entry point below replaces one family of PyTorch op call
 * sites on that path; the reference file:line it replaces is cited per function.
 * The Python host (auto-dynamic-deeplab_amd/, imported as `addk`) binds these with
 * ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every tensor is fp32, NHWC ("pixel-major"): element (n,h,w,c) of a tensor with pixel
 *     stride `ld` lives at  base[((n*H + h)*W + w)*ld + c].  `ld >= C` lets a tensor be a
 *     channel slice of a wider concat buffer (producers write at a channel offset, so
 *     torch.cat on the path — ADD.py:92,112, aspp_train.py:57, decoder.py:26 — is free).
 *   - a "lazy" activation is (raw, a, b, relu): its value is relu?(a[c]*raw + b[c]).
 *     BatchNorm (+ReLU) is never materialised: the consumer applies it while staging
 *     its input tile (a == NULL means a=1,b=0).
 *   - all pointers are device pointers; nothing is allocated or freed; no host sync;
 *     every launch goes to `stream` (a hipStream_t passed as void*).
 *   - return value: 0 ok, <0 error (see addk_last_error()).
 *   - float4 paths need base pointers 16-byte aligned and ld, C, channel offsets % 4 == 0;
 *     otherwise a scalar path is taken automatically.
 */
#ifndef ADDK_H_
#define ADDK_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADDK_MAX_SRC 12
#define ADDK_MAX_SLAB 32
#define ADDK_MAX_TERMS 4

#define ADDK_OK 0
#define ADDK_ERR_INVALID (-1)
#define ADDK_ERR_UNSUPPORTED (-2)
#define ADDK_ERR_HIP (-3)

const char* addk_last_error(void);
/* 2: the lone entries addk_slab_reduce, addk_bn_eval_affine, addk_bn_bwd_coeffs (version 1: addk_bn_bwd_coeffs_from_dmv) and
 * addk_bn_bwd_apply take one item struct where version 1 took positional arguments; the _batch entries and every struct layout
 * are those of version 1. */
int addk_version(void);
/* Probes MFMA f32 16x16x4 fragment layout on the device: out[256] = A(16x4)·B(4x16) with
 * A[i][k] = i*4+k, B[k][j] = (k+1)*(j+2) (asymmetric).  Used by smoke tests. */
int addk_selftest_mfma(float* out256, void* stream);

/* One source of a virtually concatenated NHWC input. */
typedef struct addk_src {
  const float* x;   /* raw data at channel 0 of this source, pixel 0 */
  const float* a;   /* lazy-BN scale [C] or NULL */
  const float* b;   /* lazy-BN shift [C] or NULL */
  int32_t ld;       /* pixel stride (floats) */
  int32_t C;        /* channels of this source */
  int32_t relu;     /* ReLU after the affine */
  int32_t rs_hw;    /* 0: plain source.  (SH << 16) | SW: `x` is an [N, SH, SW] map that the consumer samples bilinearly
                       (F.interpolate(mode='bilinear'), align_corners=False: ADD.py:76-77,84-90) onto ITS OWN input grid while it
                       stages the tile — the resize in front of a 1x1 convolution never materialises.  The lazy affine / ReLU apply
                       AFTER the interpolation (an affine commutes with it; the ReLU is the consumer's own, operations.py:23).  Only
                       addk_conv_fwd honours it, and only for the shapes addk_conv_fwd_resample_ok() accepts. */
} addk_src;

/* BatchNorm statistics -> lazy affine (F.batch_norm training mode, batchnorm.py:51-53): argument block of addk_bn_finalize, also
 * embedded in the conv launches whose last workgroup does the finalize itself (csrc/bnfin.h). */
typedef struct addk_bn_finalize_args {
  const double* partial; /* fp64 [rows][C][2] (sum, sumsq) — or the all-reduced [1][C][2] */
  int32_t rows, C;
  double count;          /* number of values per channel (global batch under SyncBN) */
  const float* gamma; const float* beta;
  float* running_mean; float* running_var;   /* updated in place (NULL: skip) */
  float momentum, eps;
  float* a; float* b;            /* out: lazy affine  a = gamma*invstd, b = beta - mean*a */
  float* mean; float* invstd;    /* out: saved for backward */
} addk_bn_finalize_args;

/* ---------------------------------------------------------------------------------------
 * Dense convolution, implicit GEMM on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32).
 * Replaces nn.Conv2d(groups=1) call sites: operations.py:24,38,53,57,91-92,109-110;
 * ADD.py:155,161,167,257; aspp_train.py:16-25; decoder.py:14,18,21, with the preceding
 * ReLU / BatchNorm of the producer fused as the input prologue and the per-channel
 * (sum, sum of squares) needed by the following training-mode BatchNorm fused as the
 * epilogue.  Weights are "OHWI": w[co*ldw + (kh*KW+kw)*cin_total + ci] — the memory of a
 * torch [O,I,KH,KW] tensor in channels_last format.  `pad` may be negative
 * (FactorizedReduce's shifted branch, operations.py:94,99).
 * ------------------------------------------------------------------------------------- */
typedef struct addk_conv_args {
  addk_src src[ADDK_MAX_SRC];
  int32_t nsrc;
  int32_t N, H, W;            /* input spatial size */
  int32_t OH, OW;             /* output spatial size */
  int32_t KH, KW, stride, pad, dil;
  int32_t Cout;
  int32_t ldw;                /* weight row stride (floats) */
  int32_t cin_total;          /* channels per tap in the weight layout */
  int32_t w_choff;            /* channel offset of src[0] inside a tap (sources are consecutive) */
  int32_t ldy;
  const float* w;
  float* y;                   /* raw output at channel 0 of the destination slice */
  const float* bias;          /* [Cout] or NULL (decoder.py:21) */
  const float* bias_n;        /* [N][Cout] per-image bias or NULL (ASPP image-pool branch folded
                                 into conv1, aspp_train.py:50-59) */
  double* stats;              /* fp64 [rows][stats_ld][2] partial (sum, sumsq) or NULL; rows = addk_conv_rows().
                                 Points at this conv's first channel inside the row. */
  int32_t stats_ld;           /* channels per slab row (>= Cout; FactorizedReduce's two convs share one BN) */
  int32_t _pad;
  float* wpack;               /* optional workspace of >= addk_conv_fwd_pack_floats() floats, 16-byte aligned: lets the launches
                                 that addk_conv_fwd_pack_floats() sizes run on a halo-patch kernel (weights re-packed into MFMA
                                 fragment order); NULL, short or misaligned = another kernel */
  int64_t wpack_floats;
  int32_t wpack_ready;        /* 1: wpack already holds this launch's packed weights (addk_conv_pack_batch ran since the
                                 last weight update); 0: the launch packs them itself */
  int32_t _pad2;
  float* rs_y;                /* src[0].rs_hw != 0 only: optional materialised copy of the interpolated src[0] (before the affine /
                                 ReLU), pixel stride rs_ldy — training writes it because the backward pass (weight gradient, ReLU
                                 mask, the resize's own gather backward) reads it; NULL at inference */
  int32_t rs_ldy;
  int32_t _pad3;
} addk_conv_args;
int addk_conv_fwd(const addk_conv_args* a, void* stream);
/* 1 when addk_conv_fwd takes this launch with src[i].rs_hw set (a 1x1 stride-1 convolution on the register-stationary or the
 * streaming-K pointwise kernel, pw.hip: ADD.py:84-90 `pre_preprocess` / `preprocess` behind F.interpolate), else 0: the caller
 * then runs addk_resize_fwd first.  Results are bit-identical either way (the same fp32 expressions in the same order). */
int addk_conv_fwd_resample_ok(const addk_conv_args* a);
/* floats of `wpack` the launch needs to run on a halo-patch kernel, whatever `wpack` holds now; 0 = given such a workspace it would
 * still take another kernel (no pack is read) */
int64_t addk_conv_fwd_pack_floats(const addk_conv_args* a);
/* Arithmetic of the wide k x k stride-1 contractions (the halo-patch kernels: forward, data gradient, weight gradient):
 *   0 = exact fp32 products on v_mfma_f32_16x16x4_f32;
 *   1 = "f16x3", split-fp16 (default since round 5): every fp32 operand is x = h + l with h = fp16(x), l = fp16(x - h) (2 x 11 = 22 of
 *       fp32's 24 significand bits) under an exact power-of-two scale (weights: per tensor, from an amax pass in front of the pack;
 *       activations / gradients: a running scale per tile, csrc/conv3b.h), and a product is the sum of its three largest terms on
 *       v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Split error rms 3e-9 of sum|a*b| at K = 2736 — below an fp32 accumulation chain's
 *       rounding noise (1e-8) — at half the matrix instructions of mode 2;
 *   2 = "bf16x6", split-bf16, six terms: x = h + m + l in bf16 (3 x 8 bits = fp32's 24, exact), the six largest bf16 x bf16 terms on
 *       v_mfma_f32_32x32x16_bf16 (rms 5.6e-8 vs the fp32 MFMA chain's 6.8e-8 of sum|a*b| at K = 2048);
 *   3 = "tail_x3": mode 1 in the exit heads only (launches with >= 192 output / gradient channels: ASPP and decoder forward,
 *       data gradient and weight gradient — decoder.py:14-21, aspp_train.py:16-25), mode 2 everywhere else.
 * The reference's own GPU path is 16-bit throughout (apex O1, train.py:145-165).
 * Every other kernel computes in fp32.  Process-wide; set before plans are built (packed-weight buffers are sized per mode).
 * Environment: ADDK_MATH=fp32|f16x3|bf16x6|tail_x3 (bf16x3: the old name of mode 1). */
int addk_set_conv_precision(int mode);
/* Split-bf16 modes: launches with fewer output channels than this stay on the exact fp32 kernel (default 0 = none, see
 * conv3.hip; 65 = round-2's first rule, kept for A/B runs).  c < 0 restores the default. */
int addk_set_split_min_channels(int c);
/* Specialised kernels that may replace the generic ones (all on by default; results agree to fp32 rounding).  The mask is
 * process-wide and is meant for tests and A/B timing; the environment (ADDK_PW=0, ADDK_C3=0, ADDK_WGRAD_H3=0, ADDK_DWTILE=0, ADDK_WGRAD_RS=0) sets the
 * initial value. */
#define ADDK_FAST_PW      1   /* register-stationary 1x1 convolution (pw.hip) */
#define ADDK_FAST_CONV3   2   /* halo-patch 3x3 stride-1 forward / data gradient (conv3.hip; needs wpack) */
#define ADDK_FAST_WGRAD3  4   /* halo-patch 3x3 stride-1 weight gradient (wgrad_h3.hip) */
#define ADDK_FAST_DWTILE  8   /* LDS-tiled depthwise forward / backward, tiled logits-upsample backward */
#define ADDK_FAST_WGRAD_RS 16  /* register-streaming weight gradient of the narrow cell convs (wgrad_rs.hip, wgrad_hk.hip, wgrad_pix.hip: wgrad_st_kernel) */
int addk_set_fast_paths(int mask);
int addk_get_fast_paths(void);
int addk_get_conv_precision(void);
/* number of partial-statistics rows a launch with these shapes writes (<= 1024) */
int addk_conv_rows(int64_t P, int32_t Cout);

/* Data gradient of the same convolution with respect to ONE source (autograd of
 * nn.Conv2d + the ReLU/BN prologue):  g[p,c] (+)= da_mask * sum_{tap,co} dy[..]*w[..], where
 * da_mask = a[c] * (relu ? a[c]*x[p,c]+b[c] > 0 : 1).  Also emits the partial reductions
 * dA[c] = sum_p dz*mask*x, dB[c] = sum_p dz*mask that drive the producer BN's backward. */
typedef struct addk_conv_dgrad_args {
  const float* dy; int32_t lddy; int32_t Cout;     /* gradient of the raw conv output [N,OH,OW,Cout] */
  int32_t N, H, W, OH, OW, KH, KW, stride, pad, dil;
  const float* w; int32_t ldw, cin_total, w_choff; /* w_choff: channel offset of THIS source in a tap */
  addk_src dst;                /* the source whose gradient is produced (x,a,b,relu,ld,C) */
  float* g; int32_t ldg;       /* gradient wrt dst.x (raw), same geometry as dst */
  int32_t accumulate;          /* 0: overwrite g, 1: g += */
  double* dab;                 /* fp64 [rows][C][2] partial (dA,dB) or NULL; rows = addk_conv_rows(N*H*W, C) */
  float* wpack;                /* optional packed-weight workspace (see addk_conv_args.wpack) */
  int64_t wpack_floats;
  int32_t wpack_ready;         /* see addk_conv_args.wpack_ready */
  int32_t _pad2;
} addk_conv_dgrad_args;
int addk_conv_dgrad(const addk_conv_dgrad_args* a, void* stream);
int64_t addk_conv_dgrad_pack_floats(const addk_conv_dgrad_args* a);    /* see addk_conv_fwd_pack_floats */
/* The kernel a forward / data-gradient launch takes (the same choice the launch, the pack size and descriptor, the batch key and
 * addk_conv_fwd_resample_ok read).  cfg[8] = kind, four template parameters, grid x, grid y, launches.  Kinds and parameters:
 *   0 generic implicit GEMM: PT, CT, red32          1 the same over the parity classes of a stride-2 data gradient: PT, CT, red32,
 *                                                     classes (launches > 1: one per class, the first one's parameters and grid)
 *   2 stem0: CT, red32                               3 register-stationary 1x1: CT, KG, RS, red32 (the only kind a batch merges)
 *   4 streaming-K 1x1 forward: CT, RS, red32         5 1x1 data gradient with <= 32 output channels: KMAX
 *   6 fp32 halo patch: BCT, KS                       7 split-precision halo patch: WC, KS, pixels per tile row, rows per tile
 *   8 split-precision stride-2 data gradient: planes 9 split-precision 5x5 on 16-wide tiles: KS, planes
 * Kinds 6-9 read `wpack`. */
int addk_conv_fwd_config(const addk_conv_args* a, int32_t* cfg);
int addk_conv_dgrad_config(const addk_conv_dgrad_args* a, int32_t* cfg);
/* Weight packs hoisted out of the step: fill one opaque descriptor (addk_conv_pack_desc_bytes() bytes, host memory) per
 * launch that takes a halo-patch kernel (pack_desc fails for any other), upload the array and run addk_conv_pack_batch once
 * per step before the first launch; those launches then set wpack_ready = 1. */
/* Batched pointwise convolutions: mutually independent 1x1 launches (one dependency level of the cell DAG) that map to the
 * same kernel variant run as ONE launch.  key >= 0 names the variant of a launch that on its own would take the
 * register-stationary kernel (kind 3 above; -1: any other kernel); prepare() fills a
 * host blob of kernel descriptors (host_blob = NULL: returns its size) and meta[4]; the caller uploads the blob once and
 * replays addk_conv_batch_run.  Same arithmetic as the single launches. */
int addk_conv_fwd_batch_key(const addk_conv_args* a);
int addk_conv_dgrad_batch_key(const addk_conv_dgrad_args* a);
int64_t addk_conv_fwd_batch_prepare(const addk_conv_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int64_t addk_conv_dgrad_batch_prepare(const addk_conv_dgrad_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int addk_conv_batch_run(const void* dev_blob, const int64_t* meta, void* stream);
int64_t addk_conv_pack_desc_bytes(void);
int addk_conv_fwd_pack_desc(const addk_conv_args* a, void* host_desc);
int addk_conv_dgrad_pack_desc(const addk_conv_dgrad_args* a, void* host_desc);
int addk_conv_pack_batch(const void* dev_descs, int32_t n, void* stream);

/* Weight gradient for ONE source: dw[co][tap][w_choff+ci] = sum_p dy[p,co] * z[p@tap,ci],
 * z = relu?(a*x+b).  Deterministic split-P: partial tiles go to `ws`, then are reduced into
 * dw (accumulate: the shared ASPP/decoder head is used once per exit — SURVEY Q4). */
typedef struct addk_conv_wgrad_args {
  const float* dy; int32_t lddy; int32_t Cout;
  int32_t N, H, W, OH, OW, KH, KW, stride, pad, dil;
  addk_src src;
  float* dw; int32_t ldw, cin_total, w_choff;
  int32_t accumulate;
  float* ws; int64_t ws_floats;  /* workspace, >= addk_conv_wgrad_ws() floats */
} addk_conv_wgrad_args;
int addk_conv_wgrad(const addk_conv_wgrad_args* a, void* stream);
int64_t addk_conv_wgrad_ws(int64_t P, int32_t Cout, int32_t C, int32_t taps);

/* Batched weight gradients.  The weight gradients of a backward pass are mutually independent and, for the 40-160
 * channel cell convolutions, individually far too small to fill 256 CUs (HBM-ideal 5 us, launch-latency bound at
 * 30-50 us): `n` of them that share a tile configuration run as ONE launch driven by a device-resident work list, plus
 * one batched reduce.  cfg = {kind, cty, ctz, blocks}; prepare() fills a host blob (descriptors + work lists) to be
 * copied to the device once at plan time (call with host_blob == NULL to get its size); meta[8] is host-side. */
int addk_conv_wgrad_config(const addk_conv_wgrad_args* a, int32_t* cfg);
int64_t addk_conv_wgrad_batch_prepare(const addk_conv_wgrad_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int addk_conv_wgrad_batch_run(const void* dev_blob, const int64_t* meta, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused SepConv half (reference modeling/operations.py:51-53 and :55-57): ReLU / lazy BatchNorm prologue -> depthwise
 * K x K (stride 1, dilation 1, 'same' padding) -> pointwise 1x1 on the matrix cores -> BatchNorm statistics, ONE launch
 * over 2-D LDS tiles (csrc/sepf.hip): the depthwise output never makes a round trip through HBM.  In training `t` receives
 * the depthwise output (the backward pass reads it: pointwise weight gradient, depthwise backward) and, when `fin.a` is set,
 * the LAST workgroup of the launch turns the statistics into the lazy affine (a, b) — no bn_finalize launch (`fin.partial`,
 * `fin.rows`, `fin.C` are ignored: the launch knows its own slab; `fin_counter` is a zero-initialised workspace of
 * addk_bn_fin_ws_bytes(addk_sep_rows(a), stats_ld) bytes owned by this BatchNorm call — ticket counters and group rows of the
 * two-level reduction — whose counters the launch leaves at zero again).  In inference t = NULL and the epilogue can apply the op's own
 * (frozen) BatchNorm and add the other branches of the cell block (ADD.py:108):
 *     y = ea[c]*acc + eb[c] + sum_i relu_i?(a_i*term_i + b_i)        (ea == NULL: plain y = acc)
 * Covered shapes: K in {3,5}, C == Cout in (32, 48] or (64, 80], 16-byte aligned tensors; 80 channels up to 512 workgroups.
 * `src` and every term, forward and backward: a and b both set or both NULL, ld >= C, rs_hw == 0 (a resampled source is addk_conv_fwd's
 * alone).  Any other source is refused: not supported, batch key -1, an error from the launch and from *_batch_prepare.
 *
 * Forward and backward share ONE tile choice, made from (N, H, W, C, Cout, K) alone (csrc/sep.h): the same shape gets the same
 * variant (ks, kg, kp, r) and the same tiles in both directions.  The fast-path mask (ADDK_FAST_PW) gates what the library
 * RECOMMENDS: addk_sep_fwd_supported, addk_sep_bwd_rows, the batch keys, cfg[0] and cfg[7] below.  addk_sep_rows is plain
 * geometry, and a direct addk_sep_fwd / addk_sep_bwd call (or a batch prepared from such arguments) runs the fused kernel
 * whatever the mask says.
 * addk_sep_fwd_config / addk_sep_bwd_config: cfg[8] = fused (1: recommended; forward = addk_sep_fwd_supported, arguments checked;
 * backward = addk_sep_bwd_rows > 0, shape and mask only, so that it can be asked before dy and ws exist), ks, kg, kp, r, grid x,
 * rows (= grid x; cfg[1..6] are 0 for a shape the kernels do not take), batch key or -1.
 * ------------------------------------------------------------------------------------- */
typedef struct addk_sep_args {
  addk_src src;                     /* lazy input of the depthwise conv (x, a, b, relu) */
  int32_t N, H, W;                  /* output size == input size */
  int32_t K;                        /* depthwise kernel size (3 or 5) */
  int32_t Cout; int32_t ldw;        /* pointwise: Cout x src.C weights, row stride ldw */
  const float* dw_w;                /* depthwise weights [src.C][K*K] */
  const float* pw_w;
  float* y; int32_t ldy;
  int32_t ldt; float* t;            /* depthwise output [P][ldt] or NULL */
  void* stats; int32_t stats_ld;    /* fp64 (sum, sumsq) partial slab [stats_rows][stats_ld][2] or NULL */
  int32_t stats_rows;               /* rows the caller allocated: >= addk_sep_rows(a).  Without a fused finalize the rows no workgroup owns
                                       (addk_sep_rows(a) .. stats_rows) are zero-filled, for a reduction over all stats_rows rows (addk_bn_finalize,
                                       addk_slab_reduce).  With fin.a set they are left untouched: the launch's own finalize reads exactly its
                                       addk_sep_rows(a) rows, and nothing may read the others afterwards */
  int32_t nterm;                    /* inference epilogue: number of extra terms (0..ADDK_MAX_TERMS) */
  const float* ea; const float* eb; /* inference epilogue: own affine (both NULL = none) */
  addk_src term[ADDK_MAX_TERMS];
  addk_bn_finalize_args fin;        /* fused finalize of the statistics (fin.a == NULL: none) */
  void* fin_counter;
} addk_sep_args;
int64_t addk_bn_fin_ws_bytes(int32_t nblocks, int32_t ld);
int addk_sep_rows(const addk_sep_args* a);               /* slab rows (= workgroups) of the fused launch; 0: shape not covered */
int addk_sep_fwd_supported(const addk_sep_args* a);      /* 1: the fused kernel covers this launch and the mask allows it */
int addk_sep_fwd_config(const addk_sep_args* a, int32_t* cfg);
int addk_sep_fwd(const addk_sep_args* a, void* stream);
/* table-driven batch of the fused halves of one dependency level (same protocol as addk_conv_fwd_batch_prepare / addk_conv_batch_run) */
int addk_sep_fwd_batch_key(const addk_sep_args* a);
int64_t addk_sep_fwd_batch_prepare(const addk_sep_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int addk_sep_batch_run(const void* dev_blob, const int64_t* meta, void* stream);

/* Fused BACKWARD of a SepConv half (csrc/sepb.hip): pointwise data gradient (dt = W^T dy, matrix cores) and depthwise backward
 * (dx, depthwise weight-gradient partials, (dA, dB) of the input's lazy BatchNorm) in one launch; dt stays on chip.  dy is the
 * gradient wrt the pointwise output with the BatchNorm backward already applied (addk_bn_bwd_apply).  The pointwise WEIGHT
 * gradient is not part of it (addk_conv_wgrad on dy and the stored depthwise output).  `ws` ([rows][C][K*K] floats) and `dab`
 * ([rows][C][2] fp64) get one row per workgroup, rows = addk_sep_bwd_rows(a); ws is reduced by addk_dw_wreduce_batch. */
typedef struct addk_sep_bwd_args {
  const float* dy; int32_t lddy;
  int32_t N, H, W, K;               /* stride 1, dilation 1, pad K/2: output size == input size */
  addk_src src;                     /* forward input of the depthwise conv (x, a, b, relu) */
  int32_t Cout; int32_t ldw;        /* pointwise weights [Cout][src.C], row stride ldw; Cout == src.C */
  const float* dw_w; const float* pw_w;
  float* g; int32_t ldg; int32_t accumulate;   /* gradient wrt src.x (NULL: skip) */
  double* dab;                      /* or NULL */
  float* ws;
} addk_sep_bwd_args;
int addk_sep_bwd_rows(const addk_sep_bwd_args* a);       /* reads the shape only; 0: not recommended */
int addk_sep_bwd_config(const addk_sep_bwd_args* a, int32_t* cfg);
int addk_sep_bwd(const addk_sep_bwd_args* a, void* stream);
int addk_sep_bwd_batch_key(const addk_sep_bwd_args* a);
int64_t addk_sep_bwd_batch_prepare(const addk_sep_bwd_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int addk_sep_bwd_batch_run(const void* dev_blob, const int64_t* meta, void* stream);

/* ---------------------------------------------------------------------------------------
 * Depthwise k x k convolution (groups == C), stride 1 or 2, pad k/2*dil: the depthwise
 * halves of SepConv (operations.py:52,56).  w is [C][KH*KW] (torch [C,1,KH,KW]).
 * ------------------------------------------------------------------------------------- */
typedef struct addk_dw_args {
  addk_src src;
  int32_t N, H, W, OH, OW, KH, KW, stride, pad, dil;
  const float* w;
  float* y; int32_t ldy;
} addk_dw_args;
int addk_dw_fwd(const addk_dw_args* a, void* stream);

typedef struct addk_dw_bwd_args {
  const float* dy; int32_t lddy;
  int32_t N, H, W, OH, OW, KH, KW, stride, pad, dil;
  addk_src src;                 /* forward input (x,a,b,relu) */
  const float* w;
  float* g; int32_t ldg; int32_t accumulate;   /* gradient wrt src.x (may be NULL: skip dgrad) */
  double* dab;                  /* fp64 [rows][C][2] or NULL; rows = addk_dw_rows() */
  float* dw; int32_t dw_accumulate;            /* [C][KH*KW] */
  float* ws;                    /* [rows][C][KH*KW] partial weight gradients */
  int32_t defer_wreduce;        /* 1: leave the partials in ws; the caller reduces them later with addk_dw_wreduce_batch */
  int32_t _pad;
} addk_dw_bwd_args;
int addk_dw_bwd(const addk_dw_bwd_args* a, void* stream);
/* Deferred reduction of the depthwise weight-gradient partials of MANY convolutions in one launch (they are mutually
 * independent and only needed by the optimizer): table entry i reduces ws_i [rows_i][n_i] into dw_i [n_i]. */
typedef struct addk_dw_wreduce_item { const float* ws; float* dw; int32_t rows, n, accumulate, _pad; } addk_dw_wreduce_item;
int addk_dw_wreduce_batch(const addk_dw_wreduce_item* dev_items, int32_t n_items, void* stream);
/* Batched depthwise launches (same scheme as addk_conv_*_batch_*): mutually independent depthwise convs of one dependency
 * level that run on the LDS-tiled kernel of one size share ONE launch.  key >= 0 names the variant (-1: not covered; the
 * backward form needs defer_wreduce = 1); prepare() fills the host blob of kernel descriptors and meta[5]. */
int addk_dw_fwd_batch_key(const addk_dw_args* a);
int addk_dw_bwd_batch_key(const addk_dw_bwd_args* a);
int64_t addk_dw_fwd_batch_prepare(const addk_dw_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int64_t addk_dw_bwd_batch_prepare(const addk_dw_bwd_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int addk_dw_batch_run(const void* dev_blob, const int64_t* meta, void* stream);
int addk_dw_rows(int64_t P, int32_t C);
/* The kernel a depthwise launch takes (what the launch, the batch key and prepare read): cfg[8] = kind (0 generic, 1 LDS-tiled:
 * 3x3 / 5x5, 16-byte aligned, >= 2048 pixels, backward stride 1, ADDK_FAST_DWTILE set), kernel size, rows per tile (generic: 0),
 * grid x, grid y, dynamic LDS bytes, workspace rows (forward: 0), batch key or -1. */
int addk_dw_fwd_config(const addk_dw_args* a, int32_t* cfg);
int addk_dw_bwd_config(const addk_dw_bwd_args* a, int32_t* cfg);

/* ---------------------------------------------------------------------------------------
 * BatchNorm statistics (F.batch_norm training mode, batchnorm.py:51-53; eps=1e-5, mom=0.1).
 * ------------------------------------------------------------------------------------- */
int addk_bn_finalize(const addk_bn_finalize_args* a, void* stream);
/* n independent BatchNorms in one launch; dev_table = device array of n argument structs, max_C = largest C among them */
int addk_bn_finalize_batch(const addk_bn_finalize_args* dev_table, int32_t n, int32_t max_C, void* stream);

/* Every BatchNorm op below comes as X(const item*, stream), one launch for one item, and X_batch(dev_table, n, ..., stream), one
 * launch for a device array of n items of the same type. */

/* sum the rows of a partial slab into out[C][2] (the vector that is all-reduced over RCCL) */
typedef struct addk_slab_reduce_item { const double* partial; double* out; int32_t rows, C; } addk_slab_reduce_item;
int addk_slab_reduce(const addk_slab_reduce_item* it, void* stream);
int addk_slab_reduce_batch(const addk_slab_reduce_item* dev_table, int32_t n, int32_t max_C, void* stream);

/* eval mode: a = gamma/sqrt(running_var+eps), b = beta - running_mean*a (gamma / beta NULL: 1 / 0); 56 bytes */
typedef struct addk_bn_eval_item {
  const float* gamma; const float* beta; const float* running_mean; const float* running_var; float* a; float* b; int32_t C; float eps;
} addk_bn_eval_item;
int addk_bn_eval_affine(const addk_bn_eval_item* it, void* stream);
/* the same for every BatchNorm of an inference plan in ONE launch */
int addk_bn_eval_affine_batch(const addk_bn_eval_item* dev_table, int32_t n, void* stream);

/* Backward of the statistics + affine:  given the partial (dA,dB) slabs of every consumer,
 *   dgamma (+)= invstd*(dA - mean*dB), dbeta (+)= dB,
 *   dmean_tot = -a*dB - 2*mean*dvar,  dvar = -0.5*gamma*(dA-mean*dB)*invstd^3,
 *   c1 = dmean_tot/count, c2 = 2*dvar/count  so that  dx_raw = G + c1 + c2*x.
 * With SyncBN, `dmv` receives (dmean_tot, dvar) per channel for the cross-rank all-reduce
 * and addk_bn_bwd_coeffs() finishes the job. */
typedef struct addk_bn_bwd_args {
  const double* slab[ADDK_MAX_SLAB]; int32_t rows[ADDK_MAX_SLAB]; int32_t nslab;
  int32_t C; double count;
  const float* gamma; const float* mean; const float* invstd; const float* a;
  float* dgamma; float* dbeta; int32_t accumulate;
  float* c1; float* c2;          /* out (NULL when dmv is used) */
  float* dmv;                    /* out [C][2] (dmean_tot, dvar) or NULL */
  int32_t centered; int32_t _pad; /* 1: c1 (dmv[0]) leaves out the -2*mean*dvar part: the consumer applies c2*(x - mean) */
} addk_bn_bwd_args;
int addk_bn_bwd(const addk_bn_bwd_args* a, void* stream);
int addk_bn_bwd_batch(const addk_bn_bwd_args* dev_table, int32_t n, int32_t max_C, void* stream);
/* c1 = dmv[c][0] / count, c2 = 2 * dmv[c][1] / count from the all-reduced dmv */
typedef struct addk_bn_coeffs_item { const float* dmv; float* c1; float* c2; double count; int32_t C, _pad; } addk_bn_coeffs_item;
int addk_bn_bwd_coeffs(const addk_bn_coeffs_item* it, void* stream);
int addk_bn_bwd_coeffs_batch(const addk_bn_coeffs_item* dev_table, int32_t n, int32_t max_C, void* stream);

/* ---------------------------------------------------------------------------------------
 * Elementwise "materialise" kernels.
 * affine_sum: out[p,c] = relu?( sum_i (a_i[c]*x_i[p,c] + b_i[c]) )  — the 2-way branch sum of a
 *   cell block (ADD.py:108) written straight into its slot of the concat buffer (ADD.py:112).
 * ------------------------------------------------------------------------------------- */
typedef struct addk_affine_sum_args {
  addk_src term[ADDK_MAX_TERMS]; int32_t nterm;   /* term.relu applies per term */
  int64_t P; int32_t C;
  float* out; int32_t ldo; int32_t relu_out; int32_t accumulate;
} addk_affine_sum_args;
int addk_affine_sum_fwd(const addk_affine_sum_args* a, void* stream);

/* backward: for every term i with g_i != NULL:  g_i (+)= a_i*mask_i*dout,  dab_i = partial (sum dout*mask*x_i, sum dout*mask) */
typedef struct addk_affine_sum_bwd_args {
  addk_src term[ADDK_MAX_TERMS]; int32_t nterm;
  int64_t P; int32_t C;
  const float* dout; int32_t lddo;
  const float* out; int32_t ldo; int32_t relu_out;   /* forward output, needed only when relu_out */
  float* g[ADDK_MAX_TERMS]; int32_t ldg[ADDK_MAX_TERMS]; int32_t accumulate[ADDK_MAX_TERMS];
  double* dab[ADDK_MAX_TERMS];    /* fp64 [rows][C][2] partials, rows = addk_ew_rows(P, C) */
} addk_affine_sum_bwd_args;
int addk_affine_sum_bwd(const addk_affine_sum_bwd_args* a, void* stream);
int addk_ew_rows(int64_t P, int32_t C);

/* dy[p,c] = g[p,c] + c1[c] + c2[c]*(x[p,c] - mean[c])   (BN backward applied to the accumulated gradient;
 * mean/c1/c2 may be NULL = 0).  The centred form (addk_bn_bwd_args.centered) keeps c2*x from cancelling against a c1 that
 * carries -c2*mean: the reference subtracts the mean first (batchnorm.py:51-53 / ATen batch_norm_backward).  out may alias g.
 * c1 and c2 come together; x is needed only with c2; C <= 1024.  The lone entry accepts any alignment (an item that is not
 * vector-aligned runs a generic kernel); the table form demands vector-aligned items: 16-byte pointers, ld % 4 == 0, C % 4 == 0. */
typedef struct addk_bn_apply_item {
  const float* g; const float* x; const float* c1; const float* c2; const float* mean; float* out; int64_t P; int32_t ldg, ldx, ldo, C;
} addk_bn_apply_item;
int addk_bn_bwd_apply(const addk_bn_apply_item* it, void* stream);
/* the same for n independent tensors in one launch, max_P = largest P among them */
int addk_bn_bwd_apply_batch(const addk_bn_apply_item* dev_table, int32_t n, int64_t max_P, void* stream);

/* ---------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=False, no antialias (F.interpolate call sites ADD.py:76-77,
 * 84,89,317; decoder.py:24,28).  Optional lazy prologue on the input; NCHW output / NCHW
 * gradient input for the final logits (decoder.py:28) so the caller sees [N,C,H,W].
 * ------------------------------------------------------------------------------------- */
typedef struct addk_resize_args {
  addk_src src; int32_t N, H, W, OH, OW;
  float* y; int32_t ldy;        /* NHWC destination (ignored when nchw_out) */
  int32_t nchw_out;             /* 1: y is [N,C,OH,OW] contiguous */
} addk_resize_args;
int addk_resize_fwd(const addk_resize_args* a, void* stream);

typedef struct addk_resize_bwd_args {
  const float* dy; int32_t lddy; int32_t nchw_in;   /* gradient of the resized tensor */
  const float* dy_scale;        /* optional device scalar multiplying dy (loss scale) */
  addk_src src; int32_t N, H, W, OH, OW;
  float* g; int32_t ldg; int32_t accumulate;
  double* dab;                  /* fp64 [rows][C][2] or NULL (only with a lazy+relu prologue) */
} addk_resize_bwd_args;
int addk_resize_bwd(const addk_resize_bwd_args* a, void* stream);
/* Batched form: the mutually independent resize backwards of one dependency level (the up to ten resized dense inputs of a cell,
 * ADD.py:84-90) as ONE launch.  key >= 0: the launch runs on the table-driven kernel with that variant (equal keys may share a batch);
 * prepare(host_blob = NULL) returns the blob size; meta[8] carries the launch geometry from prepare to run. */
int addk_resize_bwd_batch_key(const addk_resize_bwd_args* a);
int64_t addk_resize_bwd_batch_prepare(const addk_resize_bwd_args* a, int32_t n, void* host_blob, int64_t blob_bytes, int64_t* meta);
int addk_resize_bwd_batch_run(const void* dev_blob, const int64_t* meta, void* stream);
/* The kernel a resize backward launch takes (what the launch, the batch key and prepare read): cfg[8] = kind (0 NHWC per-thread gather,
 * 1 NHWC table-driven: 16-byte aligned, C % 4 == 0, at least 2 pixel lanes (C <= 512), OH <= 8 H + 1 and OW <= 8 W + 1, < 2^30 pixels,
 * ADDK_FAST_DWTILE set; 2 NCHW per-thread; 3 NCHW LDS-tiled: up-sampling by x1 to x8.3 per axis, ADDK_FAST_DWTILE set), taps per axis of the
 * table-driven kernel (5 / 9 / 17; else 0), grid x, grid y, dynamic LDS bytes, input pixels per row segment of the table-driven kernel
 * (else 0), number of 1024-channel slices the launch runs as (more than 1: the other entries describe the first slice and the key is -1),
 * batch key or -1.  Arguments addk_resize_bwd rejects are rejected here with the same error; addk_resize_bwd_batch_key gives -1 for them. */
int addk_resize_bwd_config(const addk_resize_bwd_args* a, int32_t* cfg);

/* ---------------------------------------------------------------------------------------
 * Global average pool with lazy prologue (AdaptiveAvgPool2d(1), aspp_train.py:13,50; ADD.py:506).
 * y[n,c] = mean_hw relu?(a*x+b).  Backward: g (+)= mask*a*dy[n,c]/(H*W).
 * ------------------------------------------------------------------------------------- */
/* ws: >= N * addk_ew_rows(HW, C) * C floats of scratch; mean=0 returns the plain per-image sum
 * (used for bias gradients). */
int addk_gap_fwd(const addk_src* src, int32_t N, int32_t HW, float* y, int32_t ldy, float* ws, int32_t mean, void* stream);
int addk_gap_bwd(const addk_src* src, int32_t N, int32_t HW, const float* dy, int32_t lddy,
                 float* g, int32_t ldg, int32_t accumulate, double* dab, void* stream);

/* 3x3 pooling primitives of the registry (operations.py:9-10; cold on every shipped genotype).
 * mode 0: max, 1: avg with count_include_pad=False.  pad=1. */
int addk_pool3_fwd(const addk_src* src, int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW,
                   int32_t stride, int32_t mode, float* y, int32_t ldy, void* stream);
int addk_pool3_bwd(const addk_src* src, int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW,
                   int32_t stride, int32_t mode, const float* dy, int32_t lddy,
                   float* g, int32_t ldg, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * Layout transforms at the model boundary.
 * ------------------------------------------------------------------------------------- */
int addk_nchw_to_nhwc(const float* x, int32_t N, int32_t C, int64_t HW, float* y, int32_t ldy, void* stream);
int addk_nhwc_to_nchw(const addk_src* src, int32_t N, int64_t HW, float* y, void* stream);
/* gradient of nhwc_to_nchw incl. the lazy prologue: g (+)= mask*a*dy_nchw, dab partials */
int addk_nchw_grad_to_nhwc(const float* dy, const addk_src* src, int32_t N, int64_t HW,
                           float* g, int32_t ldg, int32_t accumulate, double* dab, void* stream);

/* ---------------------------------------------------------------------------------------
 * Softmax cross-entropy over NCHW logits (nn.CrossEntropyLoss(weight, ignore_index), train.py:70,231).
 * loss_out[0] += scale * sum_valid w[t]*nll / sum_valid w[t];  dlogits = scale*w[t]*(softmax-onehot)/wsum.
 * `wsum` (device, 1 float) is produced by addk_ce_count.  target is int64 [N,H,W].
 * `ws` is addk_ce_ws_floats() floats of scratch (per-block partial sums, reduced in a fixed order).
 * ------------------------------------------------------------------------------------- */
int addk_ce_count(const int64_t* target, int64_t n, const float* class_w, int32_t ignore_index,
                  int32_t num_classes, float* wsum, float* ws, void* stream);
int addk_ce_fwd_bwd(const float* logits, const int64_t* target, int32_t N, int32_t C, int64_t HW,
                    const float* class_w, int32_t ignore_index, const float* wsum, float scale,
                    float* loss_out, float* dlogits, float* ws, void* stream);
int64_t addk_ce_ws_floats(int32_t N, int64_t HW);

/* The class counts C the fused heads on the low-resolution logits are compiled for, two lists in csrc/up.h.
 *   addk_head_classes       the training heads (addk_ce_upsample_fwd_bwd and its _ohem, _kd, _dice and _shaped forms, addk_ohem_select,
 *                           addk_dice_stats), the label heads (addk_label_upsample, addk_label_tiles_upsample,
 *                           addk_label_tile_views_upsample), the window gate (addk_gate_tiles_upsample) and the compile-time form of addk_ce_fwd_bwd:
 *                           19 (Cityscapes) and 21 (Pascal VOC).
 *   addk_gate_head_classes  the scoring, profile, calibration, gate and multi-view heads (addk_score_upsample, addk_profile_upsample[_t],
 *                           addk_calib_upsample, addk_gate_upsample[_t], addk_gate_label_upsample, addk_label_views_upsample): 19.
 * Each writes the first min(count, cap) counts to out (out may be NULL with cap <= 0) and returns the count.  A head's *_supported(..., C)
 * is 0 for a C outside its list.  The normalised entropy of the gate and profile heads divides by log 19, as the reference's gate
 * does whatever the dataset (modeling/ADD.py:474 calls normalized_shannon_entropy without num_class). */
int addk_head_classes(int32_t* out, int32_t cap);
int addk_gate_head_classes(int32_t* out, int32_t cap);

/* Fused form for the training step: the bilinear up-sampling of the decoder's logits (decoder.py:28,
 * F.interpolate(mode='bilinear', align_corners=False)) and the cross-entropy on it (train.py:70,231) in one pass over the
 * LOW-resolution NHWC logits [N,H,W,C] — loss_out[0] += scale * CE(upsample(logits) -> [N,C,OH,OW], target), and
 * g (+)= d loss / d logits.  The [N,C,OH,OW] tensor and its gradient are never materialised.  Deterministic (gather, fixed
 * summation order).  addk_ce_upsample_supported() is 0 for shapes the kernel does not take (C not in addk_head_classes(), more than 16 output
 * rows per input row): the caller then runs addk_resize_fwd + addk_ce_fwd_bwd + addk_resize_bwd. */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const int64_t* target;             /* [N,OH,OW] */
  const float* class_w;              /* [C] or NULL */
  int32_t ignore_index;
  const float* wsum;                 /* device scalar from addk_ce_count */
  float scale;
  float* loss_out;                   /* device scalar, accumulated */
  float* g; int32_t ldg; int32_t accumulate;
  float* ws;                         /* addk_ce_upsample_ws_floats() floats */
} addk_ce_upsample_args;
int addk_ce_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
int64_t addk_ce_upsample_ws_floats(int32_t N, int32_t H, int32_t W);
int addk_ce_upsample_fwd_bwd(const addk_ce_upsample_args* a, void* stream);

/* Online hard example mining (OHEM, "bootstrapped" cross-entropy) for the fused loss head, per exit and per process (under DDP
 * every rank mines its own batch; gradient averaging is unchanged).  Parameters: thresh = theta in (0, 1], a target-class
 * probability, and min_kept_total = K = min_kept * N.  For every full-resolution pixel
 *   z     = bilinear sample (align_corners=False) of the low-resolution NHWC logits, lh0*(lw0*a + lw1*b) + lh1*(lw0*c + lw1*d)
 *   valid = target != ignore_index and 0 <= target < C
 *   l     = max(0, logsumexp(z) - z[target])   fp32, unweighted; the clamp removes the -1e-7 rounding can leave, makes
 *           thresh = 1 mean "keep everything" and keeps the bit pattern of l monotone in l.
 * With n = number of valid pixels of the batch and l_(j) the j-th largest l among them,
 *   tau   = min(-log theta, l_(min(K, n)))          (-log theta = (float)(-log((double)thresh)), taken on the host)
 *   kept  = valid and l >= tau                      ties at tau are all kept: kept >= min(K, n); no traversal order enters.
 * In exact arithmetic this is mmseg's OHEMPixelSampler / HRNet's OhemCrossEntropy written in the loss domain, with `>=` in
 * place of their strict comparison one index further on.  n == 0: tau = -log theta, nothing is kept, wsum_kept = 0.
 *
 * addk_ohem_select writes, all on the stream (no host read; a captured hipGraph replays it; it clears its own histograms):
 *   pix_loss[N,OH,OW] = l, or -1 where the pixel is not valid
 *   tau[0], wsum_kept[0] = sum over kept pixels of class_w[target] (or 1), counts[0] = n, counts[1] = #kept
 * Selection is EXACT: tau carries the bits a full sort of pix_loss gives — a three-pass radix select on the bit pattern of l
 * (bits 31..21 binned while the map is written, then 20..10 and 9..0 over the stored map), integer histograms only.
 * wsum_kept is a fixed-order two-stage sum: bit-reproducible.  addk_ohem_select_supported() is 0 for C not in addk_head_classes(), non-positive
 * sizes, a grid beyond the limits of addk_score_upsample_supported or N*OH*OW >= 2^31 (32-bit histogram counters).
 *
 * addk_ce_upsample_ohem_fwd_bwd is addk_ce_upsample_fwd_bwd with the per-pixel weight w = kept ? class_w[t] (or 1) : 0, where
 * kept is READ from the stored map: pix_loss[n,Y,X] >= *tau — the kept set comes from one computation of l.  ce.wsum must
 * point at wsum_kept (the normaliser sum_kept w).  Supported exactly where addk_ce_upsample_supported() is 1.
 * Both entry points return ADDK_ERR_INVALID and launch nothing for a null pointer, thresh outside (0, 1],
 * min_kept_total < 1 or ld < C (the head takes no thresh: its pix_loss and tau must be non-null). */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const int64_t* target;             /* [N,OH,OW] */
  const float* class_w;              /* [C] or NULL */
  int32_t ignore_index;
  float thresh;                      /* theta in (0, 1] */
  int64_t min_kept_total;            /* K >= 1 */
  float* pix_loss;                   /* [N,OH,OW] */
  float* tau;                        /* 1 float */
  float* wsum_kept;                  /* 1 float */
  int64_t* counts;                   /* [2]: valid, kept */
  void* ws;                          /* addk_ohem_select_ws_bytes() bytes */
} addk_ohem_select_args;
int addk_ohem_select_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
int64_t addk_ohem_select_ws_bytes(int32_t N, int32_t OH, int32_t OW);
int addk_ohem_select(const addk_ohem_select_args* a, void* stream);
typedef struct {
  addk_ce_upsample_args ce;          /* ce.wsum: the wsum_kept of addk_ohem_select */
  const float* pix_loss;             /* [N,OH,OW] from addk_ohem_select */
  const float* tau;                  /* 1 float from addk_ohem_select */
} addk_ce_upsample_ohem_args;
int addk_ce_upsample_ohem_fwd_bwd(const addk_ce_upsample_ohem_args* a, void* stream);

/* Self-distillation from the final exit for the fused loss head ("Be Your Own Teacher"): a student exit's loss head gets a second term,
 * the KL divergence of its softened prediction from the last exit's.  Parameters: alpha > 0 and temperature T > 0, both finite.
 *   teacher   the low-resolution NHWC logits of the LAST exit, on the grid of ce.logits ([N,H,W,C], its own pixel stride ld_teacher);
 *             read-only and detached: the term sends no gradient into the teacher.  The last exit itself keeps the plain head.
 * For every full-resolution pixel z_s and z_t are the bilinear samples of the student's and the teacher's low-resolution logits with the
 * same src_index values and the same expression lh0*(lw0*a + lw1*b) + lh1*(lw0*c + lw1*d);
 *   valid = target != ignore_index and 0 <= target < C                       (the predicate of the plain head)
 *   q_s = softmax(z_s / T), q_t = softmax(z_t / T), each with its own maximum subtracted (1/T is rounded to fp32 once, on the host)
 *   KL  = sum_c q_t[c] * (log q_t[c] - log q_s[c])
 * With n the number of valid pixels of the batch (the device word nvalid: addk_ce_count with class_w == NULL) and s = ce.scale:
 *   kd           = s * alpha * T^2 * (1/n) * sum_valid KL
 *   loss_out[0] += s * CE (definition of addk_ce_upsample_fwd_bwd, or of the OHEM head when pix_loss / tau are set)  +  kd
 *   kd_out[0]    = kd                written, not accumulated: a replayed graph leaves the last step's value
 *   g          (+)= the CE gradient of that head + the bilinear transpose of s * alpha * T * (q_s - q_t) / n over valid pixels
 * The term is not weighted by class_w and mining never filters it (under DDP every rank uses its own n, as the CE term does).  A pixel that
 * is not valid, and n == 0, contribute exactly 0 to kd and to the gradient (a select, not a factor 0); kd_out is finite whenever the
 * logits are.  Deterministic: the KL partials of the workgroups are added in a fixed order, no float atomics.
 * ws holds addk_ce_upsample_kd_ws_floats() floats.  Supported exactly where addk_ce_upsample_supported() is 1.  Returns ADDK_ERR_INVALID
 * and launches nothing for a null teacher, nvalid, kd_out or any pointer the plain head refuses, teacher == ce.logits, ld_teacher < C,
 * a non-finite or non-positive alpha or temperature, and exactly one of pix_loss / tau set. */
typedef struct {
  addk_ce_upsample_args ce;
  const float* pix_loss; const float* tau;      /* both NULL: no mining; both set: the OHEM head's kept set */
  const float* teacher; int32_t ld_teacher;     /* NHWC [N,H,W,C] on the grid of ce.logits */
  float alpha, temperature;
  const float* nvalid;                          /* device scalar: addk_ce_count with class_w == NULL */
  float* kd_out;                                /* device scalar, written */
} addk_ce_upsample_kd_args;
int addk_ce_upsample_kd_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
int64_t addk_ce_upsample_kd_ws_floats(int32_t N, int32_t H, int32_t W);
int addk_ce_upsample_kd_fwd_bwd(const addk_ce_upsample_kd_args* a, void* stream);

/* Soft-Dice region term for the fused loss head: a per-class overlap measure beside the per-pixel cross-entropy, per exit and per process
 * (under DDP every rank uses its own sums, as mining and distillation do; gradient averaging is unchanged).  Parameters: weight > 0 and
 * smooth >= 0, both finite.  For every full-resolution pixel x
 *   z     = bilinear sample (align_corners=False) of the low-resolution NHWC logits, lh0*(lw0*a + lw1*b) + lh1*(lw0*c + lw1*d)
 *   p     = softmax(z)  (e = exp(z - max z), p = e * (1 / sum e))
 *   valid = target != ignore_index and 0 <= target < C                       (the predicate of the plain head)
 * Over the valid pixels of the batch, per class c:
 *   I_c = sum p_c(x) [t(x) = c]      P_c = sum p_c(x)      Y_c = #{x : t(x) = c}
 *   D_c = (2 I_c + smooth) / (P_c + Y_c + smooth)          present = {c : Y_c > 0}, m = |present|, s = scale
 *   dice = s * weight * (1 - (1/m) sum_{c in present} D_c),   exactly 0 when m == 0
 * and with k = s * weight / m the gradient with respect to z is
 *   A_c = k * 2 / (P_c + Y_c + smooth),  B_c = k * (2 I_c + smooth) / (P_c + Y_c + smooth)^2     (both 0 for an absent class)
 *   G_j(x) = B_j - A_j [t(x) = j],       dz_j(x) = valid ? p_j * (G_j - sum_c p_c G_c) : 0       (a select, not a factor)
 * The select is taken once per pixel, on 1 / sum e and on p_t * A_t: a pixel that is not valid adds exactly 0 whenever its logits are finite.
 * The term is not weighted by class_w and mining never filters it: a kept set filters the cross-entropy term only.
 *
 * addk_dice_stats is the reduction, all on the stream (no host read, no host memset: a captured hipGraph replays it; it clears its own
 * count table).  It writes
 *   coef[0..C)   = A_c,  coef[C..2C) = B_c         what the head reads; all zero when m == 0
 *   dice_out[0]  = dice,  dice_out[1 + c] = D_c, or -1 for an absent class        written, not accumulated
 *   loss_out[0] += dice
 * and leaves in ws, as 32-bit words, [0..C) the counts Y_c (uint32), [32..32+C) I_c and [64..64+C) P_c (float) of this call; the rest is
 * scratch.  Y_c is exact (integer atomics); I_c and P_c are per-workgroup fp32 partials added in a fixed order in fp64; D_c, A_c, B_c and
 * the term are formed in fp64 and rounded once.  No float atomics: two calls give equal bits.  addk_dice_stats_supported() is 0 for
 * C not in addk_head_classes(), non-positive sizes, a grid beyond the limits of addk_score_upsample_supported or N*OH*OW >= 2^31 (32-bit counters).
 * Returns ADDK_ERR_INVALID and launches nothing for a null pointer, ld < C, a non-finite weight or smooth, weight <= 0 or smooth < 0. */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const int64_t* target;             /* [N,OH,OW] */
  int32_t ignore_index;
  float weight, smooth, scale;
  float* coef;                       /* [2*C], written */
  float* dice_out;                   /* [1 + C], written */
  float* loss_out;                   /* device scalar, accumulated */
  void* ws;                          /* addk_dice_stats_ws_bytes_classes(N, OH, OW, C) bytes */
} addk_dice_stats_args;
int addk_dice_stats_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
/* The workspace of a launch with C classes: 0 for a C not in addk_head_classes().  The partial rows hold 2 x C floats per workgroup. */
int64_t addk_dice_stats_ws_bytes_classes(int32_t N, int32_t OH, int32_t OW, int32_t C);
/* WARNING: the 19-class size ONLY, = addk_dice_stats_ws_bytes_classes(N, OH, OW, 19); kept for callers from before the class-count list.
 * addk_dice_stats cannot check the size of ws: a launch with C = 21 on a workspace of this size writes past its end.  Size ws with the
 * query above. */
int64_t addk_dice_stats_ws_bytes(int32_t N, int32_t OH, int32_t OW);
int addk_dice_stats(const addk_dice_stats_args* a, void* stream);
/* The loss head with the term's gradient: addk_ce_upsample_kd_fwd_bwd (kd.teacher == NULL: no distillation, and alpha, temperature, nvalid
 * and kd_out are not read; kd.pix_loss == kd.tau == NULL: no mining) whose g additionally gets the bilinear transpose of dz above, with
 * A_c and B_c READ from coef (addk_dice_stats of the same logits and target, earlier on the stream).  The loss partials are the head's
 * own: the term entered loss_out in addk_dice_stats.  With an all-zero coef the gradient is the other entry points'.  ws as for the head
 * it extends: addk_ce_upsample_kd_ws_floats() floats with a teacher, addk_ce_upsample_ws_floats() without.  Supported exactly where
 * addk_ce_upsample_supported() is 1; refuses a null coef and what the head it extends refuses. */
typedef struct {
  addk_ce_upsample_kd_args kd;
  const float* coef;                 /* [2*C] from addk_dice_stats */
} addk_ce_upsample_dice_args;
int addk_ce_upsample_dice_fwd_bwd(const addk_ce_upsample_dice_args* a, void* stream);

/* Per-pixel loss shapes for the fused loss head: what stands in the place of the plain head's w_t * (-log p_t), with p = softmax(z) of the
 * up-sampled logits, t the pixel's target, w_c = class_w[c] (or 1), W = sum_c w_c, s = ce.scale and n = *ce.wsum, the head's normaliser as it is
 * (sum of w_t over the valid pixels, or over the kept ones with a kept set).  The sums run over the valid pixels (with a kept set: the kept ones).
 *   ADDK_CE_SHAPE_FOCAL   gamma >= 1, finite (Lin et al., "Focal Loss for Dense Object Detection"):
 *       loss_out[0] += (s / n) * sum w_t * (1 - p_t)^gamma * (-log p_t)
 *       d / d z_j    = (s / n) * w_t * F * (p_j - [j = t]),    F = (1 - p_t)^(gamma-1) * ((1 - p_t) + gamma * p_t * (-log p_t))
 *     1 - p_t is the sum of the OTHER classes' exponentials over the sum of all; 0^0 = 1 at gamma == 1.
 *   ADDK_CE_SHAPE_SMOOTH  0 < eps < 1: torch.nn.functional.cross_entropy(weight=, ignore_index=, label_smoothing=eps), mean reduction:
 *       loss_out[0] += (s / n) * sum [ (1-eps) * w_t * (-log p_t) + (eps/C) * sum_c w_c * (-log p_c) ]
 *       d / d z_j    = (s / n) * [ (1-eps) * w_t * (p_j - [j = t]) + (eps/C) * (p_j * W - w_j) ]
 *   ADDK_CE_SHAPE_NONE    the call is forwarded to addk_ce_upsample_dice_fwd_bwd (dice.coef set), addk_ce_upsample_kd_fwd_bwd (a teacher),
 *     addk_ce_upsample_ohem_fwd_bwd (a kept set) or addk_ce_upsample_fwd_bwd, whose bits it leaves; gamma and eps are not read.
 * A shaped head composes with a kept set (dice.kd.pix_loss / tau, both or neither: addk_ohem_select chooses the set on the plain per-pixel
 * cross-entropy, as ever) and with the soft-Dice term (dice.coef, or NULL for none: the term goes by the plain predicate, unweighted and
 * unfiltered, as in addk_ce_upsample_dice_fwd_bwd).  It has NO distillation form: a non-NULL dice.kd.teacher is refused.  n == 0 (no valid
 * pixel): the loss word gets 0 and g gets 0 (or stays, with accumulate).  Deterministic as the head it extends; ws holds
 * addk_ce_upsample_ws_floats() floats.  addk_ce_upsample_shaped_supported() is addk_ce_upsample_supported().  Returns ADDK_ERR_INVALID and launches
 * nothing for a shape outside the three, a gamma that is not finite or below 1, an eps outside (0, 1), a teacher, and what the plain head refuses. */
#define ADDK_CE_SHAPE_NONE 0
#define ADDK_CE_SHAPE_FOCAL 1
#define ADDK_CE_SHAPE_SMOOTH 2
typedef struct {
  addk_ce_upsample_dice_args dice;   /* dice.coef == NULL: no soft-Dice term */
  int32_t shape;                     /* ADDK_CE_SHAPE_* */
  float gamma;                       /* read by ADDK_CE_SHAPE_FOCAL */
  float eps;                         /* read by ADDK_CE_SHAPE_SMOOTH */
} addk_ce_upsample_shaped_args;
int addk_ce_upsample_shaped_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
int addk_ce_upsample_shaped_fwd_bwd(const addk_ce_upsample_shaped_args* a, void* stream);

/* Scoring head of a validation pass (train.py:250-322, eval.py:165-193): what the evaluator, the criterion and the entropy
 * meter need of one exit, in ONE pass over the high-resolution pixel grid, straight from the LOW-resolution NHWC logits
 * [N,H,W,C] (bilinear, align_corners=False, the arithmetic of addk_resize_fwd bit for bit) — the [N,C,OH,OW] tensor is never
 * materialised:
 *   cm[gt*C + pred] += 1          int64 [C,C]; pred = arg-max over channels (ties: lowest channel); labels outside [0,C) skipped
 *   loss_out[0]     += scale * sum_valid w[t]*nll / wsum          (definition of addk_ce_upsample_fwd_bwd)
 *   ent_out[0]      += sum_pixels (log sum e - sum e*d / sum e)   (un-normalised, as addk_entropy_sum)
 *   pred_out[n,y,x]  = pred       uint8 [N,OH,OW], optional (NULL: not written)
 * Deterministic: integer atomics for the matrix, fixed-order two-stage sums for the two scalars.  It is a gather (one thread
 * per high-resolution pixel), so the 16-rows-per-input-row limit of addk_ce_upsample_supported does NOT apply here:
 * addk_score_upsample_supported() is 0 only for C not in addk_gate_head_classes(), non-positive sizes or a grid beyond 65535 x 32 rows / 65535 images. */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const int64_t* target;             /* [N,OH,OW] */
  const float* class_w;              /* [C] or NULL */
  int32_t ignore_index;
  const float* wsum;                 /* device scalar from addk_ce_count */
  float scale;
  float* loss_out;                   /* device scalar, accumulated */
  float* ent_out;                    /* device scalar, accumulated */
  int64_t* cm;                       /* [C,C], accumulated */
  uint8_t* pred_out;                 /* [N,OH,OW] or NULL */
  float* ws;                         /* addk_score_upsample_ws_floats() floats */
} addk_score_upsample_args;
int addk_score_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
int64_t addk_score_upsample_ws_floats(int32_t N, int32_t OH, int32_t OW);
int addk_score_upsample(const addk_score_upsample_args* a, void* stream);

/* Early-exit gates that need no trained EDM (modeling/operations.py:161-180; eval.py --confidence entropy|max), on the
 * full-resolution prediction softmax(interpolate(logits, (OH,OW), bilinear, align_corners=False)) straight from the
 * LOW-resolution NHWC logits [N,H,W,C] (the arithmetic of addk_resize_fwd bit for bit; the [N,C,OH,OW] tensor is never
 * materialised), in ONE launch:
 *   out[2n]     = sum_pixels (log sum e - sum e*d / sum e) / (log 19 * OH*OW)    normalised Shannon entropy of image n (addk_gate_head_classes)
 *   out[2n + 1] = #{pixels: pmax > *max_thr} / (OH*OW),  pmax = 1 / sum_c exp(z_c - max_c z)   (operations.py:172-180)
 * max_thr is read from memory when the launch runs, so a captured graph serves every threshold.  out_host: optional
 * host-mapped (pinned) [N][2] words that receive the same bits — the host gate then needs no device-to-host copy, only
 * the completion of the launch.  ws: addk_gate_upsample_ws_bytes() bytes, ZERO-initialised once (the kernel leaves its
 * ticket word at zero: replayable from a hipGraph).  Deterministic: the last-arriving workgroup adds the per-workgroup
 * partials in a fixed order.  addk_gate_upsample_supported() is 0 for C not in addk_gate_head_classes(), non-positive sizes or a grid beyond
 * 65535 x 32 rows / 65535 images (the limits of addk_score_upsample_supported); addk_gate_upsample then returns
 * ADDK_ERR_INVALID without launching. */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const float* max_thr;              /* device-readable word: threshold of the 'max' gate */
  float* out;                        /* device [N][2]: (entropy, share) */
  float* out_host;                   /* pinned host [N][2] or NULL */
  void* ws;                          /* addk_gate_upsample_ws_bytes() zero-initialised bytes */
} addk_gate_upsample_args;
int addk_gate_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
int64_t addk_gate_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW);
int addk_gate_upsample(const addk_gate_upsample_args* a, void* stream);

/* Label head of an inference exit (decoder.py:28 + eval.py:218-221): the arg-max over channels of the up-sampled logits, one
 * byte per high-resolution pixel, straight from the LOW-resolution NHWC logits [N,H,W,C] (the arithmetic of addk_resize_fwd
 * bit for bit; the [N,C,OH,OW] tensor is never materialised), in ONE launch:
 *   labels[n,y,x] = pred, or lut256[pred];  pred = arg-max over channels (ties: lowest channel) — the bytes of
 *                   addk_score_upsample's pred_out and of addk_argmax_nchw on addk_resize_fwd's NCHW output
 * No workspace, no atomics: deterministic.  addk_label_upsample_supported() == addk_score_upsample_supported(); where it is 0
 * addk_label_upsample returns ADDK_ERR_INVALID without launching. */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const uint8_t* lut256;             /* NULL: the class index; else lut256[class] (e.g. train id -> Cityscapes labelId) */
  uint8_t* labels;                   /* [N,OH,OW] */
} addk_label_upsample_args;
int addk_label_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C);
int addk_label_upsample(const addk_label_upsample_args* a, void* stream);

/* The gate launch that also leaves the label map: addk_gate_upsample and addk_label_upsample in ONE walk.  out / out_host
 * receive the bits of addk_gate_upsample on the same input with the same *max_thr, labels the bytes of addk_label_upsample;
 * the map is written for every image, whatever the host then decides (one byte per pixel).  gate.ws: the workspace of
 * addk_gate_upsample (addk_gate_upsample_ws_bytes() zero-initialised bytes, ticket word left at zero: replayable from a
 * hipGraph).  Supported exactly where addk_gate_upsample_supported() is 1; otherwise ADDK_ERR_INVALID without launching. */
typedef struct {
  addk_gate_upsample_args gate;
  const uint8_t* lut256;             /* NULL: the class index; else lut256[class] */
  uint8_t* labels;                   /* [N,OH,OW] */
} addk_gate_label_upsample_args;
int addk_gate_label_upsample(const addk_gate_label_upsample_args* a, void* stream);

/* Multi-view label head (multi-scale + flip inference): the arg-max of the weighted mean of the class probabilities of up to
 * ADDK_MAX_VIEWS views of the same N images, each a LOW-resolution NHWC logits map of its own size (H, W) — larger or smaller
 * than (OH, OW) — in ONE launch; no [N,C,OH,OW] tensor exists for any view.  For output pixel (n, Y, X), views in order:
 *   Xv   = mirror ? OW-1-X : X
 *   z_v  = bilinear sample (align_corners=False) of image n0 + n of the view at (Y, Xv): the bits addk_resize_fwd writes there
 *   p_v  = softmax(z_v) in fp32 (max subtracted);  acc[c] += weight * p_v[c]
 *   labels[n,Y,X] = am, or lut256[am];  am = arg-max of acc (strict >: a tie keeps the lowest channel)
 * The mirrored half of a batch-2N logits tensor is addressed with n0 = N.  No workspace, no atomics: deterministic.
 * addk_label_views_upsample_supported() is 0 for nview outside 1..ADDK_MAX_VIEWS, C not in addk_gate_head_classes(), non-positive sizes or a grid beyond
 * 65535 x 16 rows / 65535 images; addk_label_views_upsample then returns ADDK_ERR_INVALID without launching, as it does for a
 * null pointer, a view with a non-positive size or a stride below C, and a weight that is not positive and finite. */
#define ADDK_MAX_VIEWS 8
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C; this view's image n is logits[n0 + n] */
  int32_t n0, H, W, mirror;
  float weight;
} addk_view;
typedef struct {
  addk_view view[ADDK_MAX_VIEWS];
  int32_t nview, N, C, OH, OW;
  const uint8_t* lut256;             /* NULL: the class index; else lut256[class] */
  uint8_t* labels;                   /* [N,OH,OW] */
} addk_label_views_args;
int addk_label_views_upsample_supported(int32_t nview, int32_t N, int32_t OH, int32_t OW, int32_t C);
int addk_label_views_upsample(const addk_label_views_args* a, void* stream);

/* Sliding-window (tiled) label maps: a plan of one fixed window size (th, tw) serves images of any size.  The windows of an image form
 * a grid of ny x nx origins (segment.tile_starts: the first at 0, the last clamped to the image edge, consecutive windows touch or overlap;
 * an image smaller than the window is one window, zero-padded).
 *
 * addk_gather_tiles fills the plan's resident NCHW input x [B,Cin,th,tw] from a table of window descriptors in DEVICE memory, in ONE
 * launch: slot b < ntiles gets image[c][y0 + i][x0 + j], 0.0f where that lies outside the image (the reference's ZeroPad2d after
 * Normalize); the slots ntiles <= b < B are zero-filled.  Every descriptor names its own image and size, so windows of images of different
 * sizes share a chunk.  Returns ADDK_ERR_INVALID without launching for a null pointer (the table may be null when ntiles == 0), ntiles
 * outside 0..B and non-positive sizes. */
typedef struct { const float* image; int32_t H, W, y0, x0; } addk_tile_desc;  /* image: NCHW planes of ONE image, [Cin][H][W] */
int addk_gather_tiles(const addk_tile_desc* tiles_dev, int32_t ntiles, int32_t Cin, int32_t th, int32_t tw,
                      float* x, int32_t B, void* stream);

/* Tiled label head: the arg-max of the summed class probabilities of every window that covers a pixel, in ONE launch over the stored
 * LOW-resolution NHWC logits of the windows; no [T,C,th,tw] tensor and no full-resolution probability buffer exists.  For output pixel
 * (n, Y, X), over the tiles (iy, ix) with y0[iy] <= Y < y0[iy] + th and x0[ix] <= X < x0[ix] + tw, ascending iy, then ascending ix:
 *   z      = bilinear sample (align_corners=False, scales h/th and w/tw) of the tile's logits at (Y - y0[iy], X - x0[ix]): the bits
 *            addk_resize_fwd writes there when it resizes (h, w) to (th, tw)
 *   e[c]   = exp(z[c] - max z);  acc[c] += (1.0f / sum e) * e[c]            (addk_label_views_upsample's expression, weight 1)
 *   labels[n,Y,X] = am, or lut256[am];  am = arg-max of acc (strict >: a tie keeps the lowest channel)
 * The sum is not divided by the cover count (the arg-max does not need it); the part of a tile beyond the image (OH < th) is never
 * sampled.  No workspace, no atomics: deterministic.
 * addk_label_tiles_upsample_supported() is 0 for C not in addk_head_classes(), ny or nx outside 1..ADDK_MAX_TILES_AXIS, non-positive
 * sizes or a grid beyond 65535 x 16 rows / 65535 images; addk_label_tiles_upsample then returns ADDK_ERR_INVALID without launching, as it
 * does for a null logits / labels pointer, non-positive h, w, th, tw, ld < C, t0 < 0, and origins that are no window grid of the image:
 * y0[0] != 0, not strictly increasing, a gap (y0[i+1] > y0[i] + th), an origin at or beyond the image, a last window that ends before
 * the image does (y0[ny-1] + th < OH); likewise x0. */
#define ADDK_MAX_TILES_AXIS 16
typedef struct {
  const float* logits; int32_t ld;   /* store of low-resolution NHWC tile logits: tile t is [h][w] pixels of stride ld >= C at logits + t*h*w*ld */
  int32_t h, w;                      /* a tile's low-resolution grid */
  int32_t th, tw;                    /* a tile's size in output pixels */
  int32_t N, C, OH, OW;              /* N images of one size (OH, OW) */
  int32_t t0, ny, nx;                /* image n's tile (iy, ix) is tile t0 + (n*ny + iy)*nx + ix */
  int32_t y0[ADDK_MAX_TILES_AXIS], x0[ADDK_MAX_TILES_AXIS];
  const uint8_t* lut256;             /* NULL: the class index; else lut256[class] */
  uint8_t* labels;                   /* [N,OH,OW] */
} addk_label_tiles_args;
int addk_label_tiles_upsample_supported(int32_t N, int32_t OH, int32_t OW, int32_t ny, int32_t nx, int32_t C);
int addk_label_tiles_upsample(const addk_label_tiles_args* a, void* stream);

/* Multi-scale + flip sliding windows (segment.TiledSegmenter with scales / flip): a view v of an image (OH, OW) is (scale, mirror, weight);
 * its scaled image S_v is the bilinear resize (align_corners=False) of the image to (Hv, Wv) = segment.view_size(OH, OW, scale), flipped
 * along the width if `mirror`; the windows of the view are tile_starts(Hv, th, sy) x tile_starts(Wv, tw, sx) over S_v.
 *
 * addk_gather_tile_views is addk_gather_tiles over S_v, which is never materialised: slot b < ntiles, plane c, position (i, j) gets, with
 * sy = y0 + i and sx = x0 + j, 0.0f outside [0, Hv) x [0, Wv) and else the bilinear sample of plane c of the (H, W) -> (Hv, Wv) resize at
 * (sy, mirror ? Wv-1-sx : sx), computed with the index arithmetic and the lerp expression of addk_resize_fwd (the bits it writes there).
 * A descriptor with Hv == H, Wv == W, mirror == 0 copies the pixel: addk_gather_tiles' bytes.  Slots >= ntiles are zero.  The refusals
 * are addk_gather_tiles'; the table lives in device memory, so a descriptor with a non-positive Hv or Wv is refused where it is read:
 * nothing of its image is touched and its slot is zero. */
typedef struct { const float* image; int32_t H, W, Hv, Wv, y0, x0, mirror; } addk_tile_view_desc;  /* image: [Cin][H][W] of ONE image */
int addk_gather_tile_views(const addk_tile_view_desc* tiles_dev, int32_t ntiles, int32_t Cin, int32_t th, int32_t tw,
                           float* x, int32_t B, void* stream);

/* Tiled multi-view label head: the arg-max of the weighted mean, over up to ADDK_MAX_VIEWS views, of the mean class probabilities of the
 * windows of the view that cover a pixel, in ONE launch over the stored low-resolution NHWC logits of every view's windows.  For output
 * pixel (n, Y, X), views in order:
 *   Xm = mirror ? OW-1-X : X;   u_y = (Y + 1/2) * Hv / OH,  u_x = (Xm + 1/2) * Wv / OW       (the pixel centre in S_v's coordinates)
 *   window (iy, ix) covers the pixel iff y0 <= u_y < y0 + th and x0 <= u_x < x0 + tw, decided in 64-bit integers:
 *   2*OH*y0 <= (2Y+1)*Hv < 2*OH*(y0 + th), likewise x.  k = (covering window rows) * (covering window columns) >= 1.
 *   for every covering window, ascending iy, then ix:
 *     z    = bilinear sample of the window's logits at a_y = (u_y - y0) * h/th - 1/2, a_x = (u_x - x0) * w/tw - 1/2 with the border rule of
 *            addk_resize_fwd (a < 0 -> 0, i0 = floor(a) capped at h-1, i1 = min(i0+1, h-1), lambda = a - i0), all in fp32
 *     e[c] = exp(z[c] - max z);  acc[c] += ((weight / k) / sum e) * e[c]
 *   labels[n,Y,X] = am, or lut256[am];  am = arg-max of acc (strict >: a tie keeps the lowest channel)
 * Image n's window (iy, ix) of view v is tile t0_v + (n*ny_v + iy)*nx_v + ix of the store.  With one view of Hv == OH, Wv == OW, no mirror,
 * weight 1 on a grid without overlap this is addk_label_tiles_upsample, bit for bit.  No workspace, no atomics: deterministic.
 * addk_label_tile_views_upsample_supported() is 0 for nview outside 1..ADDK_MAX_VIEWS, C not in addk_head_classes(), non-positive sizes or
 * a grid beyond 65535 x 16 rows / 65535 images; addk_label_tile_views_upsample then returns ADDK_ERR_INVALID without launching, as it does
 * for a null logits / labels pointer, non-positive h, w, th, tw, ld < C, and per view: ny or nx outside 1..ADDK_MAX_TILES_AXIS, non-positive
 * Hv or Wv, t0 < 0, a weight that is not positive and finite, and origins that are no window grid of (Hv, Wv) (addk_label_tiles_upsample's rule). */
typedef struct {
  int32_t Hv, Wv;                    /* the view's scaled image */
  int32_t t0, ny, nx;                /* image n's window (iy, ix) is tile t0 + (n*ny + iy)*nx + ix */
  int32_t mirror;
  float weight;
  int32_t y0[ADDK_MAX_TILES_AXIS], x0[ADDK_MAX_TILES_AXIS];      /* origins in the scaled image */
} addk_tile_view;
typedef struct {
  addk_tile_view view[ADDK_MAX_VIEWS];
  int32_t nview;
  const float* logits; int32_t ld;   /* the store: tile t is [h][w] pixels of stride ld >= C at logits + t*h*w*ld */
  int32_t h, w;                      /* a window's low-resolution grid */
  int32_t th, tw;                    /* a window's size in pixels of a scaled image */
  int32_t N, C, OH, OW;              /* N images of one size (OH, OW) */
  const uint8_t* lut256;             /* NULL: the class index; else lut256[class] */
  uint8_t* labels;                   /* [N,OH,OW] */
} addk_label_tile_views_args;
int addk_label_tile_views_upsample_supported(int32_t nview, int32_t N, int32_t OH, int32_t OW, int32_t C);
int addk_label_tile_views_upsample(const addk_label_tile_views_args* a, void* stream);

/* Per-window early exits of the sliding window (segment.TiledSegmenter with `threshold`; csrc/tiles.hip).
 *
 * addk_gate_tiles_upsample is the gate of up to B windows of one chunk over their VALID EXTENT, in ONE launch, from the tile plan's
 * low-resolution NHWC logits [B,h,w,ld].  A window that hangs over its image's edge is zero-padded (addk_gather_tiles), and the padding
 * predicts one class with confidence: judged over the whole window such a window would leave early.  For slot b < nb with the extent
 * (vh, vw) = ext[b], clamped in the kernel to 1..th and 1..tw (device data: the host cannot check it):
 *   z          = the bilinear sample addk_resize_fwd writes at (Y, X) when it resizes (h, w) to (th, tw); s = *inv_temp, or 1 when it is NULL
 *   d          = (z - max z) * s,  e = exp(d)                                     (addk_gate_upsample_t's sweep)
 *   out[2b]     = sum over Y < vh, X < vw of (log sum e - sum e*d / sum e) / (log C * vh*vw)          normalised Shannon entropy
 *   out[2b + 1] = #{Y < vh, X < vw: 1 / sum e > *max_thr} / (vh*vw)
 * With the full extent, C == 19 and inv_temp NULL these are addk_gate_upsample's words.  Slots b >= nb are not written (nb == 0 launches
 * nothing).  max_thr, inv_temp and ext are read when the launch runs, so a captured graph serves every threshold, temperature and chunk.
 * out_host: optional pinned [B][2] words that receive the same bits.  ws: addk_gate_tiles_upsample_ws_bytes() bytes, ZERO-initialised
 * once (the ticket word is left at zero: replayable from a hipGraph).  Deterministic: the last-arriving workgroup adds the per-workgroup
 * partials in a fixed order.  addk_gate_tiles_upsample_supported() is 0 for C not in addk_head_classes(), non-positive sizes or a grid
 * beyond 65535 x 32 rows / 65535 slots; addk_gate_tiles_upsample then returns ADDK_ERR_INVALID without launching, as it does for a null
 * logits / ext / max_thr / out / ws pointer, nb outside 0..B and ld < C. */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC [B,h,w,ld], pixel stride ld >= C */
  int32_t B, nb;                     /* slots of the plan; windows of this chunk, 0..B */
  int32_t h, w, C, th, tw;           /* a window's low-resolution grid, classes, a window's size */
  const int32_t* ext;                /* device [B][2]: (vh, vw) of every slot */
  const float* max_thr;              /* device-readable word: threshold of the 'max' gate */
  const float* inv_temp;             /* device-readable word 1 / temperature, or NULL */
  float* out;                        /* device [B][2]: (entropy, share) */
  float* out_host;                   /* pinned host [B][2] or NULL */
  void* ws;                          /* addk_gate_tiles_upsample_ws_bytes() zero-initialised bytes */
} addk_gate_tiles_args;
int addk_gate_tiles_upsample_supported(int32_t B, int32_t h, int32_t w, int32_t th, int32_t tw, int32_t C);
int64_t addk_gate_tiles_upsample_ws_bytes(int32_t B, int32_t th, int32_t tw);
int addk_gate_tiles_upsample(const addk_gate_tiles_args* a, void* stream);

/* addk_scatter_tile_logits copies the low-resolution logits of the windows that leave into the store the tiled label heads read, in ONE
 * launch: for i < n, the first C channels of row src_row[i] of src [B,h,w,lds] go to tile dst_tile[i] of store [T,h,w,ld], and the
 * store's padding channels C..ld-1 of those tiles are written as zero.  src_row and dst_tile are DEVICE memory, read when the launch
 * runs (src_row NULL stands for 0..n-1); an index outside 0..B-1 / 0..T-1 is skipped in the kernel.  Two entries of dst_tile must differ.
 * 16-byte accesses where both strides and both bases allow them, single floats otherwise; nothing outside the named tiles is written.
 * No atomics, no workspace: deterministic.  n == 0 launches nothing.  Returns ADDK_ERR_INVALID without launching for a null src / store /
 * dst_tile pointer, n outside 0..B, non-positive B, T, h, w, C, and lds < C or ld < C. */
typedef struct {
  const float* src; int32_t lds;     /* the plan's logits [B,h,w,lds] */
  int32_t B;
  float* store; int32_t ld;          /* [T,h,w,ld] */
  int32_t T;
  int32_t h, w, C;
  const int32_t* src_row;            /* device [n], or NULL: 0..n-1 */
  const int32_t* dst_tile;           /* device [n] */
  int32_t n;
} addk_scatter_tile_logits_args;
int addk_scatter_tile_logits(const addk_scatter_tile_logits_args* a, void* stream);

/* Exit profile of a validation pass (eval.py:195-230): what the early-exit operating curve needs of one exit, PER IMAGE, in
 * ONE launch over the LOW-resolution NHWC logits [N,H,W,C] (the walk and the arithmetic of the two heads above):
 *   ent_out[n]            = normalised Shannon entropy of image n: the bits of addk_gate_upsample's out[2n]
 *   share_out[n*nthr + j] = #{pixels of image n: pmax > thr[j]} / (OH*OW): the bits of addk_gate_upsample's out[2n + 1]
 *                           launched with *max_thr == thr[j]; 0 <= nthr <= 16 (nthr == 0: thr and share_out may be NULL)
 *   cm[n][gt*C + pred]   += 1     int64 [N,C,C], the rule of addk_score_upsample (labels outside [0,C) skipped, ties: lowest
 *                                 channel); ADDED to what cm holds: the caller zeroes it
 *   pred_out[n,y,x]       = pred  uint8 [N,OH,OW], optional (NULL: not written)
 * No loss.  thr is read from memory when the launch runs, so a captured graph serves every threshold set of one length.
 * ws: addk_profile_upsample_ws_bytes() bytes, ZERO-initialised once (the ticket word is left at zero).  Deterministic: integer
 * atomics for the matrix, the gate's fixed-order sum by the last-arriving workgroup for the rest.
 * addk_profile_upsample_supported() is 0 where addk_score_upsample_supported() is, and for nthr outside [0, 16];
 * addk_profile_upsample then returns ADDK_ERR_INVALID without launching. */
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const int64_t* target;             /* [N,OH,OW] */
  const float* thr;                  /* device [nthr]: thresholds of the top probability */
  int32_t nthr;
  float* ent_out;                    /* device [N] */
  float* share_out;                  /* device [N][nthr] */
  int64_t* cm;                       /* device [N][C,C], accumulated */
  uint8_t* pred_out;                 /* [N,OH,OW] or NULL */
  void* ws;                          /* addk_profile_upsample_ws_bytes() zero-initialised bytes */
} addk_profile_upsample_args;
int addk_profile_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C, int32_t nthr);
int64_t addk_profile_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW);
int addk_profile_upsample(const addk_profile_upsample_args* a, void* stream);

/* Tempered gate and profile: the launches above with every per-pixel probability taken from softmax(z * *inv_temp) instead of
 * softmax(z) — d = (z - max z) * *inv_temp, then the same sweep (sum e, sum e*d), entropy term, top probability 1 / sum e and
 * comparison.  inv_temp: one device-readable word, the inverse of a temperature (positive, finite), read when the launch runs, so
 * a captured graph serves every temperature.  With *inv_temp == 1.0f the outputs carry the bits of the untempered launch on the
 * same input (a multiply by 1.0f is exact; nothing else differs).  The arg-max does not depend on the temperature: labels,
 * pred_out and cm are the bytes of the untempered launches at any temperature.
 * addk_gate_upsample_t: labels == NULL is addk_gate_upsample (lut256 is ignored), otherwise addk_gate_label_upsample.
 * Workspaces, support predicates and refusals are those of the launch each one tempers; a null inv_temp is refused as well. */
typedef struct {
  addk_gate_upsample_args gate;
  const float* inv_temp;             /* device-readable word: 1 / temperature */
  const uint8_t* lut256;             /* NULL: the class index; else lut256[class] */
  uint8_t* labels;                   /* [N,OH,OW], or NULL: the gate alone */
} addk_gate_upsample_t_args;
int addk_gate_upsample_t(const addk_gate_upsample_t_args* a, void* stream);
typedef struct {
  addk_profile_upsample_args profile;
  const float* inv_temp;             /* device-readable word: 1 / temperature */
} addk_profile_upsample_t_args;
int addk_profile_upsample_t(const addk_profile_upsample_t_args* a, void* stream);

/* Calibration head (temperature scaling, Guo et al. 2017): what the reliability diagram, the expected calibration error and the
 * fit of one temperature need of one exit, for up to ADDK_CALIB_MAX_T temperatures at once, in ONE launch over the LOW-resolution
 * NHWC logits [N,H,W,C] (the walk and the bilinear arithmetic of the heads above: z carries the bits addk_resize_fwd writes; no
 * [N,C,OH,OW] tensor exists).  Per pixel whose target t lies in [0, C) (the evaluator's mask, as addk_profile_upsample), with
 * mx = max z and am = arg-max z (strict >: a tie keeps the lowest channel), and per temperature j:
 *   se_j   = sum_c exp((z_c - mx) * inv_temp[j])        every exponent <= 0: nothing overflows for any temperature
 *   nll_j  = log(se_j) - (z_t - mx) * inv_temp[j]
 *   conf_j = 1 / se_j,   b = min(ADDK_CALIB_BINS - 1, (int)(conf_j * ADDK_CALIB_BINS))
 *   bins[j][b] += (1, am == t, llrintf(conf_j * 2^24));   nll[j] += nll_j
 * Both outputs are ADDED to: the caller zeroes them.  Deterministic: the bins take integer atomics (into replicas inside ws, which
 * the last-arriving workgroup sums into bins and leaves at zero); the NLL leaves every workgroup as one fp32 partial per temperature,
 * and the last-arriving workgroup adds them in a fixed order in fp64 and adds the launch's sum to nll[j] once.  No floating-point
 * atomics.  ws: addk_calib_upsample_ws_bytes() bytes, ZERO-initialised once (the ticket word is
 * left at zero: replayable from a hipGraph).  addk_calib_upsample_supported() is 0 where addk_score_upsample_supported() is, and for
 * nt outside [1, ADDK_CALIB_MAX_T]; addk_calib_upsample then returns ADDK_ERR_INVALID without launching, as it does for a null
 * pointer or ld < C. */
#define ADDK_CALIB_MAX_T 8
#define ADDK_CALIB_BINS 16
typedef struct {
  const float* logits; int32_t ld;   /* NHWC, pixel stride ld >= C */
  int32_t N, H, W, C, OH, OW;
  const int64_t* target;             /* [N,OH,OW] */
  const float* inv_temp; int32_t nt; /* device [nt]: 1 / temperature, read when the launch runs */
  int64_t* bins;                     /* device [nt][ADDK_CALIB_BINS][3]: count, hits, confidence sum in units of 2^-24; accumulated */
  double* nll;                       /* device [nt]: sum of the NLL over the counted pixels; accumulated */
  void* ws;                          /* addk_calib_upsample_ws_bytes() zero-initialised bytes */
} addk_calib_upsample_args;
int addk_calib_upsample_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C, int32_t nt);
int64_t addk_calib_upsample_ws_bytes(int32_t N, int32_t OH, int32_t OW);
int addk_calib_upsample(const addk_calib_upsample_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused SGD (torch.optim.SGD(momentum, weight_decay, nesterov), train.py:126) on a flat buffer.
 *   d = g*gscale + wd*p;  buf = first ? d : mom*buf + d;  p -= lr*(nesterov ? d + mom*buf : buf)
 * lr is read from device memory so a captured graph can be replayed with a new poly-LR value.
 * ------------------------------------------------------------------------------------- */
int addk_sgd_step(float* p, const float* g, float* buf, int64_t n, const float* lr_dev, float momentum,
                  float weight_decay, int32_t nesterov, int32_t first, float gscale, void* stream);

/* ---------------------------------------------------------------------------------------
 * Earlier-Decision-Maker head in ONE launch (ADD.py:502-525, the gate of dynamic_inference ADD.py:420-423):
 *   relu?(a*x+b) -> conv 3x3 stride 2 pad 1, C -> 128, no bias -> ReLU -> global average pool -> Linear 128-64 -> ReLU
 *   -> Linear 64-32 -> ReLU -> Linear 32-1.   out[n * ldo] = confidence of image n.
 * conv_w: [128][3][3][C] (a torch [128,C,3,3] tensor in channels_last memory); w1 [64][128], w2 [32][64], w3 [1][32] row-major
 * (torch Linear weights), b1/b2/b3 their biases.  ws: addk_edm_head_ws_bytes() bytes, ZERO-initialised once (the kernel leaves its
 * ticket word at zero, so the launch can be replayed from a hipGraph).  out_host: optional host-mapped (pinned) word the confidence is
 * ALSO written to — the host gate then needs no device-to-host copy, only the completion of the launch.
 * ------------------------------------------------------------------------------------- */
typedef struct addk_edm_args {
  addk_src src; int32_t N, H, W;
  int32_t ldo;                /* out[n * ldo] = confidence of image n (an [N,1,1,1] NHWC tensor with a padded pixel stride); >= 1 */
  const float* conv_w;
  const float* w1; const float* b1; const float* w2; const float* b2; const float* w3; const float* b3;
  float* out; float* out_host;
  void* ws;
} addk_edm_args;
int64_t addk_edm_head_ws_bytes(int32_t N, int32_t H, int32_t W);
int addk_edm_head_supported(const addk_edm_args* a);
int addk_edm_head(const addk_edm_args* a, void* stream);

/* misc */
int addk_fill(float* p, int64_t n, float v, void* stream);
/* Earlier-Decision-Maker support (operations.py:161-170): per-pixel normalised entropy summed */
int addk_entropy_sum(const float* logits_nchw, int32_t N, int32_t C, int64_t HW, float* out1, float* ws, void* stream);
/* argmax over channels of NCHW logits -> int64 [N,HW], and confusion matrix accumulation
 * (utils/metrics.py:34-43) */
int addk_argmax_nchw(const float* logits, int32_t N, int32_t C, int64_t HW, int64_t* out, void* stream);
int addk_confusion(const int64_t* gt, const int64_t* pred, int64_t n, int32_t num_class, int64_t* cm, void* stream);

/* ---------------------------------------------------------------------------------------
 * Boundary-band ("trimap") confusion (csrc/trimap.hip): the confusion matrix restricted to the pixels within d pixels of a ground-truth
 * class boundary, for a ladder of d (the trimap plot of the DeepLab papers).  Integer-only; the semantics are this project's own.
 *
 * For one image with target t (int64 [OH,OW]) and C classes:
 *   valid(p)  : 0 <= t(p) < C, compared as 64-bit values.
 *   E(p)      : p is an EDGE pixel when valid(p) and some 4-neighbour q INSIDE THE SAME IMAGE has valid(q) and t(q) != t(p).  The image
 *               border makes no edge; a neighbour that is ignore or out of range makes no edge; two different invalid values make none.
 *   D2(p)     : min over the edge pixels e of the same image of (py-ey)^2 + (px-ex)^2 (squared Euclidean distance; 0 on an edge pixel).
 *   dist[p]   : the smallest integer k >= 0 with k*k >= D2(p) when k <= radius; otherwise, and when the image has no edge pixel,
 *               ADDK_TRIMAP_FAR.  1 <= radius <= ADDK_TRIMAP_MAX_RADIUS.  For an integer d <= radius, "p lies within d of a
 *               boundary" is exactly dist[p] <= d.  dist is defined for every pixel, valid or not.
 * The definition is separable and the kernels use that form: h(y,x) = min |x-x'| over E(y,x'), and
 * D2(y,x) = min over |dy| <= radius of dy^2 + h(y+dy,x)^2 with h <= radius (a nearest edge pixel within the radius has both offsets
 * within it, so the windowed search is exact).  It is Euclidean, not Chebyshev or Manhattan: one foreign pixel in a uniform field
 * gives discs.
 *
 * addk_boundary_dist: two launches on `stream` — edge flags (64-bit ballot words) and the row distance h as bytes into ws, then the
 * column pass over an LDS tile of h with a halo of `radius` rows that never crosses an image.  ws needs no initialisation.
 *
 * Banded confusion, for strictly ascending integer widths w[0..nw) with 0 <= w[j] <= 254 and nw <= ADDK_TRIMAP_MAX_WIDTHS:
 *   ring j holds the pixels with w[j-1] < dist <= w[j] (w[-1] = -1).  A pixel is counted when valid(p), pred[p] < C and
 *   dist[p] <= w[nw-1]; it adds 1 to cm[ring][t*C + pred].  The rings are disjoint (one atomic per pixel); the matrix "within w[j]"
 *   is the prefix sum over the rings, taken by the caller.  A pred byte >= C is skipped, never used as an index.
 * addk_confusion_banded: one launch; per-workgroup LDS histograms flushed with 64-bit integer atomics.
 *
 * *_supported is 0 for non-positive sizes, C outside [1, 32], radius outside [1, ADDK_TRIMAP_MAX_RADIUS], nw outside
 * [1, ADDK_TRIMAP_MAX_WIDTHS] and N*OH*OW >= 2^31.  The launchers return ADDK_ERR_INVALID WITHOUT launching where *_supported is 0,
 * for a null pointer, for widths that are not strictly ascending or outside [0, 254], and for 0 < image_stride < nw*C*C.  Both work on
 * the stream only (no host reads, no memsets, no state left behind: a captured hipGraph replays them), and their only atomics are
 * integer atomics: two calls give equal bits.
 * ------------------------------------------------------------------------------------- */
#define ADDK_TRIMAP_MAX_RADIUS 64
#define ADDK_TRIMAP_MAX_WIDTHS 8
#define ADDK_TRIMAP_FAR 255
typedef struct {
  const int64_t* target;            /* [N,OH,OW] */
  int32_t N, OH, OW, C, radius;
  uint8_t* dist;                    /* [N,OH,OW], written (every byte) */
  void* ws;                         /* addk_boundary_dist_ws_bytes() bytes, needs no initialisation */
} addk_boundary_dist_args;
int     addk_boundary_dist_supported(int32_t N, int32_t OH, int32_t OW, int32_t C, int32_t radius);
int64_t addk_boundary_dist_ws_bytes(int32_t N, int32_t OH, int32_t OW);
int     addk_boundary_dist(const addk_boundary_dist_args* a, void* stream);

typedef struct {
  const int64_t* target; const uint8_t* pred; const uint8_t* dist;   /* [N,OH,OW] each */
  int32_t N, OH, OW, C, nw;
  int32_t width[ADDK_TRIMAP_MAX_WIDTHS];
  int64_t* cm;                      /* ring matrices, ADDED to: the caller zeroes them */
  int64_t image_stride;             /* 0: one set [nw][C][C] for the batch; else int64 words between the sets of
                                       consecutive images (>= nw*C*C): per-image matrices */
} addk_confusion_banded_args;
int addk_confusion_banded_supported(int32_t N, int32_t OH, int32_t OW, int32_t C, int32_t nw);
int addk_confusion_banded(const addk_confusion_banded_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * Row gather / scatter over several buffers in ONE launch (csrc/rows.hip): batch compaction of batched dynamic inference
 * (dynamic.BatchedGate).  Every item is a buffer of equal-sized rows (one row per image); for every item i and every r < nrows the launch
 * copies row_bytes bytes from  src + src_row[r] * row_bytes  to  dst + dst_row[r] * row_bytes.  A NULL index array stands for 0..nrows-1.
 * The same entry point compacts the survivors' activations into the buffers of a smaller plan (dst_row NULL) and scatters label rows
 * to their original indices (src_row = rows of the exit's map, dst_row = original indices, row_bytes = H*W).
 *   - items, src_row, dst_row are DEVICE memory.  The indices are read when the launch RUNS, so a table built once serves every call
 *     and only the index words change between calls.
 *   - Sources and destinations NEVER overlap (they belong to different plans); rows that overlap give undefined bytes.  Two rows of
 *     dst_row must differ.
 *   - Any row_bytes >= 1 and any alignment: 16-byte accesses where a row's source and destination share their offset inside a 16-byte
 *     line (4-byte accesses where they share it inside a word, bytes otherwise), single bytes at the two ends of a row; nothing outside
 *     the destination rows is written.  No atomics, no workspace: deterministic.
 *   - The work is cut into units of 16 KiB of one row; workgroups walk the units of all items in one sequence (a running prefix over the
 *     items), so items that differ in size by orders of magnitude load the grid evenly.
 * The launch function reads the item table back (a stream-ordered copy of nitems entries and a wait on `stream`) to check it and to
 * count the units; it therefore cannot be captured into a hipGraph (ADDK_ERR_INVALID while `stream` is capturing).
 * Returns ADDK_ERR_INVALID and launches nothing for a null argument struct, table or item pointer, nitems < 1 or > 65536, nrows < 1,
 * row_bytes < 1, or more than 2^31 - 1 units.
 * ------------------------------------------------------------------------------------- */
typedef struct { const void* src; void* dst; int64_t row_bytes; } addk_rows_item;
typedef struct {
  const addk_rows_item* items; int32_t nitems;   /* device table */
  const int32_t* src_row; const int32_t* dst_row;/* device [nrows]; NULL = 0..nrows-1 */
  int32_t nrows;
} addk_gather_rows_args;
int addk_gather_rows(const addk_gather_rows_args* a, void* stream);

/* ---------------------------------------------------------------------------------------
 * GPU input pipeline: Cityscapes sample preparation from DECODED 8-bit planes (reference
 * dataloaders/datasets/cityscapes.py:64-91 encode_segmap; dataloaders/custom_transforms.py:238-286 train_preprocess,
 * :322-347 full_image_eval_preprocess).  Bit-exact with the reference's PIL calls: the resampling tables are built on the
 * host with PIL's own arithmetic (addk/data.py) and the kernels apply them in PIL's fixed point.
 * ------------------------------------------------------------------------------------- */
int addk_lut_u8(const uint8_t* in, uint8_t* out, int64_t n, const uint8_t* lut256, void* stream);
/* one pass of the antialiased 8-bit resize (interleaved C channels): out = clip8(((1<<21) + sum_k in*coef[k]) >> 22);
 * bounds[2*o] = first source index, bounds[2*o+1] = tap count of output index o; coef is [out extent][ksize] int32.
 * vertical = 0: along x (mirror = 1 reads the row right-to-left: the random flip); vertical = 1: along y. */
int addk_resample_u8(const uint8_t* in, int32_t IH, int32_t IW, uint8_t* out, int32_t OH, int32_t OW, int32_t C, const int32_t* bounds,
                     const int32_t* coef, int32_t ksize, int32_t vertical, int32_t mirror, void* stream);
/* NEAREST resize of a label plane through source-index tables (xtab[OW], ytab[OH]) */
int addk_nearest_u8(const uint8_t* in, int32_t IH, int32_t IW, uint8_t* out, int32_t OH, int32_t OW, const int32_t* xtab, const int32_t* ytab,
                    int32_t mirror, void* stream);
/* ToTensor + Normalize + pad (image 0, label 255) + crop at (i0, j0): HWC u8 -> CHW float [3][CH][CW], labels -> int64 [CH][CW] (lbl/out_lbl may be NULL) */
int addk_finish_sample(const uint8_t* img, const uint8_t* lbl, int32_t IH, int32_t IW, int32_t i0, int32_t j0, int32_t CH, int32_t CW,
                       const float* mean3, const float* std3, float* out_img, int64_t* out_lbl, void* stream);

/* ---- small-message all-reduce of the SyncBN statistics inside one node (csrc/comm.hip) -------------------------------------------------
 * Replaces, for the (sum, sumsq) / (dmean, dvar) vectors of the BatchNorms of one dependency level, what the reference moves through its
 * master / slave pipes per BatchNorm call (modeling/sync_batchnorm/batchnorm.py:95-108, comm.py:56-129) and what rounds 2-4 sent through a
 * stock RCCL all_reduce.  Every rank owns a mailbox in its own HBM (fine-grained allocation, exported as a hipIpc handle, mapped by every
 * peer); an exchange is ONE single-workgroup launch: push the vector into every mailbox, flag it, poll the own mailbox (bounded: a missing
 * flag sets an error word and the kernel returns), add the ranks' vectors in rank order (bit-identical on every rank).  Capturable in a
 * hipGraph (the sequence number lives in device memory).  Every rank issues the same sequence of addk_comm_allreduce calls.
 *   host flow: addk_comm_alloc -> exchange the 64-byte handles (any out-of-band channel, e.g. the process group) -> addk_comm_open
 *              -> addk_comm_allreduce ... -> addk_comm_status (error word) -> addk_comm_close.
 * Error behaviour: negative status + addk_last_error() for invalid arguments / HIP failures; a timed-out exchange is reported by
 * addk_comm_status (err != 0: bit 63 | sequence number << 8 | rank whose flag never arrived), never by a hang. */
int64_t addk_comm_mailbox_bytes(int32_t world, int64_t max_bytes);
int addk_comm_alloc(int32_t world, int64_t max_bytes, void** mailbox, void* handle64);
int addk_comm_open(int32_t rank, int32_t world, int64_t max_bytes, void* my_mailbox, const void* handles, void** comm_out);
int addk_comm_allreduce(void* comm, void* buf, int64_t count, int32_t dtype /* 0 fp32, 1 fp64 */, void* stream);
int addk_comm_status(void* comm, int64_t* seq, int64_t* err);
int addk_comm_close(void* comm, void* my_mailbox);

/* diagnostic: print the NATIVE stack on SIGABRT / SIGSEGV (stderr), then die as before.  tests/conftest.py and bench.py's child processes call it. */
int addk_debug_trace_fatal_signals(void);

#ifdef __cplusplus
}
#endif
#endif
