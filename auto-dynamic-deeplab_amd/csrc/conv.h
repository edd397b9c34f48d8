// The kernel choice of one forward / data-gradient convolution launch (addk_conv_fwd, addk_conv_dgrad).  conv_choose_* makes the
// ordered decision once; the launch, the weight-pack size and descriptor, the batch key and prepare, addk_conv_fwd_resample_ok
// and addk_conv_*_config all read it.  The coverage rules and launchers of the specialised kernels live next to them (pw.hip,
// conv3.hip); conv.hip orders them and owns the generic kernel.
#pragma once
#include "common.h"

// The numbers are what addk_conv_fwd_config / addk_conv_dgrad_config return in cfg[0] (include/addk.h documents cfg).
enum ConvKind : int {
  CK_GENERIC = 0,     // implicit-GEMM kernel (conv.hip conv_kernel)
  CK_PARITY = 1,      // the same kernel over the input-pixel parity classes of a stride-2 data gradient
  CK_STEM0 = 2,       // 3-channel 3x3 stride-2 stem (pw.hip stem0_kernel)
  CK_PW = 3,          // register-stationary 1x1 (pw.hip pw_kernel): the only kind a conv batch merges
  CK_PWK = 4,         // streaming-K 1x1 forward (pw.hip pwk_kernel)
  CK_K1S = 5,         // 1x1 data gradient with few output channels (pw.hip k1s_dgrad_kernel)
  CK_HALO = 6,        // fp32 halo-patch kernel (conv3.hip conv3_kernel)
  CK_SPLIT = 7,       // split-precision halo-patch kernel (conv3b.h conv3b_kernel): one- or two-row tiles, stride-2 forward
  CK_SPLIT_S2D = 8,   // split-precision stride-2 data gradient, four parity classes per workgroup (conv3b_s2.hip conv3s_kernel)
  CK_C3N = 9,         // split-precision 5x5 on 16-wide channel tiles (conv3n.hip conv3n_kernel)
};
inline bool conv_kind_halo(int kind) { return kind >= CK_HALO; }

// The kernel of a halo-kind launch.  Every unit that instantiates such kernels exposes them through plain lookup functions (conv3b.h: c3_variant_fp32,
// c3b_variant_*, c3n_variant), so no kernel symbol crosses files; fn == nullptr: no such instantiation.  A lookup only takes addresses, it does not
// touch the HIP runtime: raise_lds (null for a kernel with static LDS) lifts the kernel's dynamic-LDS limit and is called where the launch is.
struct C3K;
typedef void (*C3Fn)(const C3K);
struct C3Variant { C3Fn fn; unsigned threads; void (*raise_lds)(); };

struct ConvChoice {
  int kind;
  // template parameters, as cfg[1..4] reports them:
  //   GENERIC / PARITY: PT, CT, red32, classes | STEM0: CT, red32 | PW: CT, KG, RS, red32 | PWK: CT, RS, red32 | K1S: KMAX
  //   HALO: BCT, KS | SPLIT: WC, KS, pixels per tile row, rows per tile | SPLIT_S2D: planes | C3N: KS, planes
  int v[4];
  int gx, gy, launches;   // grid of the (first) launch; launches (PARITY: one per class when the slab has fewer than 16 rows)
  int rows;               // statistics-slab rows (addk_conv_rows)
  size_t lds;             // dynamic LDS bytes
  int key;                // PW: the batch key; -1 otherwise
  // PARITY: the classes in workgroup order (one launch: each owns [gx0, gx0 + gx) of the grid) or launch order
  struct Cls { long P; int ph, pw, MH, MW, ntaps, kill, gx, gx0, slab_row, pt, ct; int taplist[9]; } cls[4];
  int ncls;
  long P;                 // GENERIC / PARITY (one launch): pixels of the M side (the largest class)
  // halo kinds: tile walk and weight pack
  int HT, spr, ntiles, nT; long wp_blk;
  int planes, bct, dil_odd, s2d, nchunks, pack_blocks;
  int64_t pack_floats;
  C3Variant var;          // the kernel that kind and v[] name: a halo kind is only chosen when it exists
};

int conv_choose_fwd(const addk_conv_args* a, int mode, int mask, ConvChoice& c);
int conv_choose_dgrad(const addk_conv_dgrad_args* a, int mode, int mask, ConvChoice& c);
// pw.hip: STEM0, PW, PWK forward / PW, K1S data gradient; conv3.hip: the halo kinds (false: not covered, including a missing,
// short or misaligned wpack and a form that no unit instantiates)
bool pw_choose_fwd(const addk_conv_args* a, ConvChoice& c);
bool pw_choose_dgrad(const addk_conv_dgrad_args* a, ConvChoice& c);
bool c3_choose_fwd(const addk_conv_args* a, int mode, int mask, ConvChoice& c);
bool c3_choose_dgrad(const addk_conv_dgrad_args* a, int mode, int mask, ConvChoice& c);
int pw_run_fwd(const ConvChoice& c, const addk_conv_args* a, hipStream_t st);
int pw_run_dgrad(const ConvChoice& c, const addk_conv_dgrad_args* a, hipStream_t st);
int c3_run_fwd(const ConvChoice& c, const addk_conv_args* a, hipStream_t st);
int c3_run_dgrad(const ConvChoice& c, const addk_conv_dgrad_args* a, hipStream_t st);
