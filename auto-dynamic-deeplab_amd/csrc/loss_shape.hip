// The training head with a per-pixel loss shape: focal loss and label-smoothed cross-entropy (addk_ce_upsample_shaped_fwd_bwd).  The
// kernel is ce_up_kernel of ce_up.h with SHAPE = CE_FOCAL / CE_SMOOTH, alone, with a kept set (OHEM), with the soft-Dice term (DICE) and
// with both: eight instantiations per class count, in a unit of their own beside loss_up.hip's twelve.  There is no distillation form.
#include "ce_up.h"

namespace {

// second stage of a shaped head: the partials in the order of sum_partials_kernel, accumulated into the loss word; n == 0 (no valid
// pixel) adds exactly 0 where the plain head's sum leaves 0/0
__global__ void __launch_bounds__(256) shape_sum_kernel(const float* ws, int n, float scale, const float* denom, float* out) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += ws[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float d = *denom;
    *out += d > 0.f ? s * scale / d : 0.f;
  }
}

template <int CC, int SHAPE>
void shape_launch(bool ohem, bool dice, dim3 grid, hipStream_t st, const CeUpShapeK& k) {
  if (ohem && dice) hipLaunchKernelGGL((ce_up_kernel<CC, true, false, false, true, SHAPE>), grid, dim3(256), 0, st, k);
  else if (dice) hipLaunchKernelGGL((ce_up_kernel<CC, false, false, false, true, SHAPE>), grid, dim3(256), 0, st, k);
  else if (ohem) hipLaunchKernelGGL((ce_up_kernel<CC, true, false, false, false, SHAPE>), grid, dim3(256), 0, st, k);
  else hipLaunchKernelGGL((ce_up_kernel<CC, false, false, false, false, SHAPE>), grid, dim3(256), 0, st, k);
}

}  // namespace

extern "C" int addk_ce_upsample_shaped_supported(int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t C) {
  return ceu_ok(N, H, W, OH, OW, C) ? 1 : 0;
}

extern "C" int addk_ce_upsample_shaped_fwd_bwd(const addk_ce_upsample_shaped_args* s, void* stream) {
  ADDK_REQUIRE(s, "ce_upsample_shaped: null pointer");
  const addk_ce_upsample_dice_args* d = &s->dice;
  const addk_ce_upsample_kd_args* b = &d->kd;
  const addk_ce_upsample_args* a = &b->ce;
  ADDK_REQUIRE(s->shape == ADDK_CE_SHAPE_NONE || s->shape == ADDK_CE_SHAPE_FOCAL || s->shape == ADDK_CE_SHAPE_SMOOTH,
               "ce_upsample_shaped: shape must be ADDK_CE_SHAPE_NONE, _FOCAL or _SMOOTH");
  if (s->shape == ADDK_CE_SHAPE_NONE) {                           // the other entry points, with their own checks and their bits
    if (d->coef) return addk_ce_upsample_dice_fwd_bwd(d, stream);
    if (b->teacher) return addk_ce_upsample_kd_fwd_bwd(b, stream);
    if (b->pix_loss || b->tau) {
      const addk_ce_upsample_ohem_args o{*a, b->pix_loss, b->tau};
      return addk_ce_upsample_ohem_fwd_bwd(&o, stream);
    }
    return addk_ce_upsample_fwd_bwd(a, stream);
  }
  ADDK_REQUIRE(a->logits && a->target && a->wsum && a->loss_out && a->g && a->ws, "ce_upsample_shaped: null pointer");
  ADDK_REQUIRE((b->pix_loss == nullptr) == (b->tau == nullptr), "ce_upsample_shaped: pix_loss and tau come together (both NULL: no mining)");
  ADDK_REQUIRE(!b->teacher, "ce_upsample_shaped: the focal and label-smoothed heads have no distillation form (teacher must be NULL)");
  if (s->shape == ADDK_CE_SHAPE_FOCAL)
    ADDK_REQUIRE(isfinite(s->gamma) && s->gamma >= 1.f, "ce_upsample_shaped: gamma must be finite and at least 1");
  else
    ADDK_REQUIRE(s->eps > 0.f && s->eps < 1.f, "ce_upsample_shaped: eps must lie in (0, 1)");
  ADDK_REQUIRE(a->ld >= a->C && a->ldg >= a->C, "ce_upsample_shaped: short stride");
  ADDK_REQUIRE(ceu_ok(a->N, a->H, a->W, a->OH, a->OW, a->C), "ce_upsample_shaped: unsupported shape (%s, at most %d output rows per input row)",
               head_classes_text().c_str(), CEU_MAXBAND);
  CeUpShapeK k{};
  const dim3 grid = ceu_fill(k, a, b->pix_loss, b->tau);
  k.coef = d->coef; k.gamma = s->gamma; k.eps = s->eps;
  const int nblk = (int)(grid.x * grid.y * grid.z);
  hipStream_t st = (hipStream_t)stream;
  head_classes(a->C, [&](auto cc) {                               // ceu_ok: a->C is of the list
    constexpr int CC = decltype(cc)::value;
    if (s->shape == ADDK_CE_SHAPE_FOCAL) shape_launch<CC, CE_FOCAL>(b->pix_loss != nullptr, d->coef != nullptr, grid, st, k);
    else shape_launch<CC, CE_SMOOTH>(b->pix_loss != nullptr, d->coef != nullptr, grid, st, k);
  });
  int rc = addk_check_launch("ce_upsample_shaped");
  if (rc) return rc;
  hipLaunchKernelGGL(shape_sum_kernel, dim3(1), dim3(256), 0, st, a->ws, nblk, a->scale, a->wsum, a->loss_out);
  return addk_check_launch("ce_upsample_shaped_sum");
}
