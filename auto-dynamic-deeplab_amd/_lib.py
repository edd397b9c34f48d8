"""ctypes binding of libaddk.so (the C ABI declared in include/addk.h).

The product path has no CPU fallback: if the shared library is missing or a
symbol is absent, importing/using `addk` raises immediately.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ADDK_LIB') or os.path.join(_HERE, 'libaddk.so')      # ADDK_LIB: an A/B or diagnostic build of the same sources (scripts/*.sh)

MAX_SRC, MAX_SLAB, MAX_TERMS = 12, 32, 4
MAX_VIEWS = 8
MAX_TILES_AXIS = 16
fp = C.POINTER(C.c_float)
i32, i64, f32, f64, vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p


class Src(C.Structure):
    _fields_ = [('x', vp), ('a', vp), ('b', vp), ('ld', i32), ('C', i32), ('relu', i32), ('rs_hw', i32)]


class ConvArgs(C.Structure):
    _fields_ = [('src', Src * MAX_SRC), ('nsrc', i32), ('N', i32), ('H', i32), ('W', i32), ('OH', i32), ('OW', i32),
                ('KH', i32), ('KW', i32), ('stride', i32), ('pad', i32), ('dil', i32), ('Cout', i32), ('ldw', i32),
                ('cin_total', i32), ('w_choff', i32), ('ldy', i32), ('w', vp), ('y', vp), ('bias', vp), ('bias_n', vp),
                ('stats', vp), ('stats_ld', i32), ('_pad', i32), ('wpack', vp), ('wpack_floats', i64), ('wpack_ready', i32), ('_pad2', i32),
                ('rs_y', vp), ('rs_ldy', i32), ('_pad3', i32)]


class ConvDgradArgs(C.Structure):
    _fields_ = [('dy', vp), ('lddy', i32), ('Cout', i32), ('N', i32), ('H', i32), ('W', i32), ('OH', i32), ('OW', i32),
                ('KH', i32), ('KW', i32), ('stride', i32), ('pad', i32), ('dil', i32), ('w', vp), ('ldw', i32),
                ('cin_total', i32), ('w_choff', i32), ('dst', Src), ('g', vp), ('ldg', i32), ('accumulate', i32),
                ('dab', vp), ('wpack', vp), ('wpack_floats', i64), ('wpack_ready', i32), ('_pad2', i32)]


class ConvWgradArgs(C.Structure):
    _fields_ = [('dy', vp), ('lddy', i32), ('Cout', i32), ('N', i32), ('H', i32), ('W', i32), ('OH', i32), ('OW', i32),
                ('KH', i32), ('KW', i32), ('stride', i32), ('pad', i32), ('dil', i32), ('src', Src), ('dw', vp),
                ('ldw', i32), ('cin_total', i32), ('w_choff', i32), ('accumulate', i32), ('ws', vp), ('ws_floats', i64)]


class BnFinalizeArgs(C.Structure):
    _fields_ = [('partial', vp), ('rows', i32), ('C', i32), ('count', f64), ('gamma', vp), ('beta', vp),
                ('running_mean', vp), ('running_var', vp), ('momentum', f32), ('eps', f32), ('a', vp), ('b', vp),
                ('mean', vp), ('invstd', vp)]


class SepArgs(C.Structure):
    _fields_ = [('src', Src), ('N', i32), ('H', i32), ('W', i32), ('K', i32), ('Cout', i32), ('ldw', i32), ('dw_w', vp), ('pw_w', vp),
                ('y', vp), ('ldy', i32), ('ldt', i32), ('t', vp), ('stats', vp), ('stats_ld', i32), ('stats_rows', i32), ('nterm', i32), ('ea', vp), ('eb', vp),
                ('term', Src * MAX_TERMS), ('fin', BnFinalizeArgs), ('fin_counter', vp)]


class SepBwdArgs(C.Structure):
    _fields_ = [('dy', vp), ('lddy', i32), ('N', i32), ('H', i32), ('W', i32), ('K', i32), ('src', Src), ('Cout', i32), ('ldw', i32),
                ('dw_w', vp), ('pw_w', vp), ('g', vp), ('ldg', i32), ('accumulate', i32), ('dab', vp), ('ws', vp)]


class CeUpsampleArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('target', vp), ('class_w', vp), ('ignore_index', i32), ('wsum', vp), ('scale', f32), ('loss_out', vp),
                ('g', vp), ('ldg', i32), ('accumulate', i32), ('ws', vp)]


class OhemSelectArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('target', vp), ('class_w', vp), ('ignore_index', i32), ('thresh', f32), ('min_kept_total', i64), ('pix_loss', vp),
                ('tau', vp), ('wsum_kept', vp), ('counts', vp), ('ws', vp)]


class CeUpsampleOhemArgs(C.Structure):
    _fields_ = [('ce', CeUpsampleArgs), ('pix_loss', vp), ('tau', vp)]


class CeUpsampleKdArgs(C.Structure):
    _fields_ = [('ce', CeUpsampleArgs), ('pix_loss', vp), ('tau', vp), ('teacher', vp), ('ld_teacher', i32), ('alpha', f32),
                ('temperature', f32), ('nvalid', vp), ('kd_out', vp)]


class DiceStatsArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('target', vp), ('ignore_index', i32), ('weight', f32), ('smooth', f32), ('scale', f32), ('coef', vp), ('dice_out', vp),
                ('loss_out', vp), ('ws', vp)]


class CeUpsampleDiceArgs(C.Structure):
    _fields_ = [('kd', CeUpsampleKdArgs), ('coef', vp)]


CE_SHAPE_NONE, CE_SHAPE_FOCAL, CE_SHAPE_SMOOTH = 0, 1, 2


class CeUpsampleShapedArgs(C.Structure):
    _fields_ = [('dice', CeUpsampleDiceArgs), ('shape', i32), ('gamma', f32), ('eps', f32)]


class ScoreUpsampleArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('target', vp), ('class_w', vp), ('ignore_index', i32), ('wsum', vp), ('scale', f32), ('loss_out', vp),
                ('ent_out', vp), ('cm', vp), ('pred_out', vp), ('ws', vp)]


class GateUpsampleArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('max_thr', vp), ('out', vp), ('out_host', vp), ('ws', vp)]


class LabelUpsampleArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('lut256', vp), ('labels', vp)]


class GateLabelUpsampleArgs(C.Structure):
    _fields_ = [('gate', GateUpsampleArgs), ('lut256', vp), ('labels', vp)]


class View(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('n0', i32), ('H', i32), ('W', i32), ('mirror', i32), ('weight', f32)]


class LabelViewsArgs(C.Structure):
    _fields_ = [('view', View * MAX_VIEWS), ('nview', i32), ('N', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('lut256', vp), ('labels', vp)]


class TileDesc(C.Structure):
    _fields_ = [('image', vp), ('H', i32), ('W', i32), ('y0', i32), ('x0', i32)]


class LabelTilesArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('h', i32), ('w', i32), ('th', i32), ('tw', i32), ('N', i32), ('C', i32), ('OH', i32),
                ('OW', i32), ('t0', i32), ('ny', i32), ('nx', i32), ('y0', i32 * MAX_TILES_AXIS), ('x0', i32 * MAX_TILES_AXIS),
                ('lut256', vp), ('labels', vp)]


class TileViewDesc(C.Structure):
    _fields_ = [('image', vp), ('H', i32), ('W', i32), ('Hv', i32), ('Wv', i32), ('y0', i32), ('x0', i32), ('mirror', i32)]


class TileView(C.Structure):
    _fields_ = [('Hv', i32), ('Wv', i32), ('t0', i32), ('ny', i32), ('nx', i32), ('mirror', i32), ('weight', f32),
                ('y0', i32 * MAX_TILES_AXIS), ('x0', i32 * MAX_TILES_AXIS)]


class LabelTileViewsArgs(C.Structure):
    _fields_ = [('view', TileView * MAX_VIEWS), ('nview', i32), ('logits', vp), ('ld', i32), ('h', i32), ('w', i32), ('th', i32), ('tw', i32),
                ('N', i32), ('C', i32), ('OH', i32), ('OW', i32), ('lut256', vp), ('labels', vp)]


class GateTilesArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('B', i32), ('nb', i32), ('h', i32), ('w', i32), ('C', i32), ('th', i32), ('tw', i32),
                ('ext', vp), ('max_thr', vp), ('inv_temp', vp), ('out', vp), ('out_host', vp), ('ws', vp)]


class ScatterTileLogitsArgs(C.Structure):
    _fields_ = [('src', vp), ('lds', i32), ('B', i32), ('store', vp), ('ld', i32), ('T', i32), ('h', i32), ('w', i32), ('C', i32),
                ('src_row', vp), ('dst_tile', vp), ('n', i32)]


class ProfileUpsampleArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('target', vp), ('thr', vp), ('nthr', i32), ('ent_out', vp), ('share_out', vp), ('cm', vp), ('pred_out', vp), ('ws', vp)]


class GateUpsampleTArgs(C.Structure):
    _fields_ = [('gate', GateUpsampleArgs), ('inv_temp', vp), ('lut256', vp), ('labels', vp)]


class ProfileUpsampleTArgs(C.Structure):
    _fields_ = [('profile', ProfileUpsampleArgs), ('inv_temp', vp)]


CALIB_MAX_T, CALIB_BINS = 8, 16


class CalibUpsampleArgs(C.Structure):
    _fields_ = [('logits', vp), ('ld', i32), ('N', i32), ('H', i32), ('W', i32), ('C', i32), ('OH', i32), ('OW', i32),
                ('target', vp), ('inv_temp', vp), ('nt', i32), ('bins', vp), ('nll', vp), ('ws', vp)]


TRIMAP_MAX_RADIUS, TRIMAP_MAX_WIDTHS, TRIMAP_FAR = 64, 8, 255


class BoundaryDistArgs(C.Structure):
    _fields_ = [('target', vp), ('N', i32), ('OH', i32), ('OW', i32), ('C', i32), ('radius', i32), ('dist', vp), ('ws', vp)]


class ConfusionBandedArgs(C.Structure):
    _fields_ = [('target', vp), ('pred', vp), ('dist', vp), ('N', i32), ('OH', i32), ('OW', i32), ('C', i32), ('nw', i32),
                ('width', i32 * TRIMAP_MAX_WIDTHS), ('cm', vp), ('image_stride', i64)]


class RowsItem(C.Structure):
    _fields_ = [('src', vp), ('dst', vp), ('row_bytes', i64)]


class GatherRowsArgs(C.Structure):
    _fields_ = [('items', vp), ('nitems', i32), ('src_row', vp), ('dst_row', vp), ('nrows', i32)]


class DwArgs(C.Structure):
    _fields_ = [('src', Src), ('N', i32), ('H', i32), ('W', i32), ('OH', i32), ('OW', i32), ('KH', i32), ('KW', i32),
                ('stride', i32), ('pad', i32), ('dil', i32), ('w', vp), ('y', vp), ('ldy', i32)]


class DwBwdArgs(C.Structure):
    _fields_ = [('dy', vp), ('lddy', i32), ('N', i32), ('H', i32), ('W', i32), ('OH', i32), ('OW', i32), ('KH', i32),
                ('KW', i32), ('stride', i32), ('pad', i32), ('dil', i32), ('src', Src), ('w', vp), ('g', vp), ('ldg', i32),
                ('accumulate', i32), ('dab', vp), ('dw', vp), ('dw_accumulate', i32), ('ws', vp), ('defer_wreduce', i32), ('_pad', i32)]


class DwWreduceItem(C.Structure):
    _fields_ = [('ws', vp), ('dw', vp), ('rows', i32), ('n', i32), ('accumulate', i32), ('_pad', i32)]


class BnEvalItem(C.Structure):
    _fields_ = [('gamma', vp), ('beta', vp), ('running_mean', vp), ('running_var', vp), ('a', vp), ('b', vp), ('C', i32), ('eps', f32)]


class BnBwdArgs(C.Structure):
    _fields_ = [('slab', vp * MAX_SLAB), ('rows', i32 * MAX_SLAB), ('nslab', i32), ('C', i32), ('count', f64),
                ('gamma', vp), ('mean', vp), ('invstd', vp), ('a', vp), ('dgamma', vp), ('dbeta', vp),
                ('accumulate', i32), ('c1', vp), ('c2', vp), ('dmv', vp), ('centered', i32), ('_pad', i32)]


class SlabReduceItem(C.Structure):
    _fields_ = [('partial', vp), ('out', vp), ('rows', i32), ('C', i32)]


class BnCoeffsItem(C.Structure):
    _fields_ = [('dmv', vp), ('c1', vp), ('c2', vp), ('count', f64), ('C', i32), ('_pad', i32)]


class BnApplyItem(C.Structure):
    _fields_ = [('g', vp), ('x', vp), ('c1', vp), ('c2', vp), ('mean', vp), ('out', vp), ('P', i64), ('ldg', i32), ('ldx', i32), ('ldo', i32),
                ('C', i32)]


class AffineSumArgs(C.Structure):
    _fields_ = [('term', Src * MAX_TERMS), ('nterm', i32), ('P', i64), ('C', i32), ('out', vp), ('ldo', i32),
                ('relu_out', i32), ('accumulate', i32)]


class AffineSumBwdArgs(C.Structure):
    _fields_ = [('term', Src * MAX_TERMS), ('nterm', i32), ('P', i64), ('C', i32), ('dout', vp), ('lddo', i32),
                ('out', vp), ('ldo', i32), ('relu_out', i32), ('g', vp * MAX_TERMS), ('ldg', i32 * MAX_TERMS),
                ('accumulate', i32 * MAX_TERMS), ('dab', vp * MAX_TERMS)]


class EdmArgs(C.Structure):
    _fields_ = [('src', Src), ('N', i32), ('H', i32), ('W', i32), ('ldo', i32), ('conv_w', vp), ('w1', vp), ('b1', vp), ('w2', vp), ('b2', vp),
                ('w3', vp), ('b3', vp), ('out', vp), ('out_host', vp), ('ws', vp)]


class ResizeArgs(C.Structure):
    _fields_ = [('src', Src), ('N', i32), ('H', i32), ('W', i32), ('OH', i32), ('OW', i32), ('y', vp), ('ldy', i32),
                ('nchw_out', i32)]


class ResizeBwdArgs(C.Structure):
    _fields_ = [('dy', vp), ('lddy', i32), ('nchw_in', i32), ('dy_scale', vp), ('src', Src), ('N', i32), ('H', i32),
                ('W', i32), ('OH', i32), ('OW', i32), ('g', vp), ('ldg', i32), ('accumulate', i32), ('dab', vp)]


# header type name (include/addk.h) -> its mirror above; tests/test_abi.py compares sizes and offsets, and that no mirror is missing here
STRUCTS = {
    'addk_src': Src, 'addk_conv_args': ConvArgs, 'addk_conv_dgrad_args': ConvDgradArgs, 'addk_conv_wgrad_args': ConvWgradArgs,
    'addk_bn_finalize_args': BnFinalizeArgs, 'addk_sep_args': SepArgs, 'addk_sep_bwd_args': SepBwdArgs,
    'addk_ce_upsample_args': CeUpsampleArgs, 'addk_ohem_select_args': OhemSelectArgs, 'addk_ce_upsample_ohem_args': CeUpsampleOhemArgs,
    'addk_ce_upsample_kd_args': CeUpsampleKdArgs, 'addk_dice_stats_args': DiceStatsArgs, 'addk_ce_upsample_dice_args': CeUpsampleDiceArgs,
    'addk_ce_upsample_shaped_args': CeUpsampleShapedArgs,
    'addk_score_upsample_args': ScoreUpsampleArgs, 'addk_gate_upsample_args': GateUpsampleArgs, 'addk_label_upsample_args': LabelUpsampleArgs,
    'addk_gate_label_upsample_args': GateLabelUpsampleArgs, 'addk_view': View, 'addk_label_views_args': LabelViewsArgs,
    'addk_tile_desc': TileDesc, 'addk_label_tiles_args': LabelTilesArgs,
    'addk_tile_view_desc': TileViewDesc, 'addk_tile_view': TileView, 'addk_label_tile_views_args': LabelTileViewsArgs,
    'addk_gate_tiles_args': GateTilesArgs, 'addk_scatter_tile_logits_args': ScatterTileLogitsArgs,
    'addk_profile_upsample_args': ProfileUpsampleArgs, 'addk_gate_upsample_t_args': GateUpsampleTArgs,
    'addk_profile_upsample_t_args': ProfileUpsampleTArgs, 'addk_calib_upsample_args': CalibUpsampleArgs,
    'addk_boundary_dist_args': BoundaryDistArgs, 'addk_confusion_banded_args': ConfusionBandedArgs, 'addk_rows_item': RowsItem,
    'addk_gather_rows_args': GatherRowsArgs, 'addk_dw_args': DwArgs, 'addk_dw_bwd_args': DwBwdArgs, 'addk_dw_wreduce_item': DwWreduceItem,
    'addk_bn_eval_item': BnEvalItem, 'addk_bn_bwd_args': BnBwdArgs, 'addk_slab_reduce_item': SlabReduceItem,
    'addk_bn_coeffs_item': BnCoeffsItem, 'addk_bn_apply_item': BnApplyItem, 'addk_affine_sum_args': AffineSumArgs,
    'addk_affine_sum_bwd_args': AffineSumBwdArgs, 'addk_edm_args': EdmArgs, 'addk_resize_args': ResizeArgs,
    'addk_resize_bwd_args': ResizeBwdArgs,
}

_SIGS = {
    'addk_last_error': (C.c_char_p, []),
    'addk_version': (i32, []),
    'addk_selftest_mfma': (i32, [vp, vp]),
    'addk_conv_fwd': (i32, [C.POINTER(ConvArgs), vp]),
    'addk_conv_rows': (i32, [i64, i32]),
    'addk_set_conv_precision': (i32, [i32]),
    'addk_set_split_min_channels': (i32, [i32]),
    'addk_get_conv_precision': (i32, []),
    'addk_conv_dgrad': (i32, [C.POINTER(ConvDgradArgs), vp]),
    'addk_set_fast_paths': (i32, [i32]),
    'addk_get_fast_paths': (i32, []),
    'addk_conv_fwd_pack_floats': (i64, [C.POINTER(ConvArgs)]),
    'addk_conv_dgrad_pack_floats': (i64, [C.POINTER(ConvDgradArgs)]),
    'addk_conv_fwd_batch_key': (i32, [C.POINTER(ConvArgs)]),
    'addk_conv_dgrad_batch_key': (i32, [C.POINTER(ConvDgradArgs)]),
    'addk_conv_fwd_batch_prepare': (i64, [vp, i32, vp, i64, vp]),
    'addk_conv_dgrad_batch_prepare': (i64, [vp, i32, vp, i64, vp]),
    'addk_conv_batch_run': (i32, [vp, vp, vp]),
    'addk_conv_pack_desc_bytes': (i64, []),
    'addk_conv_fwd_pack_desc': (i32, [C.POINTER(ConvArgs), vp]),
    'addk_conv_dgrad_pack_desc': (i32, [C.POINTER(ConvDgradArgs), vp]),
    'addk_conv_pack_batch': (i32, [vp, i32, vp]),
    'addk_conv_fwd_resample_ok': (i32, [C.POINTER(ConvArgs)]),
    'addk_conv_fwd_config': (i32, [C.POINTER(ConvArgs), C.POINTER(i32)]),
    'addk_conv_dgrad_config': (i32, [C.POINTER(ConvDgradArgs), C.POINTER(i32)]),
    'addk_debug_trace_fatal_signals': (i32, []),
    'addk_comm_mailbox_bytes': (i64, [i32, i64]),
    'addk_comm_alloc': (i32, [i32, i64, C.POINTER(vp), vp]),
    'addk_comm_open': (i32, [i32, i32, i64, vp, vp, C.POINTER(vp)]),
    'addk_comm_allreduce': (i32, [vp, vp, i64, i32, vp]),
    'addk_comm_status': (i32, [vp, C.POINTER(i64), C.POINTER(i64)]),
    'addk_comm_close': (i32, [vp, vp]),
    'addk_edm_head_ws_bytes': (i64, [i32, i32, i32]),
    'addk_edm_head_supported': (i32, [C.POINTER(EdmArgs)]),
    'addk_edm_head': (i32, [C.POINTER(EdmArgs), vp]),
    'addk_conv_wgrad': (i32, [C.POINTER(ConvWgradArgs), vp]),
    'addk_conv_wgrad_ws': (i64, [i64, i32, i32, i32]),
    'addk_conv_wgrad_config': (i32, [C.POINTER(ConvWgradArgs), C.POINTER(i32)]),
    'addk_conv_wgrad_batch_prepare': (i64, [C.POINTER(ConvWgradArgs), i32, vp, i64, C.POINTER(i64)]),
    'addk_conv_wgrad_batch_run': (i32, [vp, C.POINTER(i64), vp]),
    'addk_lut_u8': (i32, [vp, vp, i64, vp, vp]),
    'addk_resample_u8': (i32, [vp, i32, i32, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp]),
    'addk_nearest_u8': (i32, [vp, i32, i32, vp, i32, i32, vp, vp, i32, vp]),
    'addk_finish_sample': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    'addk_sep_fwd_supported': (i32, [C.POINTER(SepArgs)]),
    'addk_sep_rows': (i32, [C.POINTER(SepArgs)]),
    'addk_sep_fwd_config': (i32, [C.POINTER(SepArgs), C.POINTER(i32)]),
    'addk_sep_bwd_config': (i32, [C.POINTER(SepBwdArgs), C.POINTER(i32)]),
    'addk_bn_fin_ws_bytes': (i64, [i32, i32]),
    'addk_sep_bwd_rows': (i32, [C.POINTER(SepBwdArgs)]),
    'addk_sep_bwd': (i32, [C.POINTER(SepBwdArgs), vp]),
    'addk_sep_bwd_batch_key': (i32, [C.POINTER(SepBwdArgs)]),
    'addk_sep_bwd_batch_prepare': (i64, [vp, i32, vp, i64, vp]),
    'addk_sep_bwd_batch_run': (i32, [vp, vp, vp]),
    'addk_sep_fwd': (i32, [C.POINTER(SepArgs), vp]),
    'addk_sep_fwd_batch_key': (i32, [C.POINTER(SepArgs)]),
    'addk_sep_fwd_batch_prepare': (i64, [vp, i32, vp, i64, vp]),
    'addk_sep_batch_run': (i32, [vp, vp, vp]),
    'addk_dw_fwd': (i32, [C.POINTER(DwArgs), vp]),
    'addk_dw_bwd': (i32, [C.POINTER(DwBwdArgs), vp]),
    'addk_dw_rows': (i32, [i64, i32]),
    'addk_dw_fwd_config': (i32, [C.POINTER(DwArgs), C.POINTER(i32)]),
    'addk_dw_bwd_config': (i32, [C.POINTER(DwBwdArgs), C.POINTER(i32)]),
    'addk_dw_wreduce_batch': (i32, [vp, i32, vp]),
    'addk_dw_fwd_batch_key': (i32, [C.POINTER(DwArgs)]),
    'addk_dw_bwd_batch_key': (i32, [C.POINTER(DwBwdArgs)]),
    'addk_dw_fwd_batch_prepare': (i64, [vp, i32, vp, i64, vp]),
    'addk_dw_bwd_batch_prepare': (i64, [vp, i32, vp, i64, vp]),
    'addk_dw_batch_run': (i32, [vp, vp, vp]),
    'addk_bn_finalize_batch': (i32, [vp, i32, i32, vp]),
    'addk_slab_reduce_batch': (i32, [vp, i32, i32, vp]),
    'addk_bn_bwd_coeffs_batch': (i32, [vp, i32, i32, vp]),
    'addk_bn_bwd_batch': (i32, [vp, i32, i32, vp]),
    'addk_bn_bwd_apply_batch': (i32, [vp, i32, i64, vp]),
    'addk_bn_finalize': (i32, [C.POINTER(BnFinalizeArgs), vp]),
    'addk_slab_reduce': (i32, [C.POINTER(SlabReduceItem), vp]),
    'addk_bn_eval_affine': (i32, [C.POINTER(BnEvalItem), vp]),
    'addk_bn_eval_affine_batch': (i32, [vp, i32, vp]),
    'addk_bn_bwd': (i32, [C.POINTER(BnBwdArgs), vp]),
    'addk_bn_bwd_coeffs': (i32, [C.POINTER(BnCoeffsItem), vp]),
    'addk_affine_sum_fwd': (i32, [C.POINTER(AffineSumArgs), vp]),
    'addk_affine_sum_bwd': (i32, [C.POINTER(AffineSumBwdArgs), vp]),
    'addk_ew_rows': (i32, [i64, i32]),
    'addk_bn_bwd_apply': (i32, [C.POINTER(BnApplyItem), vp]),
    'addk_resize_fwd': (i32, [C.POINTER(ResizeArgs), vp]),
    'addk_resize_bwd': (i32, [C.POINTER(ResizeBwdArgs), vp]),
    'addk_resize_bwd_config': (i32, [C.POINTER(ResizeBwdArgs), C.POINTER(i32)]),
    'addk_resize_bwd_batch_key': (i32, [C.POINTER(ResizeBwdArgs)]),
    'addk_resize_bwd_batch_prepare': (i64, [vp, i32, vp, i64, vp]),
    'addk_resize_bwd_batch_run': (i32, [vp, vp, vp]),
    'addk_gap_fwd': (i32, [C.POINTER(Src), i32, i32, vp, i32, vp, i32, vp]),
    'addk_gap_bwd': (i32, [C.POINTER(Src), i32, i32, vp, i32, vp, i32, i32, vp, vp]),
    'addk_pool3_fwd': (i32, [C.POINTER(Src), i32, i32, i32, i32, i32, i32, i32, vp, i32, vp]),
    'addk_pool3_bwd': (i32, [C.POINTER(Src), i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, i32, i32, vp]),
    'addk_nchw_to_nhwc': (i32, [vp, i32, i32, i64, vp, i32, vp]),
    'addk_nhwc_to_nchw': (i32, [C.POINTER(Src), i32, i64, vp, vp]),
    'addk_nchw_grad_to_nhwc': (i32, [vp, C.POINTER(Src), i32, i64, vp, i32, i32, vp, vp]),
    'addk_ce_count': (i32, [vp, i64, vp, i32, i32, vp, vp, vp]),
    'addk_ce_fwd_bwd': (i32, [vp, vp, i32, i32, i64, vp, i32, vp, f32, vp, vp, vp, vp]),
    'addk_ce_ws_floats': (i64, [i32, i64]),
    'addk_head_classes': (i32, [C.POINTER(i32), i32]),
    'addk_gate_head_classes': (i32, [C.POINTER(i32), i32]),
    'addk_ce_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_ce_upsample_ws_floats': (i64, [i32, i32, i32]),
    'addk_ce_upsample_fwd_bwd': (i32, [C.POINTER(CeUpsampleArgs), vp]),
    'addk_ohem_select_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_ohem_select_ws_bytes': (i64, [i32, i32, i32]),
    'addk_ohem_select': (i32, [C.POINTER(OhemSelectArgs), vp]),
    'addk_ce_upsample_ohem_fwd_bwd': (i32, [C.POINTER(CeUpsampleOhemArgs), vp]),
    'addk_ce_upsample_kd_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_ce_upsample_kd_ws_floats': (i64, [i32, i32, i32]),
    'addk_ce_upsample_kd_fwd_bwd': (i32, [C.POINTER(CeUpsampleKdArgs), vp]),
    'addk_dice_stats_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_dice_stats_ws_bytes': (i64, [i32, i32, i32]),
    'addk_dice_stats_ws_bytes_classes': (i64, [i32, i32, i32, i32]),
    'addk_dice_stats': (i32, [C.POINTER(DiceStatsArgs), vp]),
    'addk_ce_upsample_dice_fwd_bwd': (i32, [C.POINTER(CeUpsampleDiceArgs), vp]),
    'addk_ce_upsample_shaped_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_ce_upsample_shaped_fwd_bwd': (i32, [C.POINTER(CeUpsampleShapedArgs), vp]),
    'addk_score_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_score_upsample_ws_floats': (i64, [i32, i32, i32]),
    'addk_score_upsample': (i32, [C.POINTER(ScoreUpsampleArgs), vp]),
    'addk_gate_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_gate_upsample_ws_bytes': (i64, [i32, i32, i32]),
    'addk_gate_upsample': (i32, [C.POINTER(GateUpsampleArgs), vp]),
    'addk_label_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_label_upsample': (i32, [C.POINTER(LabelUpsampleArgs), vp]),
    'addk_gate_label_upsample': (i32, [C.POINTER(GateLabelUpsampleArgs), vp]),
    'addk_label_views_upsample_supported': (i32, [i32, i32, i32, i32, i32]),
    'addk_label_views_upsample': (i32, [C.POINTER(LabelViewsArgs), vp]),
    'addk_gather_tiles': (i32, [vp, i32, i32, i32, i32, vp, i32, vp]),
    'addk_label_tiles_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_label_tiles_upsample': (i32, [C.POINTER(LabelTilesArgs), vp]),
    'addk_gather_tile_views': (i32, [vp, i32, i32, i32, i32, vp, i32, vp]),
    'addk_label_tile_views_upsample_supported': (i32, [i32, i32, i32, i32, i32]),
    'addk_label_tile_views_upsample': (i32, [C.POINTER(LabelTileViewsArgs), vp]),
    'addk_gate_tiles_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32]),
    'addk_gate_tiles_upsample_ws_bytes': (i64, [i32, i32, i32]),
    'addk_gate_tiles_upsample': (i32, [C.POINTER(GateTilesArgs), vp]),
    'addk_scatter_tile_logits': (i32, [C.POINTER(ScatterTileLogitsArgs), vp]),
    'addk_profile_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32, i32]),
    'addk_profile_upsample_ws_bytes': (i64, [i32, i32, i32]),
    'addk_profile_upsample': (i32, [C.POINTER(ProfileUpsampleArgs), vp]),
    'addk_gate_upsample_t': (i32, [C.POINTER(GateUpsampleTArgs), vp]),
    'addk_profile_upsample_t': (i32, [C.POINTER(ProfileUpsampleTArgs), vp]),
    'addk_calib_upsample_supported': (i32, [i32, i32, i32, i32, i32, i32, i32]),
    'addk_calib_upsample_ws_bytes': (i64, [i32, i32, i32]),
    'addk_calib_upsample': (i32, [C.POINTER(CalibUpsampleArgs), vp]),
    'addk_sgd_step': (i32, [vp, vp, vp, i64, vp, f32, f32, i32, i32, f32, vp]),
    'addk_fill': (i32, [vp, i64, f32, vp]),
    'addk_entropy_sum': (i32, [vp, i32, i32, i64, vp, vp, vp]),
    'addk_argmax_nchw': (i32, [vp, i32, i32, i64, vp, vp]),
    'addk_confusion': (i32, [vp, vp, i64, i32, vp, vp]),
    'addk_boundary_dist_supported': (i32, [i32, i32, i32, i32, i32]),
    'addk_boundary_dist_ws_bytes': (i64, [i32, i32, i32]),
    'addk_boundary_dist': (i32, [C.POINTER(BoundaryDistArgs), vp]),
    'addk_confusion_banded_supported': (i32, [i32, i32, i32, i32, i32]),
    'addk_confusion_banded': (i32, [C.POINTER(ConfusionBandedArgs), vp]),
    'addk_gather_rows': (i32, [C.POINTER(GatherRowsArgs), vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


class AddkError(RuntimeError):
    pass


def load():
    """Load libaddk.so and bind every declared symbol.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AddkError('libaddk.so not found at %s — run `python -c "import __graft_entry__ as g; g.build()"` '
                        '(hipcc --offload-arch=gfx950).  addk has no CPU fallback.' % LIB_PATH)
    # libaddk.so needs libamdhip64.so.7; PyTorch bundles its own copy under the same soname.  Import torch FIRST so that the
    # process has one HIP runtime (torch's): loaded the other way round, launches on torch's streams fail with
    # hipErrorNoDevice ("no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _classes(query):
    out = (i32 * query(None, 0))()
    query(out, len(out))
    return tuple(out)


def _classes_text(counts):
    first, *more = counts
    return '%d classes' % first + (' (or %s)' % ', '.join(map(str, more)) if more else '')


def head_classes():
    """The class counts the training heads and the label head are compiled for (`addk_head_classes`: csrc/up.h holds the list)."""
    return _classes(load().addk_head_classes)


def gate_head_classes():
    """The class counts the scoring, profile, calibration, gate and multi-view heads are compiled for (`addk_gate_head_classes`)."""
    return _classes(load().addk_gate_head_classes)


def head_classes_text():
    """'19 classes (or 21)': how the error messages name head_classes()."""
    return _classes_text(head_classes())


def gate_head_classes_text():
    """'19 classes': how the error messages name gate_head_classes()."""
    return _classes_text(gate_head_classes())


def check(rc, what=''):
    if rc != 0:
        raise AddkError('%s failed (%d): %s' % (what or 'addk call', rc, load().addk_last_error().decode()))
