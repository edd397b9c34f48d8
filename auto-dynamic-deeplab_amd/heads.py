"""The consumers of the decoder's low-resolution logits: what plan.Graph.resize_to_nchw emits for an exit whose plan names a head
(`Graph.head`, `Graph.lut`) or a gate (`Graph.gate`).  HEADS maps the head's name to the function that emits it, logits_head states
which of them takes an exit.  Every function takes the Graph first and uses only its emission interface: src, lz, _add, buf, _rs_args,
_grad_into, keep, nbytes, lib, device, and the late-emitter lists _fwd_late / _bwd_emitters."""
import ctypes as C
import math

import torch

from . import _lib as L
from .plan import OutRef, _on


def _logits_resize(g, src, OH, OW):
    """The full-resolution logits: (y [N,C,OH,OW], emit); emit() appends the `resize_nchw` launch that writes y, now or later."""
    y = torch.empty((src.N, src.C, OH, OW), dtype=torch.float32, device=g.device)
    g.nbytes += y.numel() * 4
    ar = g._rs_args(L.ResizeArgs, src, OH, OW)
    ar.y, ar.ldy, ar.nchw_out = y.data_ptr(), 0, 1
    g.keep.append(ar)
    return y, lambda: g._add(g.fwd, 'resize_nchw', g.lib.addk_resize_fwd, C.byref(ar), rd=g.lz(src), wr=[y])


def _up_args(g, cls, src, OH, OW):
    """A *UpsampleArgs struct with the prefix the three share filled in: the low-resolution NHWC logits and the two grids."""
    a, s = cls(), g.src(src)
    a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = s.x, s.ld, src.N, src.H, src.W, src.C, OH, OW
    return a


def _late_head(g, head, src, OH, OW, lst, emitters, emit):
    """The OutRef of a head whose step binds its tensors only after the module tree was emitted: no resize, no [N,C,OH,OW] buffer, `y`
    is None and `shape` says what the logits would be.  finalize() runs `emitters`; by then `binding` must be there, and
    `emit(binding)` appends the head's launches to `lst` under the tag of the exit."""
    out = OutRef(None)
    out.head, out.shape = head, (src.N, src.C, OH, OW)
    tag = g.tag

    def late():
        assert out.binding is not None, 'fused logits output without a %s binding' % head
        first = len(lst)
        emit(out.binding)
        for c in lst[first:]:
            c.tag = tag
    emitters.append(late)
    return out


def _bind_loss(a, b):
    """The loss binding a step attached to an OutRef ('ce' / 'score') into the loss head's or the scoring head's arguments."""
    a.target, a.class_w, a.ignore_index = b['target'].data_ptr(), b['class_w'], b['ignore_index']
    a.wsum, a.scale, a.loss_out = b['wsum'].data_ptr(), b['scale'], b['loss'].data_ptr()


def _ce_head(g, src, OH, OW):
    """Logits output of a fused training step (head 'ce', set by train.TrainStep): nobody reads the full-resolution logits, so
    the resize is not emitted at all and the OutRef carries `shape` and the `binding` TrainStep sets; finalize() then places ONE
    fused up-sampling + cross-entropy launch (`addk_ce_upsample_fwd_bwd`) at the head of the backward list.  A binding with
    `ohem = (thresh, min_kept_total)` mines hard examples (include/addk.h, addk_ohem_select): `ohem_select` leaves this exit's own
    per-pixel loss map, tau and kept weight sum, and `ce_upsample_ohem` is the loss head that reads them; the binding gets the
    tensors back as `ohem_state` (TrainStep.ohem_stats).  A binding with `distill = (alpha, temperature, teacher OutRef)` and `nvalid`
    (the count word) makes the exit a student of the teacher's low-resolution logits (`OutRef.src`): `ce_upsample_kd` takes the place
    of `ce_upsample` / `ce_upsample_ohem`, and the binding gets `distill_state` (TrainStep.distill_stats).  A binding with
    `dice = (weight, smooth)` adds the soft-Dice region term (include/addk.h, addk_dice_stats): `dice_stats`, directly in front of the
    head, leaves the coefficient table and the term; the head is `ce_upsample_dice`, whatever else it is, and reads the table; the
    binding gets `dice_state` (TrainStep.dice_stats).  A binding with `focal = gamma` or `smooth = eps` (never both, never with `distill`)
    shapes the per-pixel loss (include/addk.h, addk_ce_upsample_shaped_fwd_bwd): the ONE launch `ce_upsample_shaped` stands where
    `ce_upsample`, `ce_upsample_ohem` or `ce_upsample_dice` would, with their arguments inside its own, their reads and their writes;
    `ohem_select` and `dice_stats` in front of it are untouched."""
    def emit_ce(ce):
        lib, ohem, kd, dice = g.lib, ce.get('ohem'), ce.get('distill'), ce.get('dice')
        focal, smooth = ce.get('focal'), ce.get('smooth')
        shaped = focal is not None or smooth is not None
        assert not (shaped and kd) and (focal is None or smooth is None), 'a shaped loss head has no distillation form and one shape'
        f32 = dict(dtype=torch.float32, device=g.device)
        a = _up_args(g, L.CeUpsampleArgs, src, OH, OW)
        _bind_loss(a, ce)
        gs, a.accumulate, _ = g._grad_into(src)
        a.g, a.ldg = gs.ptr, gs.ld
        ws_floats = lib.addk_ce_upsample_kd_ws_floats if kd else lib.addk_ce_upsample_ws_floats
        ws = torch.zeros(int(ws_floats(src.N, src.H, src.W)), **f32)
        a.ws = ws.data_ptr()
        g.keep += [a, ws]
        if kd:                                         # the KL term's word: kept here, before the mining tensors (the plan's kept order)
            kdo = torch.zeros(1, **f32)
            g.keep.append(kdo)
        # the launch: the plain head, unless a block below changes it; the KD struct is a superset of the mining struct
        args = L.CeUpsampleKdArgs() if kd or dice or shaped else L.CeUpsampleOhemArgs() if ohem else a
        name, fn, norm = 'ce_upsample', lib.addk_ce_upsample_fwd_bwd, [ce['wsum']]
        rd_more, wr = [], [gs, ce['loss'], ws]
        if ohem:
            # mining: this exit's loss map, tau and kept weight sum; the head reads them, the kept weight sum is its normaliser
            if lib.addk_ohem_select_supported(src.N, src.H, src.W, OH, OW, src.C) != 1:
                raise L.AddkError('hard example mining takes %s and fewer than 2^31 pixels (got %d classes, [%d,%d,%d] -> %dx%d)'
                                  % (L.head_classes_text(), src.C, src.N, src.H, src.W, OH, OW))
            lmap, tau, wkept = torch.zeros((src.N, OH, OW), **f32), torch.zeros(1, **f32), torch.zeros(1, **f32)
            counts = torch.zeros(2, dtype=torch.int64, device=g.device)
            sws = torch.zeros(int(lib.addk_ohem_select_ws_bytes(src.N, OH, OW)), dtype=torch.uint8, device=g.device)
            g.nbytes += lmap.numel() * 4
            s = _up_args(g, L.OhemSelectArgs, src, OH, OW)
            s.target, s.class_w, s.ignore_index = a.target, a.class_w, a.ignore_index
            s.thresh, s.min_kept_total = ohem
            s.pix_loss, s.tau, s.wsum_kept, s.counts, s.ws = lmap.data_ptr(), tau.data_ptr(), wkept.data_ptr(), counts.data_ptr(), sws.data_ptr()
            ce['ohem_state'] = dict(pix_loss=lmap, tau=tau, wsum_kept=wkept, counts=counts)
            g.keep += [s, lmap, tau, wkept, counts, sws]
            g._add(g.bwd, 'ohem_select', lib.addk_ohem_select, C.byref(s), rd=g.lz(src) + [ce['target']], wr=[lmap, tau, wkept, counts, sws])
            a.wsum, args.pix_loss, args.tau = wkept.data_ptr(), lmap.data_ptr(), tau.data_ptr()
            name, fn, norm = 'ce_upsample_ohem', lib.addk_ce_upsample_ohem_fwd_bwd, [lmap, tau, wkept]
        if kd:
            # a student: the head's own normaliser and kept set as above, plus the last exit's low-resolution logits and the count word
            alpha, temp, teacher = kd
            tsrc = teacher.src
            assert tsrc.bn is None and not tsrc.relu and (tsrc.N, tsrc.H, tsrc.W, tsrc.C) == (src.N, src.H, src.W, src.C)
            t = g.src(tsrc)
            args.teacher, args.ld_teacher, args.alpha, args.temperature = t.x, t.ld, alpha, temp
            args.nvalid, args.kd_out = ce['nvalid'].data_ptr(), kdo.data_ptr()
            ce['distill_state'] = dict(kd=kdo)
            name, fn = 'ce_upsample_kd', lib.addk_ce_upsample_kd_fwd_bwd
            rd_more, wr = g.lz(tsrc) + [ce['nvalid']], wr + [kdo]
        if args is not a:
            args.ce = a                                # a copy of the base arguments, with the final normaliser
            g.keep.append(args)
        if dice:
            # the region term: the batch's per-class sums first (they add the term to the loss), then the head with their table
            if lib.addk_dice_stats_supported(src.N, src.H, src.W, OH, OW, src.C) != 1:
                raise L.AddkError('the soft-Dice term takes %s and fewer than 2^31 pixels (got %d classes, [%d,%d,%d] -> %dx%d)'
                                  % (L.head_classes_text(), src.C, src.N, src.H, src.W, OH, OW))
            coef, dout = torch.zeros(2 * src.C, **f32), torch.zeros(1 + src.C, **f32)
            dws = torch.zeros(int(lib.addk_dice_stats_ws_bytes_classes(src.N, OH, OW, src.C)), dtype=torch.uint8, device=g.device)
            d = _up_args(g, L.DiceStatsArgs, src, OH, OW)
            d.target, d.ignore_index, d.scale, d.loss_out = a.target, a.ignore_index, a.scale, a.loss_out
            d.weight, d.smooth = dice
            d.coef, d.dice_out, d.ws = coef.data_ptr(), dout.data_ptr(), dws.data_ptr()
            ce['dice_state'] = dict(dice=dout, coef=coef)
            g._add(g.bwd, 'dice_stats', lib.addk_dice_stats, C.byref(d), rd=g.lz(src) + [ce['target']], wr=[coef, dout, ce['loss'], dws])
            head = L.CeUpsampleDiceArgs()
            head.kd, head.coef = args, coef.data_ptr()       # a copy of the head's arguments, complete by now
            g.keep += [d, coef, dout, dws, head]
            args, name, fn, rd_more = head, 'ce_upsample_dice', lib.addk_ce_upsample_dice_fwd_bwd, rd_more + [coef]
        if shaped:
            # the shape: the head's arguments, complete by now (kept set and table included), inside the shaped launch's own
            sh = L.CeUpsampleShapedArgs()
            if dice:
                sh.dice = args
            else:
                sh.dice.kd = args
            if focal is not None:
                sh.shape, sh.gamma = L.CE_SHAPE_FOCAL, focal
            else:
                sh.shape, sh.eps = L.CE_SHAPE_SMOOTH, smooth
            g.keep.append(sh)
            args, name, fn = sh, 'ce_upsample_shaped', lib.addk_ce_upsample_shaped_fwd_bwd
        g._add(g.bwd, name, fn, C.byref(args), rd=g.lz(src) + [ce['target']] + norm + rd_more, wr=wr)
    out = _late_head(g, 'ce', src, OH, OW, g.bwd, g._bwd_emitters, emit_ce)
    out.src = src
    return out


def _score_head(g, src, OH, OW):
    """Logits output of a validation plan (head 'score', set by validate.ValidationStep): nobody reads the full-resolution
    logits, so no resize is emitted and no [N,C,OH,OW] buffer exists.  The OutRef carries `shape` and the `binding` the step
    sets (target, class weights, wsum and the per-exit loss / entropy / confusion / prediction tensors); finalize() then appends
    ONE `score_upsample` launch per exit to the forward list (`addk_score_upsample`).  Where the library does not take the shape
    (`addk_score_upsample_supported` == 0, e.g. a class count outside `_lib.gate_head_classes()`) the same quantities come from the stand-alone kernels inside this plan:
    resize + ce_fwd_bwd without a gradient + argmax_nchw + confusion + entropy_sum.  A binding with `trimap` (_confusion_banded) adds
    ONE `confusion_banded` launch behind the exit's `score_upsample`; the stand-alone path refuses it (ValueError)."""
    lib = g.lib
    N, H, W, Cc = src.N, src.H, src.W, src.C

    def emit_score(sc):
        tgt, wsum, loss, ent, cm, pred = sc['target'], sc['wsum'], sc['loss'], sc['entropy'], sc['confusion'], sc.get('pred')
        if lib.addk_score_upsample_supported(N, H, W, OH, OW, Cc) == 1:
            a = _up_args(g, L.ScoreUpsampleArgs, src, OH, OW)
            _bind_loss(a, sc)
            a.ent_out, a.cm, a.pred_out = ent.data_ptr(), cm.data_ptr(), pred.data_ptr() if pred is not None else None
            ws = torch.zeros(int(lib.addk_score_upsample_ws_floats(N, OH, OW)), dtype=torch.float32, device=g.device)
            a.ws = ws.data_ptr()
            g.keep += [a, ws]
            g._add(g.fwd, 'score_upsample', lib.addk_score_upsample, C.byref(a),
                   rd=g.lz(src) + [tgt, wsum], wr=[loss, ent, cm, pred, ws])
            if sc.get('trimap') is not None:
                _confusion_banded(g, sc['trimap'], tgt, pred, N, OH, OW, Cc)
        else:
            if sc.get('trimap') is not None:
                raise ValueError('the trimap metric reads the uint8 map of the fused scoring head, which does not take this exit '
                                 '(%d classes, [%d,%d,%d] -> %dx%d): the stand-alone path keeps an int64 map' % (Cc, N, H, W, OH, OW))
            y, emit_resize = _logits_resize(g, src, OH, OW)
            am = torch.empty((N, OH, OW), dtype=torch.int64, device=g.device)
            ws = torch.zeros(int(lib.addk_ce_ws_floats(N, OH * OW)), dtype=torch.float32, device=g.device)
            g.nbytes += am.numel() * 8
            g.keep += [y, am, ws]
            emit_resize()
            g._add(g.fwd, 'ce_fwd_bwd', lib.addk_ce_fwd_bwd, y.data_ptr(), tgt.data_ptr(), N, Cc, OH * OW, sc['class_w'],
                   sc['ignore_index'], wsum.data_ptr(), sc['scale'], loss.data_ptr(), None, ws.data_ptr(),
                   rd=[y, tgt, wsum], wr=[loss, ws])
            g._add(g.fwd, 'argmax_nchw', lib.addk_argmax_nchw, y.data_ptr(), N, Cc, OH * OW, am.data_ptr(), rd=[y], wr=[am])
            g._add(g.fwd, 'confusion', lib.addk_confusion, tgt.data_ptr(), am.data_ptr(), N * OH * OW, Cc, cm.data_ptr(),
                   rd=[tgt, am], wr=[cm])
            # addk_entropy_sum overwrites its output: the step zeroes `ent` before every pass, which makes that the same thing
            g._add(g.fwd, 'entropy_sum', lib.addk_entropy_sum, y.data_ptr(), N, Cc, OH * OW, ent.data_ptr(), ws.data_ptr(),
                   rd=[y], wr=[ent, ws])
            sc['pred_i64'] = am                    # the map of this path is int64: ValidationStep.predictions() narrows it
    return _late_head(g, 'score', src, OH, OW, g.fwd, g._fwd_late, emit_score)


def _profile_head(g, src, OH, OW):
    """Logits output of an exit-profile plan (head 'profile', set by exit_profile.ExitProfile): as in _score_head no resize is emitted
    and no [N,C,OH,OW] buffer exists.  The OutRef carries `shape` and the `binding` the step sets (target, the device array of
    top-probability thresholds and its length, and this exit's per-image entropy [N], share [N,nthr], confusion [N,C,C] and optional
    prediction tensors); finalize() then appends ONE `profile_upsample` launch per exit (`addk_profile_upsample`).  There is no
    stand-alone form: a shape the library does not take is an error.  A binding with `trimap` (_confusion_banded) adds ONE
    `confusion_banded` launch behind the exit's profile launch."""
    lib = g.lib
    N, H, W, Cc = src.N, src.H, src.W, src.C

    def emit_profile(pr):
        tgt, thr, nthr, ent, share, cm, pred = pr['target'], pr['thr'], pr['nthr'], pr['entropy'], pr['share'], pr['confusion'], pr.get('pred')
        if lib.addk_profile_upsample_supported(N, H, W, OH, OW, Cc, nthr) != 1:
            raise L.AddkError('the exit profile takes %s and at most 16 thresholds (got %d classes, %d thresholds, '
                              '[%d,%d,%d] -> %dx%d)' % (L.gate_head_classes_text(), Cc, nthr, N, H, W, OH, OW))
        a = _up_args(g, L.ProfileUpsampleArgs, src, OH, OW)
        a.target, a.thr, a.nthr = tgt.data_ptr(), thr.data_ptr() if nthr else None, nthr
        a.ent_out, a.share_out, a.cm = ent.data_ptr(), share.data_ptr() if nthr else None, cm.data_ptr()
        a.pred_out = pred.data_ptr() if pred is not None else None
        ws = torch.zeros(int(lib.addk_profile_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=g.device)
        a.ws = ws.data_ptr()
        temp = pr.get('temp')
        if temp is not None:                     # the tempered launch: entropy and shares of softmax(z * *temp)
            b = L.ProfileUpsampleTArgs()
            b.profile, b.inv_temp = a, temp.data_ptr()
            g.keep += [b, ws]
            g._add(g.fwd, 'profile_upsample_t', lib.addk_profile_upsample_t, C.byref(b),
                   rd=g.lz(src) + [tgt, thr, temp], wr=[ent, share, cm, pred, ws])
        else:
            g.keep += [a, ws]
            g._add(g.fwd, 'profile_upsample', lib.addk_profile_upsample, C.byref(a),
                   rd=g.lz(src) + [tgt, thr], wr=[ent, share, cm, pred, ws])
        if pr.get('trimap') is not None:
            _confusion_banded(g, pr['trimap'], tgt, pred, N, OH, OW, Cc)
    return _late_head(g, 'profile', src, OH, OW, g.fwd, g._fwd_late, emit_profile)


def _confusion_banded(g, tm, tgt, pred, N, OH, OW, Cc):
    """ONE `confusion_banded` launch (`addk_confusion_banded`) behind the head launch of an exit whose binding carries `trimap`: a dict
    with `rings` (int64 [nw,C,C], or [N,nw,C,C] with `image_stride` = nw*C*C; added to), `widths` and `dist` (the uint8 map the step's one
    `boundary_dist` launch writes).  It reads the head's uint8 prediction map."""
    lib, widths = g.lib, tm['widths']
    assert pred is not None, 'a trimap binding needs the exit\'s uint8 prediction map'
    if lib.addk_confusion_banded_supported(N, OH, OW, Cc, len(widths)) != 1:
        raise ValueError('the trimap metric takes 1 to 32 classes, 1 to %d widths and fewer than 2^31 pixels (got %d classes, %d widths, '
                         '[%d,%d,%d])' % (L.TRIMAP_MAX_WIDTHS, Cc, len(widths), N, OH, OW))
    a = L.ConfusionBandedArgs()
    a.target, a.pred, a.dist = tgt.data_ptr(), pred.data_ptr(), tm['dist'].data_ptr()
    a.N, a.OH, a.OW, a.C, a.nw = N, OH, OW, Cc, len(widths)
    for j, w in enumerate(widths):
        a.width[j] = w
    a.cm, a.image_stride = tm['rings'].data_ptr(), tm.get('image_stride', 0)
    g.keep.append(a)
    g._add(g.fwd, 'confusion_banded', lib.addk_confusion_banded, C.byref(a), rd=[tgt, pred, tm['dist']], wr=[tm['rings']])


def _calib_head(g, src, OH, OW):
    """Logits output of a calibration plan (head 'calib', set by calibrate.ExitCalibration): as in _profile_head no resize is emitted and
    no [N,C,OH,OW] buffer exists.  The OutRef carries `shape` and the `binding` the step sets (target, the device array of inverse
    temperatures and its length, and this exit's bins [nt,16,3] int64 and nll [nt] fp64, both added to); finalize() then appends ONE
    `calib_upsample` launch per exit (`addk_calib_upsample`).  There is no stand-alone form: a shape the library does not take is an
    error."""
    lib = g.lib
    N, H, W, Cc = src.N, src.H, src.W, src.C

    def emit_calib(cb):
        tgt, it, nt, bins, nll = cb['target'], cb['inv_temp'], cb['nt'], cb['bins'], cb['nll']
        if lib.addk_calib_upsample_supported(N, H, W, OH, OW, Cc, nt) != 1:
            raise L.AddkError('the calibration head takes %s and 1..%d temperatures (got %d classes, %d temperatures, '
                              '[%d,%d,%d] -> %dx%d)' % (L.gate_head_classes_text(), L.CALIB_MAX_T, Cc, nt, N, H, W, OH, OW))
        a = _up_args(g, L.CalibUpsampleArgs, src, OH, OW)
        a.target, a.inv_temp, a.nt, a.bins, a.nll = tgt.data_ptr(), it.data_ptr(), nt, bins.data_ptr(), nll.data_ptr()
        ws = torch.zeros(int(lib.addk_calib_upsample_ws_bytes(N, OH, OW)), dtype=torch.uint8, device=g.device)
        a.ws = ws.data_ptr()
        g.keep += [a, ws]
        g._add(g.fwd, 'calib_upsample', lib.addk_calib_upsample, C.byref(a), rd=g.lz(src) + [tgt, it], wr=[bins, nll, ws])
    return _late_head(g, 'calib', src, OH, OW, g.fwd, g._fwd_late, emit_calib)


def _label_map(g, src, OH, OW):
    """The plan-owned uint8 [N,OH,OW] label map of a label head and its OutRef (`shape`: the logits it stands for)."""
    lab = torch.zeros((src.N, OH, OW), dtype=torch.uint8, device=g.device)
    g.nbytes += lab.numel()
    out = OutRef(lab)
    out.head, out.shape = 'labels', (src.N, src.C, OH, OW)
    return lab, out


def _label_head(g, src, OH, OW):
    """Logits output of a label-map plan (head 'labels', set by dynamic.DynamicPlan / GatePlan and segment.Segmenter): what inference
    keeps of an exit is the arg-max of its up-sampled logits (eval.py:218-221), so no resize is emitted and no [N,C,OH,OW] buffer exists.
    ONE `label_upsample` launch (`addk_label_upsample`) writes the OutRef's `y`, a plan-owned uint8 [N,OH,OW] map: the class index, or
    lut[class] with the table `g.lut`.  Where the library does not take the shape (`addk_label_upsample_supported` == 0, e.g.
    a class count outside `_lib.head_classes()`) the same plan uses the stand-alone kernels: resize + argmax_nchw + a cast in torch ops (_labels_cold)."""
    lib = g.lib
    lab, out = _label_map(g, src, OH, OW)
    lut = g.lut
    if lib.addk_label_upsample_supported(src.N, src.H, src.W, OH, OW, src.C) == 1:
        a = _up_args(g, L.LabelUpsampleArgs, src, OH, OW)
        a.lut256, a.labels = lut.data_ptr() if lut is not None else None, lab.data_ptr()
        g.keep += [a, lut]
        g._add(g.fwd, 'label_upsample', lib.addk_label_upsample, C.byref(a), rd=g.lz(src) + [lut], wr=[lab])
    else:
        y, emit_resize = _logits_resize(g, src, OH, OW)
        emit_resize()
        _labels_cold(g, y, lab, lut)
    return out


class _Views:
    """What the 'views' head of one plan knows until finalize(): the OutRefs of the plan's logits outputs, in emission order (= kernel
    order of their views), and the segment tag of the last one, stamped on the one launch.  The first views output creates it as the
    plan's late emitter (Graph._fwd_late), and the later ones find it there."""

    def __init__(self, g):
        self.g, self.outs, self.tag = g, [], ''

    def __call__(self):
        _emit_views(self.g, self.outs, self.tag)


def _views_head(g, src, OH, OW):
    """Logits output of a multi-view plan (head 'views', set by segment.MultiViewSegmenter): the plan emits the model several times —
    once per input scale, at batch 2N where the mirrored images ride along — and ALL its logits outputs end in one label map.  Nothing is
    emitted here and no [N,C,OH,OW] buffer exists: the OutRef keeps the low-resolution source (`src`), `shape`, and the `binding` the step
    sets — {'N': images per view, 'size': (OH, OW) of the map, 'views': [(n0, mirror, weight), ...]}, the views this output holds (n0:
    its first image in the batch).  The (OH, OW) passed here, the size the model would up-sample this output to, only goes into `shape`.
    finalize() then appends ONE `label_views_upsample` launch (`addk_label_views_upsample`) that reads every view's source and writes
    `Graph.view_labels`, the plan-owned uint8 [N,OH,OW] map.  There is no stand-alone form: a class count outside `_lib.gate_head_classes()` or more than 8 views is an error."""
    if src.C not in L.gate_head_classes():
        raise L.AddkError('the multi-view label head takes %s (got %d)' % (L.gate_head_classes_text(), src.C))
    out = OutRef(None)
    out.head, out.shape, out.src = 'views', (src.N, src.C, OH, OW), src
    views = next((em for em in g._fwd_late if isinstance(em, _Views)), None)
    if views is None:
        views = _Views(g)
        g._fwd_late.append(views)
    views.outs.append(out)
    views.tag = g.tag
    return out


def _emit_views(g, outs, tag):
    lib = g.lib
    assert all(o.binding is not None for o in outs), 'multi-view logits output without a views binding'
    views = [(o, v) for o in outs for v in o.binding['views']]
    b0, Cc = outs[0].binding, outs[0].shape[1]
    N, (OH, OW) = b0['N'], b0['size']
    assert all(o.binding['N'] == N and tuple(o.binding['size']) == (OH, OW) and o.shape[1] == Cc for o in outs)
    assert all(0 <= n0 and n0 + N <= o.shape[0] for o, (n0, _, _) in views)
    if len(views) > L.MAX_VIEWS or lib.addk_label_views_upsample_supported(len(views), N, OH, OW, Cc) != 1:
        raise L.AddkError('the multi-view label head takes 1..%d views of %s (got %d views, %d classes, %d x %dx%d)'
                          % (L.MAX_VIEWS, L.gate_head_classes_text(), len(views), Cc, N, OH, OW))
    lab = g.view_labels = torch.zeros((N, OH, OW), dtype=torch.uint8, device=g.device)
    g.nbytes += lab.numel()
    a, lut, rd = L.LabelViewsArgs(), g.lut, []
    for i, (o, (n0, mirror, weight)) in enumerate(views):
        s, v = g.src(o.src), a.view[i]
        v.logits, v.ld, v.n0, v.H, v.W, v.mirror, v.weight = s.x, s.ld, n0, o.src.H, o.src.W, int(bool(mirror)), weight
        rd += g.lz(o.src)
    a.nview, a.N, a.C, a.OH, a.OW = len(views), N, Cc, OH, OW
    a.lut256, a.labels = lut.data_ptr() if lut is not None else None, lab.data_ptr()
    g.keep += [a, lut]
    g._add(g.fwd, 'label_views_upsample', lib.addk_label_views_upsample, C.byref(a), rd=rd + [lut], wr=[lab]).tag = tag


def _tiles_head(g, src, OH, OW):
    """Logits output of a tile plan (head 'tiles', set by segment.TiledSegmenter): the plan is ONE window of a sliding-window pass, and
    what becomes of its logits is decided outside the plan — the step copies each chunk's low-resolution logits into its store and ends a
    call with one `addk_label_tiles_upsample` launch per image, which up-samples, soft-maxes and sums every window that covers a pixel.  So,
    as in _views_head, nothing is emitted here and no [N,C,OH,OW] buffer exists: the OutRef keeps the low-resolution source (`src`) and
    `shape`.  There is no stand-alone form: a class count outside `_lib.head_classes()` is an error, and so is a gate."""
    if g.gate is not None:
        raise L.AddkError('the tiled label head has no gated form: a window is no image to leave early with')
    if src.C not in L.head_classes():
        raise L.AddkError('the tiled label head takes %s (got %d)' % (L.head_classes_text(), src.C))
    out = OutRef(None)
    out.head, out.shape, out.src = 'tiles', (src.N, src.C, OH, OW), src
    g.lz(src)                                    # a still-deferred resize of the logits is emitted now: the step reads src.raw itself
    return out


def _tile_gate_head(g, src, OH, OW):
    """Logits output of a gated tile plan (head 'tile_gate', set by segment.TileGatePlan): the plan is ONE chunk of windows of a
    sliding-window pass whose windows leave at the first exit that is sure of them.  As in _tiles_head nothing becomes of the logits
    inside the plan — the step scatters the rows that leave into its store (`addk_scatter_tile_logits`) — and the OutRef keeps the
    low-resolution source (`src`) and `shape`.  An early exit (`Graph.gate` is set: GatePlan's dict plus 'ext', the int32 [B,2] device
    words of every slot's valid extent) ends in ONE `gate_tiles_upsample` launch (`addk_gate_tiles_upsample`) that judges every window
    over the part of it that lies on its image and writes (entropy, share) to `gate_out` [B,2] and to the pinned words; `gate_cut` is
    the list position behind it.  The last exit (no gate) emits nothing.  There is no stand-alone form: a class count outside
    `_lib.head_classes()` or a shape the gate launch does not take is an error."""
    lib, gate = g.lib, g.gate
    if src.C not in L.head_classes():
        raise L.AddkError('the tiled label head takes %s (got %d)' % (L.head_classes_text(), src.C))
    out = OutRef(None)
    out.head, out.shape, out.src = 'tile_gate', (src.N, src.C, OH, OW), src
    rd = g.lz(src)                               # a still-deferred resize of the logits is emitted now: the step reads src.raw itself
    if gate is None:
        return out
    if lib.addk_gate_tiles_upsample_supported(src.N, src.H, src.W, OH, OW, src.C) != 1:
        raise L.AddkError('the tile gate takes %s (got %d classes, [%d,%d,%d] -> %dx%d)'
                          % (L.head_classes_text(), src.C, src.N, src.H, src.W, OH, OW))
    thr, host, ext, temp = gate['thr'], gate['host'], gate['ext'], gate.get('temp')
    a, s = L.GateTilesArgs(), g.src(src)
    a.logits, a.ld, a.B, a.nb, a.h, a.w, a.C, a.th, a.tw = s.x, s.ld, src.N, src.N, src.H, src.W, src.C, OH, OW
    gout = torch.zeros((src.N, 2), dtype=torch.float32, device=g.device)
    ws = g.buf((int(lib.addk_gate_tiles_upsample_ws_bytes(src.N, OH, OW)) + 3) // 4, zero=True)
    a.ext, a.max_thr, a.inv_temp = ext.data_ptr(), thr.data_ptr(), temp.data_ptr() if temp is not None else None
    a.out, a.out_host, a.ws = gout.data_ptr(), host.data_ptr() if host is not None else None, ws.ptr
    g.keep += [a, gout, thr, host, ext, temp]
    g._add(g.fwd, 'gate_tiles_upsample', lib.addk_gate_tiles_upsample, C.byref(a), rd=rd + [thr, ext] + [temp] * (temp is not None),
           wr=[gout, ws])
    out.gate_out, out.gate_fused, out.gate_cut = gout, True, len(g.fwd)
    return out


def _labels_cold(g, y, lab, lut):
    """Cold path of the two label heads: the map from materialised logits y [N,C,OH,OW] — `argmax_nchw`, then the cast / table look-up
    to uint8 in torch ops."""
    N, Cc, OH, OW = y.shape
    am = torch.empty((N, OH, OW), dtype=torch.int64, device=g.device)
    g.nbytes += am.numel() * 8
    g.keep += [y, am, lut]
    g._add(g.fwd, 'argmax_nchw', g.lib.addk_argmax_nchw, y.data_ptr(), N, Cc, OH * OW, am.data_ptr(), rd=[y], wr=[am])
    g._add(g.fwd, 'label_cast_torch', _label_cast_torch, am, lut, lab, rd=[am, lut], wr=[lab], pin=True)


def _gate_args(g, src, OH, OW, thr, gout, host_out):
    """(GateUpsampleArgs, workspace) of the fused gate launch, with and without the label map: a zeroed ticket workspace of its own"""
    a = _up_args(g, L.GateUpsampleArgs, src, OH, OW)
    ws = g.buf((int(g.lib.addk_gate_upsample_ws_bytes(src.N, OH, OW)) + 3) // 4, zero=True)
    a.max_thr, a.out, a.ws = thr.data_ptr(), gout.data_ptr(), ws.ptr
    a.out_host = host_out.data_ptr() if host_out is not None else None
    return a, ws


def gate_head(g, src, OH, OW, host_out, thr, kind='entropy', temp=None):
    """Logits output of a gated early exit (`Graph.gate`, set by dynamic.GatePlan): the exit's gate value (modeling/operations.py:161-180)
    and, separately, the resize that writes the [N,C,OH,OW] logits.  Fused form (_gate_fused): ONE `gate_upsample` launch
    (`addk_gate_upsample`) reads the low-resolution NHWC logits and writes (entropy, share) to the OutRef's `gate_out` [N,2] and to the
    pinned words `host_out`; the `resize_nchw` launch FOLLOWS it, so a plan cut at `gate_cut` replays the resize only for an image that
    leaves here.  `thr`: the device word the 'max' gate compares against.
    Where the library does not take the shape (`addk_gate_upsample_supported` == 0, e.g. a class count outside `_lib.gate_head_classes()`) or with ADDK_FUSE_GATE=0, the same
    plan uses the stand-alone kernels on the materialised logits (_gate_alone) — `resize_nchw` first, then `entropy_sum` ('entropy':
    gate_out[0, 0] holds the un-normalised sum, `gate_scale` the factor the host applies) or a count in torch ops ('max':
    gate_out[0, 1]); nothing is left behind the cut and the host copies `gate_out` itself (`gate_fused` False).
    In a label-map plan (head 'labels') the OutRef's `y` is the uint8 [N,OH,OW] map of _label_head.  Fused form: ONE
    `gate_label_upsample` launch (`addk_gate_label_upsample`) leaves the gate value AND the map, for every image; nothing follows the
    cut and no [N,C,OH,OW] buffer exists.  Stand-alone form: the stand-alone gate above, then, behind the cut, _labels_cold.
    `temp`: the device word 1 / temperature of a tempered gate, which judges softmax(z * *temp): ONE `gate_upsample_t` launch
    (`addk_gate_upsample_t`) stands where `gate_upsample` / `gate_label_upsample` stand, everything else is the same.  There is no
    stand-alone tempered form: a shape the library does not take, or ADDK_FUSE_GATE=0, is an error."""
    N, H, W, Cc = src.N, src.H, src.W, src.C
    fused = _on('ADDK_FUSE_GATE') and g.lib.addk_gate_upsample_supported(N, H, W, OH, OW, Cc) == 1
    if temp is not None and not fused:
        raise L.AddkError('a tempered gate needs the fused gate launch: %s and ADDK_FUSE_GATE=1 (got %d classes, [%d,%d,%d] -> %dx%d)'
                          % (L.gate_head_classes_text(), Cc, N, H, W, OH, OW))
    labels = g.head == 'labels'
    # the [N,C,OH,OW] logits and their resize: not where the fused launch of a label plan leaves the map itself
    y, emit_resize = (None, None) if labels and fused else _logits_resize(g, src, OH, OW)
    gout = torch.zeros((N, 2), dtype=torch.float32, device=g.device)
    g.keep += [gout, thr, host_out]
    lab, out = _label_map(g, src, OH, OW) if labels else (None, OutRef(y))
    out.gate_out, out.gate_fused = gout, fused
    if fused:
        _gate_fused(g, src, OH, OW, out, lab, emit_resize, host_out, thr, temp)
    else:
        _gate_alone(g, out, y, lab, emit_resize, thr, kind)
    return out


def _gate_fused(g, src, OH, OW, out, lab, emit_resize, host_out, thr, temp):
    """The fused gate launch in the form (label map or not, tempered or not) selects, the cut behind it, and behind the cut the resize
    of a logits output (`lab` is None)."""
    labels, tempered, lut = lab is not None, temp is not None, g.lut
    a, ws = _gate_args(g, src, OH, OW, thr, out.gate_out, host_out)
    name, kept = 'gate_upsample_t' if tempered else 'gate_label_upsample' if labels else 'gate_upsample', []
    if tempered or labels:                       # the plain gate's arguments, complete by now, inside the form's own struct
        gate, a, kept = a, (L.GateUpsampleTArgs if tempered else L.GateLabelUpsampleArgs)(), [lut]
        a.gate = gate
    if tempered:
        a.inv_temp, kept = temp.data_ptr(), kept + [temp]
    if labels:
        a.lut256, a.labels = lut.data_ptr() if lut is not None else None, lab.data_ptr()
    g.keep += [a] + kept
    g._add(g.fwd, name, getattr(g.lib, 'addk_' + name), C.byref(a), rd=g.lz(src) + [thr] + [temp] * tempered + [lut] * labels,
           wr=[out.gate_out, ws] + [lab] * labels)
    out.gate_cut = len(g.fwd)
    if not labels:
        emit_resize()


def _gate_alone(g, out, y, lab, emit_resize, thr, kind):
    """The stand-alone gate on the materialised logits `y`: the resize, `entropy_sum` or the count in torch ops, the cut, and behind the
    cut the map of a label plan (`lab` is not None)."""
    N, Cc, OH, OW = y.shape
    emit_resize()
    if kind == 'entropy':
        ws = torch.zeros(int(g.lib.addk_ce_ws_floats(N, OH * OW)), dtype=torch.float32, device=g.device)
        g.keep.append(ws)
        g._add(g.fwd, 'entropy_sum', g.lib.addk_entropy_sum, y.data_ptr(), N, Cc, OH * OW, out.gate_out.data_ptr(), ws.data_ptr(),
               rd=[y], wr=[out.gate_out, ws])
        # log 19 at every class count, as the fused launch (csrc/up.h, up_tail_fill): the reference's gate calls
        # normalized_shannon_entropy without num_class (modeling/ADD.py:474), whatever the dataset
        out.gate_scale = 1.0 / (math.log(19.0) * OH * OW)
    else:
        g._add(g.fwd, 'gate_count_torch', _gate_count_torch, y, thr, out.gate_out, rd=[y, thr], wr=[out.gate_out], pin=True)
    out.gate_cut = len(g.fwd)
    if lab is not None:
        _labels_cold(g, y, lab, g.lut)           # behind the cut: only for an image that leaves here


def _gate_count_torch(y, thr, gout, stream):
    """Cold path of gate_head ('max' gate on materialised logits): share of pixels with 1 / sum_c exp(z_c - max z) > thr, in torch
    ops on the current stream (the command is pinned to the plan's main stream, which is the current one in eager runs and captures)."""
    se = (y - y.amax(1, keepdim=True)).exp_().sum(1)
    gout[:, 1] = (se.reciprocal_() > thr).flatten(1).float().mean(1)
    return 0


def _label_cast_torch(am, lut, lab, stream):
    """Cold path of the label heads: the int64 arg-max map as uint8, through the table where there is one; torch ops on the current
    stream (pinned to the plan's main stream, as _gate_count_torch)."""
    lab.copy_(am if lut is None else lut[am])
    return 0


def label_lut(lut, device):
    """`label_lut` of the public label-map calls as what the plan binds: None, or a uint8 [256] tensor on `device`.  Anything that is
    not 256 uint8 entries is a ValueError."""
    if lut is None:
        return None
    t = lut if isinstance(lut, torch.Tensor) else torch.as_tensor(lut)
    if t.dtype != torch.uint8 or tuple(t.shape) != (256,):
        raise ValueError('label_lut must be 256 uint8 entries (got %s %s)' % (t.dtype, tuple(t.shape)))
    return t.detach().to(device).contiguous().clone()


# Graph.head / OutRef.head: who consumes the decoder's low-resolution logits -> the function that emits that head.  None (no entry) =
# nobody: Graph.resize_to_nchw writes [N,C,OH,OW] itself.  A gate (Graph.gate) is no head of its own: it composes with None and 'labels'.
HEADS = {'ce': _ce_head, 'score': _score_head, 'profile': _profile_head, 'calib': _calib_head, 'labels': _label_head, 'views': _views_head,
         'tiles': _tiles_head, 'tile_gate': _tile_gate_head}


def logits_head(g, src, OH, OW):
    """The OutRef of the head that takes this logits output, or None where the plain resize does.  A plan with gradients only ever takes
    'ce', and only where the library takes the shape and the logits need a gradient.  An inference plan takes 'score', 'profile' or 'calib'
    first ('tile_gate' among them: it emits its own gate); then its gate, over head None or 'labels' ('tiles' refuses one); then 'labels',
    'views' or 'tiles'."""
    head, gate = g.head, g.gate
    if g.want_grad:
        fused = head == 'ce' and src.needs_grad and g.lib.addk_ce_upsample_supported(src.N, src.H, src.W, OH, OW, src.C) == 1
        return HEADS['ce'](g, src, OH, OW) if fused else None
    if head in ('score', 'profile', 'calib', 'tile_gate'):
        return HEADS[head](g, src, OH, OW)
    if gate is not None and head != 'tiles':     # 'tiles' has no gated form: _tiles_head refuses the gate
        return gate_head(g, src, OH, OW, gate['host'], gate['thr'], gate['kind'], gate.get('temp'))
    if head in ('labels', 'views', 'tiles'):
        return HEADS[head](g, src, OH, OW)
    return None
