#!/usr/bin/env python
"""Writes tests/golden/head_parent_bits.json: sha256 of what the logits heads (csrc/loss_up.hip, score_up.hip, label_up.hip, shared
code in up.h) write on seeded inputs -- first the three the tool began with, addk_ce_upsample_fwd_bwd (fused loss head),
addk_score_upsample (validation scoring head) and addk_gate_upsample (exit gate), then the heads that came after them (below).  All
read the decoder's low-resolution NHWC logits through a bilinear up-sampling and are deterministic by construction (partial sums
added in a fixed order, integer histogram atomics, a last-arriver ticket), so a hash of their outputs is well defined.

N = 2, 19 classes; the shapes are the smallest that reach every branch (CASES), each with pixel stride 24 (16-byte loads, finite
garbage in the padding channels) and 19 (scalar loads).  Per launch every buffer the launch writes is hashed, workspace and ticket
word included:
  score  plain / class-weighted x with / without the uint8 map; targets with 255, labels >= 19 and negative labels; loss, entropy
         and confusion matrix start non-zero; map and workspace prefilled (77 / NaN)
  gate   thresholds 0.2 / 0.8 x with / without the pinned host words; outputs prefilled, workspace zeroed (its ticket's contract)
  ce     accumulate 0 onto a NaN gradient (plain), accumulate 1 onto a seeded gradient (class-weighted); loss starts non-zero;
         a shape with more than 16 output rows in a band (`two_pass`) is recorded as refused: addk_ce_upsample_supported == 0 and
         the launch returns an error code with every buffer untouched
The later heads take further inputs from a RandomState(seed + 1000) of their own (make_inputs2, hashed as `inputs2`), so the inputs and
records of the first three stay what they were:
  ce_ohem     addk_ohem_select (thresh 0.7, min_kept_total = a sixteenth of the valid pixels, at least 1), then
              addk_ce_upsample_ohem_fwd_bwd, the two launches of `ce`; map, tau, kept weight sum, counts, the select workspace, g, loss, ws
  ce_kd       addk_ce_upsample_kd_fwd_bwd, alpha 0.5, T 2: teacher stride 24 and 19 x without / with mining; g, loss, kd_out, both halves of ws
  label       addk_label_upsample without a table and with a reversed table
  gate_label  addk_gate_label_upsample, the four launches of `gate`; also the map
  profile     addk_profile_upsample, 0 / 3 / 16 thresholds x with / without the prediction map; the per-image matrices start non-zero
  views       addk_label_views_upsample, three views (the case's own grid; (H+3, W+5) mirrored, image offset 1 in a batch of N + 1;
              (2H, 2W); weights 0.5, 1, 1.5): every view at the run's stride, and the second view at stride 19
`two_pass` is refused by ce_ohem and ce_kd as it is by ce (the select before them runs); the gather heads take it.

Run it on the MI355X with the library of the commit whose bits are to be pinned (ADDK_LIB selects another build of libaddk.so):

    ADDK_LIB=/path/to/parent/libaddk.so python tests/tools/make_head_bits.py

tests/test_gpu_head_bits.py imports CASES, LDS, KERNELS, make_inputs and run_case from here and compares a library with the fixture.
The inputs come from numpy.random.RandomState, whose stream is frozen; their hash is stored too, so that a changed input shows up as
such and not as a changed kernel."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'head_parent_bits.json')

N, NC = 2, 19
# name, (H, W), (OH, OW), seed
CASES = [
    ('x8', (8, 16), (64, 128), 500),                 # integer ratio, full tiles
    ('odd_ladder', (9, 17), (65, 129), 501),         # non-integer ratio, a one-pixel partial tile in X and in Y
    ('partial_tiles', (5, 7), (33, 49), 502),        # OW < 64, one ce_up column block
    ('two_pass', (5, 7), (60, 49), 503),             # 12 output rows per input row; 18 in the first band, more than ce_up takes: refused
    ('two_pass_ce', (5, 7), (50, 49), 505),          # 10 output rows per input row, 15 in the first band: ce_up's band takes two passes of 8 rows
    ('bands', (16, 33), (128, 264), 504),            # two input rows per ce_up block and two column blocks: the carry and the left-neighbour lane
]
LDS = (24, 19)
KERNELS = ('score', 'gate', 'ce', 'ce_ohem', 'ce_kd', 'label', 'gate_label', 'profile', 'views')
NTHR = 16
ODD_LABELS = [19, 20, 254, 256, 1000, 2 ** 40, -1, -2, -255, -1000, -2 ** 40, 19]


def sha(*arrays):
    h = hashlib.sha256()
    for v in arrays:
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def make_inputs(case):
    """({name: array}, sha256 of all of them): x (19 channels), pad (the 5 padding channels of stride 24), target, class_w, g0
    (stride 24; stride 19 takes its first 19 channels), cm0."""
    name, (H, W), (OH, OW), seed = case
    rs = np.random.RandomState(seed)
    arrs = {'x': (3.0 * rs.standard_normal((N, H, W, NC))).astype(np.float32),
            'pad': (50.0 * rs.standard_normal((N, H, W, 24 - NC))).astype(np.float32)}
    t = rs.randint(0, NC, (N, OH, OW)).astype(np.int64)
    t[rs.random_sample((N, OH, OW)) < 0.05] = 255
    t.reshape(-1)[rs.choice(t.size, len(ODD_LABELS), replace=False)] = ODD_LABELS
    arrs['target'] = t
    arrs['class_w'] = (rs.random_sample(NC) + 0.5).astype(np.float32)
    arrs['g0'] = rs.standard_normal((N, H, W, 24)).astype(np.float32)
    arrs['cm0'] = rs.randint(0, 1 << 40, (NC, NC)).astype(np.int64)
    return arrs, sha(*[arrs[k] for k in sorted(arrs)])


def make_inputs2(case):
    """The further inputs of the later heads, from their own stream: the teacher's logits tx / tpad on the case's grid, the second and
    third view (v2x / v2pad, N + 1 images; v3x / v3pad), the profile's thresholds and its per-image matrices pcm0."""
    name, (H, W), (OH, OW), seed = case
    rs = np.random.RandomState(seed + 1000)
    arrs = {}
    for key, n, h, w in (('t', N, H, W), ('v2', N + 1, H + 3, W + 5), ('v3', N, 2 * H, 2 * W)):
        arrs[key + 'x'] = (3.0 * rs.standard_normal((n, h, w, NC))).astype(np.float32)
        arrs[key + 'pad'] = (50.0 * rs.standard_normal((n, h, w, 24 - NC))).astype(np.float32)
    arrs['thr'] = np.sort(rs.random_sample(NTHR)).astype(np.float32)
    arrs['pcm0'] = rs.randint(0, 1 << 40, (N, NC, NC)).astype(np.int64)
    return arrs, sha(*[arrs[k] for k in sorted(arrs)])


def wsum(arrs, weighted):
    """The loss denominator of nn.CrossEntropyLoss, as addk_ce_count leaves it: the (weights of the) labels in [0, 19) but 255."""
    t = arrs['target']
    ok = (t >= 0) & (t < NC)
    return np.float32(arrs['class_w'][t[ok]].astype(np.float64).sum() if weighted else ok.sum())


def run_case(L, case, ld, kernel, arrs):
    """The launches of one kernel on one case and pixel stride: {launch: {buffer: sha256}}."""
    import torch
    lb = L.load()
    name, (H, W), (OH, OW), seed = case
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    x = np.concatenate([arrs['x'], arrs['pad']], axis=3) if ld == 24 else arrs['x']
    assert x.shape[3] == ld
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    td = torch.from_numpy(arrs['target']).to(dev)
    wd = torch.from_numpy(arrs['class_w']).to(dev)
    full = lambda v, *sh, dt=torch.float32: torch.full(sh, v, device=dev, dtype=dt)      # noqa: E731
    hashes = lambda b: {k: sha(v.cpu().numpy()) for k, v in sorted(b.items()) if v is not None}      # noqa: E731

    def prefix(a):
        a.logits, a.ld, a.N, a.H, a.W, a.C, a.OH, a.OW = xd.data_ptr(), ld, N, H, W, NC, OH, OW

    def loss_binding(a, weighted, ws_dev):
        a.target, a.class_w, a.ignore_index = td.data_ptr(), wd.data_ptr() if weighted else None, 255
        a.wsum, a.scale = ws_dev.data_ptr(), 0.5

    def logits(key, stride):
        """a further NHWC map of arrs (teacher, view) on the device at the given pixel stride"""
        v = np.concatenate([arrs[key + 'x'], arrs[key + 'pad']], axis=3) if stride == 24 else arrs[key + 'x']
        return torch.from_numpy(np.ascontiguousarray(v)).to(dev)

    def ce_args(acc, wsd, nws=None):
        """the argument block and the buffers of a loss-head launch: accumulate 0 onto NaN without class weights, 1 onto g0 with them"""
        g = torch.from_numpy(np.ascontiguousarray(arrs['g0'][..., :ld])).to(dev) if acc else full(float('nan'), N, H, W, ld)
        b = {'loss': full(0.25, 1), 'g': g, 'ws': full(float('nan'), nws if nws is not None else int(lb.addk_ce_upsample_ws_floats(N, H, W)))}
        a = L.CeUpsampleArgs()
        prefix(a)
        loss_binding(a, acc, wsd)
        a.loss_out, a.g, a.ldg, a.accumulate, a.ws = b['loss'].data_ptr(), g.data_ptr(), ld, acc, b['ws'].data_ptr()
        return a, b

    def select(weighted):
        """addk_ohem_select on fresh buffers: {map, tau, wkept, counts, sel_ws}"""
        assert lb.addk_ohem_select_supported(N, H, W, OH, OW, NC) == 1
        s = {'map': full(float('nan'), N, OH, OW), 'tau': full(float('nan'), 1), 'wkept': full(float('nan'), 1),
             'counts': full(-1, 2, dt=torch.int64), 'sel_ws': full(0x5a, int(lb.addk_ohem_select_ws_bytes(N, OH, OW)), dt=torch.uint8)}
        a = L.OhemSelectArgs()
        prefix(a)
        a.target, a.class_w, a.ignore_index = td.data_ptr(), wd.data_ptr() if weighted else None, 255
        a.thresh, a.min_kept_total = 0.7, max(1, int(wsum(arrs, 0)) // 16)
        a.pix_loss, a.tau, a.wsum_kept, a.counts, a.ws = (s[k].data_ptr() for k in ('map', 'tau', 'wkept', 'counts', 'sel_ws'))
        L.check(lb.addk_ohem_select(C.byref(a), st), 'ohem_select')
        return s

    lut = torch.arange(255, -1, -1, dtype=torch.uint8).to(dev)           # the reversed table of the label heads
    got = {}
    if kernel == 'score':
        assert lb.addk_score_upsample_supported(N, H, W, OH, OW, NC) == 1
        for weighted in (0, 1):
            wsd = full(float(wsum(arrs, weighted)), 1)
            for want_map in (0, 1):
                b = {'loss': full(0.25, 1), 'ent': full(0.5, 1), 'cm': torch.from_numpy(arrs['cm0']).to(dev),
                     'pred': full(77, N, OH, OW, dt=torch.uint8) if want_map else None,
                     'ws': full(float('nan'), int(lb.addk_score_upsample_ws_floats(N, OH, OW)))}
                a = L.ScoreUpsampleArgs()
                prefix(a)
                loss_binding(a, weighted, wsd)
                a.loss_out, a.ent_out, a.cm, a.ws = b['loss'].data_ptr(), b['ent'].data_ptr(), b['cm'].data_ptr(), b['ws'].data_ptr()
                a.pred_out = b['pred'].data_ptr() if want_map else None
                L.check(lb.addk_score_upsample(C.byref(a), st), 'score_upsample')
                torch.cuda.synchronize()
                got['%s/%s' % ('weighted' if weighted else 'plain', 'map' if want_map else 'nomap')] = hashes(b)
    elif kernel == 'gate':
        assert lb.addk_gate_upsample_supported(N, H, W, OH, OW, NC) == 1
        for thr in (0.2, 0.8):
            thd = full(thr, 1)
            for want_host in (0, 1):
                b = {'out': full(-7.0, N, 2), 'ws': full(0, int(lb.addk_gate_upsample_ws_bytes(N, OH, OW)), dt=torch.uint8)}
                host = torch.full((N, 2), -9.0).pin_memory() if want_host else None
                a = L.GateUpsampleArgs()
                prefix(a)
                a.max_thr, a.out, a.ws = thd.data_ptr(), b['out'].data_ptr(), b['ws'].data_ptr()
                a.out_host = host.data_ptr() if want_host else None
                L.check(lb.addk_gate_upsample(C.byref(a), st), 'gate_upsample')
                torch.cuda.synchronize()
                b['host'] = host
                got['thr%g/%s' % (thr, 'host' if want_host else 'nohost')] = hashes(b)
    elif kernel == 'ce':
        refused = lb.addk_ce_upsample_supported(N, H, W, OH, OW, NC) != 1
        for acc in (0, 1):
            wsd = full(float(wsum(arrs, acc)), 1)
            a, b = ce_args(acc, wsd)
            rc = lb.addk_ce_upsample_fwd_bwd(C.byref(a), st)
            assert refused == (rc != 0), '%s: addk_ce_upsample_supported and the launch disagree (rc %d)' % (name, rc)
            torch.cuda.synchronize()
            got['acc%d%s' % (acc, '/refused' if refused else '')] = hashes(b)
    elif kernel == 'ce_ohem':
        refused = lb.addk_ce_upsample_supported(N, H, W, OH, OW, NC) != 1
        for acc in (0, 1):
            s = select(acc)
            a, b = ce_args(acc, s['wkept'])
            o = L.CeUpsampleOhemArgs()
            o.ce, o.pix_loss, o.tau = a, s['map'].data_ptr(), s['tau'].data_ptr()
            rc = lb.addk_ce_upsample_ohem_fwd_bwd(C.byref(o), st)
            assert refused == (rc != 0), '%s: addk_ce_upsample_supported and the launch disagree (rc %d)' % (name, rc)
            torch.cuda.synchronize()
            b.update(s)
            got['acc%d%s' % (acc, '/refused' if refused else '')] = hashes(b)
    elif kernel == 'ce_kd':
        refused = lb.addk_ce_upsample_kd_supported(N, H, W, OH, OW, NC) != 1
        nvd = full(float(wsum(arrs, 0)), 1)
        for tld in LDS:
            yd = logits('t', tld)
            for mining in (0, 1):                                         # the mined launch is the class-weighted, accumulating one
                s = select(mining) if mining else None
                wsd = s['wkept'] if mining else full(float(wsum(arrs, 0)), 1)
                a, b = ce_args(mining, wsd, int(lb.addk_ce_upsample_kd_ws_floats(N, H, W)))
                b['kd'] = full(-3.0, 1)
                o = L.CeUpsampleKdArgs()
                o.ce, o.teacher, o.ld_teacher, o.alpha, o.temperature = a, yd.data_ptr(), tld, 0.5, 2.0
                o.nvalid, o.kd_out = nvd.data_ptr(), b['kd'].data_ptr()
                if mining:
                    o.pix_loss, o.tau = s['map'].data_ptr(), s['tau'].data_ptr()
                rc = lb.addk_ce_upsample_kd_fwd_bwd(C.byref(o), st)
                assert refused == (rc != 0), '%s: addk_ce_upsample_kd_supported and the launch disagree (rc %d)' % (name, rc)
                torch.cuda.synchronize()
                got['t%d/%s%s' % (tld, 'mined' if mining else 'all', '/refused' if refused else '')] = hashes(b)
    elif kernel == 'label':
        assert lb.addk_label_upsample_supported(N, H, W, OH, OW, NC) == 1
        for table in (None, lut):
            b = {'labels': full(77, N, OH, OW, dt=torch.uint8)}
            a = L.LabelUpsampleArgs()
            prefix(a)
            a.lut256, a.labels = table.data_ptr() if table is not None else None, b['labels'].data_ptr()
            L.check(lb.addk_label_upsample(C.byref(a), st), 'label_upsample')
            torch.cuda.synchronize()
            got['table' if table is not None else 'plain'] = hashes(b)
    elif kernel == 'gate_label':
        for thr, table in ((0.2, None), (0.8, lut)):
            thd = full(thr, 1)
            for want_host in (0, 1):
                b = {'out': full(-7.0, N, 2), 'ws': full(0, int(lb.addk_gate_upsample_ws_bytes(N, OH, OW)), dt=torch.uint8),
                     'labels': full(77, N, OH, OW, dt=torch.uint8)}
                host = torch.full((N, 2), -9.0).pin_memory() if want_host else None
                o = L.GateLabelUpsampleArgs()
                a = o.gate
                prefix(a)
                a.max_thr, a.out, a.ws = thd.data_ptr(), b['out'].data_ptr(), b['ws'].data_ptr()
                a.out_host = host.data_ptr() if want_host else None
                o.lut256, o.labels = table.data_ptr() if table is not None else None, b['labels'].data_ptr()
                L.check(lb.addk_gate_label_upsample(C.byref(o), st), 'gate_label_upsample')
                torch.cuda.synchronize()
                b['host'] = host
                got['thr%g/%s' % (thr, 'host' if want_host else 'nohost')] = hashes(b)
    elif kernel == 'profile':
        thd = torch.from_numpy(arrs['thr']).to(dev)
        for nthr in (0, 3, NTHR):
            assert lb.addk_profile_upsample_supported(N, H, W, OH, OW, NC, nthr) == 1
            for want_map in (0, 1):
                b = {'ent': full(-7.0, N), 'share': full(-7.0, N, nthr) if nthr else None, 'cm': torch.from_numpy(arrs['pcm0']).to(dev),
                     'pred': full(77, N, OH, OW, dt=torch.uint8) if want_map else None,
                     'ws': full(0, int(lb.addk_profile_upsample_ws_bytes(N, OH, OW)), dt=torch.uint8)}
                a = L.ProfileUpsampleArgs()
                prefix(a)
                a.target, a.thr, a.nthr = td.data_ptr(), thd.data_ptr() if nthr else None, nthr
                a.ent_out, a.share_out, a.cm = b['ent'].data_ptr(), b['share'].data_ptr() if nthr else None, b['cm'].data_ptr()
                a.pred_out, a.ws = b['pred'].data_ptr() if want_map else None, b['ws'].data_ptr()
                L.check(lb.addk_profile_upsample(C.byref(a), st), 'profile_upsample')
                torch.cuda.synchronize()
                got['nthr%d/%s' % (nthr, 'map' if want_map else 'nomap')] = hashes(b)
    else:
        assert kernel == 'views'
        assert lb.addk_label_views_upsample_supported(3, N, OH, OW, NC) == 1
        for launch, ld2, table in (('same_ld', ld, None), ('second_ld19', 19, lut)):
            v2, v3 = logits('v2', ld2), logits('v3', ld)
            b = {'labels': full(77, N, OH, OW, dt=torch.uint8)}
            a = L.LabelViewsArgs()
            for v, (t, vld, n0, mirror, weight) in zip(a.view, ((xd, ld, 0, 0, 0.5), (v2, ld2, 1, 1, 1.0), (v3, ld, 0, 0, 1.5))):
                v.logits, v.ld, v.n0, v.H, v.W, v.mirror, v.weight = t.data_ptr(), vld, n0, t.shape[1], t.shape[2], mirror, weight
            a.nview, a.N, a.C, a.OH, a.OW = 3, N, NC, OH, OW
            a.lut256, a.labels = table.data_ptr() if table is not None else None, b['labels'].data_ptr()
            L.check(lb.addk_label_views_upsample(C.byref(a), st), 'label_views_upsample')
            torch.cuda.synchronize()
            got[launch] = hashes(b)
    return got


def main():
    sys.path.insert(0, ROOT)
    import addk  # noqa: F401
    from addk import _lib as L
    import torch
    assert torch.cuda.is_available(), 'needs the MI355X'
    doc = {'about': 'sha256 of what addk_ce_upsample_fwd_bwd, addk_score_upsample and addk_gate_upsample write on RandomState-seeded inputs; '
                    'written by tests/tools/make_head_bits.py from the parent of the commit that gave the three heads one up-sampling walk',
           'about2': 'ce_ohem, ce_kd, label, gate_label, profile and views (inputs2: their further inputs) were added to the tool later and '
                     'recorded from the parent of the commit that split csrc/loss.hip by head family',
           'cases': []}
    for case in CASES:
        arrs, hin = make_inputs(case)
        arrs2, hin2 = make_inputs2(case)
        arrs.update(arrs2)
        rec = {'name': case[0], 'lo': list(case[1]), 'hi': list(case[2]), 'seed': case[3], 'inputs': hin, 'inputs2': hin2, 'runs': {}}
        for ld in LDS:
            for kernel in KERNELS:
                got = run_case(L, case, ld, kernel, arrs)
                rec['runs']['ld%d/%s' % (ld, kernel)] = got
                print(case[0], ld, kernel, hin[:12], ' '.join('%s:%s' % (ln, '/'.join(h[:8] for h in hs.values())) for ln, hs in got.items()), flush=True)
        doc['cases'].append(rec)
    out = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = out[0] if out else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
